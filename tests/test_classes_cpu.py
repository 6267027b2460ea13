"""The class dimension without a device: the float64 yardstick of tests/test_gpu_classes.py against numbers the reference itself
produced, and the inputs of its online-evaluation cases with the preconditions that make their counts well defined."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle
from tests.helpers import golden, seeded_input, seeded_labels

# (B, K, dims) of the online-evaluation cases: every class block (KB = 4, 8, 16, 32) on an odd shape below 256 voxels per class
# plane, and one shape of several workgroups per sample
EVAL_CASES = [(3, 2, (5, 7, 9)), (3, 5, (5, 7, 9)), (3, 8, (5, 7, 9)), (3, 9, (5, 7, 9)), (3, 17, (5, 7, 9)), (3, 32, (5, 7, 9)),
              (1, 5, (20, 33, 35))]
MIN_GAP = 1e-4


def top2_gap(logits):
    """largest minus second largest logit of every voxel, [B, spatial...]"""
    top = logits.topk(2, dim=1).values
    return top[:, 0] - top[:, 1]


def online_eval_case(b, k, dims):
    """(logits [B,K,...], target [B,1,...], tie voxel, the two bad-label voxels) of one online-evaluation case.
    Logits are seeded_input * 2; where the two largest of a voxel are closer than MIN_GAP the maximum is raised by 1e-2 (no
    voxel is dropped); one voxel carries an exact two-way tie at its maximum; labels are uniform in [0, K) with -1 and K planted
    at two voxels.  Voxels are flat indices into [B, spatial]."""
    spatial = int(np.prod(dims))
    logits = seeded_input((b, k) + dims, seed=300 + k + spatial).mul(2.0)
    close = top2_gap(logits) < MIN_GAP
    if bool(close.any()):
        top = logits.argmax(1, keepdim=True)
        logits.scatter_add_(1, top, close.unsqueeze(1).float() * 1e-2)
    flat = logits.view(b, k, spatial)
    tie = (b - 1, spatial // 2)                                  # (sample, voxel)
    lo, hi = (0, 1) if k == 2 else (1, k - 1)
    peak = float(flat[tie[0], :, tie[1]].max()) + 1.0
    flat[tie[0], lo, tie[1]] = peak
    flat[tie[0], hi, tie[1]] = peak
    target = seeded_labels((b, 1) + dims, k, seed=400 + k + spatial)
    bad = ((0, 3), (b - 1, spatial - 2))
    target.view(b, spatial)[bad[0]] = -1.0
    target.view(b, spatial)[bad[1]] = float(k)
    return logits, target, tie, bad


def hard_counts_torch(logits, target, seg=None):
    """[K, 3] tp / fp / fn of argmax(softmax) against the labels, in the reference's torch expressions (run_online_evaluation),
    for all K classes; `seg` replaces the argmax"""
    if seg is None:
        seg = F.softmax(logits, 1).argmax(1)
    tgt = target[:, 0]
    k = logits.shape[1]
    rows = [[((seg == c).float() * (tgt == c).float()).sum().item(), ((seg == c).float() * (tgt != c).float()).sum().item(),
             ((seg != c).float() * (tgt == c).float()).sum().item()] for c in range(k)]
    return np.array(rows, dtype=np.int64)


@pytest.mark.parametrize("tag,batch_dice", [("sample", False), ("batch", True)])
def test_float64_loss_reproduces_the_reference_golden(tag, batch_dice):
    """oracle.deep_supervision_loss on double logits against tests/golden/loss.npz (the reference's own fp32 run): loss to 2e-6,
    gradients to 2e-7.  The float64 values that the device tests compare with are the reference's up to its fp32 rounding."""
    g = golden("loss.npz")
    k = 4
    shapes = [(2, k, 8, 12, 10), (2, k, 4, 6, 5), (2, k, 2, 3, 5), (2, k, 1, 3, 5)]
    logits = [seeded_input(s, seed=50 + i).mul(2.0).double().requires_grad_(True) for i, s in enumerate(shapes)]
    targets = [seeded_labels((s[0], 1) + s[2:], k, seed=60 + i) for i, s in enumerate(shapes)]
    loss = oracle.deep_supervision_loss(logits, targets, oracle.ds_weights(5), batch_dice)
    assert loss.dtype == torch.float64
    print("%s: loss fp64 %.12f golden %.9f diff %.3g" % (tag, loss.item(), float(g[tag + "_loss"]), loss.item() - float(g[tag + "_loss"])))
    assert abs(loss.item() - float(g[tag + "_loss"])) < 2e-6
    loss.backward()
    for i, l in enumerate(logits):
        assert l.grad.dtype == torch.float64
        print("  g%d max abs diff %.3g" % (i, np.abs(l.grad.numpy() - g[tag + "_g%d" % i]).max()))
        np.testing.assert_allclose(l.grad.numpy(), g[tag + "_g%d" % i], rtol=0, atol=2e-7)


@pytest.mark.parametrize("b,k,dims", EVAL_CASES)
def test_online_evaluation_inputs_hold_their_preconditions(b, k, dims):
    """What makes the hard counts of a case independent of the last ulp of an exponential: the two largest logits of every voxel
    differ by at least 1e-4, except at one voxel with an exact two-way tie at the maximum, where the lower index wins in torch as
    in the kernel (first maximum).  The voxels labelled -1 and K are false positives of the predicted class and nobody's false
    negatives in the reference's expressions."""
    logits, target, tie, bad = online_eval_case(b, k, dims)
    spatial = int(np.prod(dims))
    assert logits.shape == (b, k) + dims and target.shape == (b, 1) + dims
    gap = top2_gap(logits).view(b, spatial)
    assert float(gap[tie]) == 0.0
    vals = logits.view(b, k, spatial)[tie[0], :, tie[1]]
    lo = 0 if k == 2 else 1
    assert int((vals == vals.max()).sum()) == 2 and int(vals.argmax()) == lo
    assert int(F.softmax(logits, 1).argmax(1).view(b, spatial)[tie]) == lo
    gap[tie] = float("inf")
    print("K %d: smallest top-2 gap %.3g" % (k, float(gap.min())))
    assert float(gap.min()) >= MIN_GAP
    tgt = target.view(b, spatial)
    assert float(tgt[bad[0]]) == -1.0 and float(tgt[bad[1]]) == float(k) and tie not in bad
    inside = (tgt >= 0) & (tgt < k)
    assert int((~inside).sum()) == 2 and bool((tgt == tgt.round()).all())
    assert sorted(tgt[inside].unique().tolist()) == list(range(k))               # every class occurs
    want = hard_counts_torch(logits, target)
    seg = F.softmax(logits, 1).argmax(1).view(b, spatial)
    clean = target.clone()
    for v in bad:
        clean.view(b, spatial)[v] = seg[v].float()                              # the same voxels as true positives
    base = hard_counts_torch(logits, clean)
    delta = np.zeros_like(want)
    for v in bad:
        delta[int(seg[v])] += np.array([-1, 1, 0])
    assert np.array_equal(want, base + delta)
    assert want.sum() >= b * spatial                                             # every voxel is a tp or an fp of its prediction
    assert (want[:, 0] + want[:, 1]).sum() == b * spatial
