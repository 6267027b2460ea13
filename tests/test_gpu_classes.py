"""The class dimension of the default training path against float64: the 1x1x1 heads, the fused softmax Dice+CE loss (K8) and
the online evaluation counts, across every class block (KB = 4, 8, 16, 32; the heads make a second pass over the classes from
K = 17), labels outside [0, K), the fp32 -> fp64 partial-sum flushes that only long volumes reach, and the whole chain at
k = 7 and k = 20.  Every reference is a plain float64 evaluation with torch on the CPU (oracle.dc_ce_loss, region_loss_fp64,
F.conv3d); tests/test_classes_cpu.py ties that yardstick to the reference's own numbers.

Not covered here: the `& 127` flush of online_eval_regions_kernel needs 67 M voxels per sample, too large for a unit test."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle
from tests.helpers import seeded_input, seeded_labels
from tests.test_classes_cpu import EVAL_CASES, online_eval_case, hard_counts_torch, top2_gap
from tests.test_regions_cpu import region_loss_fp64

pytestmark = pytest.mark.gpu

LOSS_SHAPES = ((2, 7, 9, 11), (3, 5, 7, 5), (2, 8, 12, 16), (1, 4, 4, 4))       # (B, spatial dims)
LOSS_CONFIGS = ((False, 0.), (True, 1e-5), (False, 1e-5))                         # (batch_dice, smooth)
WEIGHT = 0.75
LRELU_SLOPE = 0.01


def _stream():
    return torch.cuda.current_stream().cuda_stream


def class_block(k):
    """KB of DISPATCH_LK (loss.hip)"""
    return 4 if k <= 4 else 8 if k <= 8 else 16 if k <= 16 else 32


def softmax_loss(logits, target, batch_dice, smooth, weight=WEIGHT, with_grad=True, loss=None):
    """one scale through e2e_dc_ce_reduce / e2e_dc_ce_grad on device tensors; dlogits starts as NaN; `loss` is the device scalar
    the value is added to (a fresh zero by default).  Returns (loss on the CPU, dlogits on the CPU or None, the device scalar)."""
    from e2enet_medical_amd._lib import lib
    L = lib()
    b, k = logits.shape[:2]
    spatial = logits[0, 0].numel()
    ws = torch.empty(L.loss_ws_bytes(b, k) // 8, dtype=torch.float64, device="cuda")
    dl = torch.full_like(logits, float("nan")) if with_grad else None
    if loss is None:
        loss = torch.zeros(1, dtype=torch.float32, device="cuda")
    L.dc_ce_reduce(logits.data_ptr(), target.data_ptr(), ws.data_ptr(), b, k, spatial, _stream())
    L.dc_ce_grad(logits.data_ptr(), target.data_ptr(), ws.data_ptr(), weight, 1 if batch_dice else 0, smooth,
                 None if dl is None else dl.data_ptr(), loss.data_ptr(), b, k, spatial, _stream())
    torch.cuda.synchronize()
    return loss.cpu(), (None if dl is None else dl.cpu()), loss


def softmax_loss_fp64(logits, target, batch_dice, smooth):
    """(loss, dloss/dlogits) of oracle.dc_ce_loss on double logits"""
    leaf = logits.double().requires_grad_(True)
    loss = oracle.dc_ce_loss(leaf, target, batch_dice, smooth)
    loss.backward()
    return loss.detach(), leaf.grad


def _loss_inputs(k, shape, seed_labels):
    b, spatial = shape[0], int(np.prod(shape[1:]))
    logits = seeded_input((b, k) + shape[1:], seed=7 * k + spatial).mul(2.0)
    flat = logits.view(-1)
    flat[3], flat[11], flat[-1] = 100.0, -100.0, 100.0
    target = seeded_labels((b, 1) + shape[1:], k, seed=seed_labels + k + spatial)
    return logits, target


def _assert_loss_bars(got_loss, got_grad, ref_loss, ref_grad, what):
    """the bars of test_loss_kernels and of the region fp64 test: value 2e-6, gradient 2e-8 + 1e-4 of the largest gradient"""
    want = WEIGHT * ref_grad
    lerr = abs(got_loss.item() - WEIGHT * ref_loss.item())
    gerr = float((got_grad.double() - want).abs().max())
    print("%s: loss %.9f ref %.9f err %.3g | grad err %.3g of max %.3g" % (what, got_loss.item(), WEIGHT * ref_loss.item(), lerr,
                                                                          gerr, float(want.abs().max())))
    assert torch.isfinite(got_loss).all() and torch.isfinite(got_grad).all(), what
    assert lerr < 2e-6, (what, got_loss.item(), WEIGHT * ref_loss.item())
    assert gerr < 2e-8 + 1e-4 * float(want.abs().max()), (what, gerr)


# ------------------------------------------------------------------------------------------------ A: softmax loss
@pytest.mark.parametrize("k", [2, 3, 4, 5, 8, 9, 16, 17, 32])
def test_softmax_loss_kernels_against_float64(k):
    """K on both sides of every class block (KB = 4: 2, 3, 4; 8: 5, 8; 16: 9, 16; 32: 17, 32), odd sizes and one scale below 256
    voxels, logits of +-100 planted, per-sample and batch dice with and without smoothing at weight 0.75.  Loss against float64
    to 2e-6, gradients to 2e-8 + 1e-4 of the largest gradient, every gradient element written; dlogits = NULL gives the same value
    bit for bit; a second call onto the same loss scalar gives exactly twice the value (the += of the deep-supervision scales)."""
    for shape in LOSS_SHAPES:
        logits, target = _loss_inputs(k, shape, 500)
        assert float(target.min()) >= 0 and float(target.max()) <= k - 1
        if k == 32 and shape == (1, 4, 4, 4):
            assert len(target.unique()) < k - 2                      # several classes absent from the sample
        lg, tg = logits.cuda(), target.cuda()
        for bd, smooth in LOSS_CONFIGS:
            ref_loss, ref_grad = softmax_loss_fp64(logits, target, bd, smooth)
            la, ga, dev = softmax_loss(lg, tg, bd, smooth)
            _assert_loss_bars(la, ga, ref_loss, ref_grad, "K %d %s bd %d smooth %g" % (k, shape, bd, smooth))
            lv, _, _ = softmax_loss(lg, tg, bd, smooth, with_grad=False)
            assert torch.equal(la, lv), (shape, bd, smooth, la.item(), lv.item())
            l2, g2, _ = softmax_loss(lg, tg, bd, smooth, loss=dev)
            assert l2.item() == 2.0 * la.item() and torch.equal(g2, ga), (shape, bd, smooth, la.item(), l2.item())


# ------------------------------------------------------------------------------------------------ B: labels outside [0, K)
@pytest.mark.parametrize("k", [3, 5, 9, 17, 4, 32])
def test_softmax_loss_turns_nan_for_a_label_outside_the_classes(k):
    """A single label of K, KB - 1 (where the class block is padded past K: a padded slot holds -INF), 40 or -1: the loss is NaN,
    not +-Inf, from the full call and from the value-only call.  The same tensors without it: a finite loss inside the bars.
    (dlogits under a bad label are unspecified.)"""
    shape = (2, 5, 7, 3)
    logits, target = _loss_inputs(k, shape, 600)
    lg = logits.cuda()
    kb = class_block(k)
    bad_labels = [k] + ([kb - 1] if kb - 1 > k else []) + [40, -1]
    assert (k in (4, 32)) == (kb == k)
    for bd, smooth in ((False, 0.), (True, 1e-5)):
        ref_loss, ref_grad = softmax_loss_fp64(logits, target, bd, smooth)
        la, ga, _ = softmax_loss(lg, target.cuda(), bd, smooth)
        _assert_loss_bars(la, ga, ref_loss, ref_grad, "K %d clean bd %d" % (k, bd))
        for bad in bad_labels:
            planted = target.clone()
            planted.view(-1)[17] = float(bad)
            tg = planted.cuda()
            full, _, _ = softmax_loss(lg, tg, bd, smooth)
            value, _, _ = softmax_loss(lg, tg, bd, smooth, with_grad=False)
            print("K %d label %d: loss %r value-only %r" % (k, bad, full.item(), value.item()))
            assert torch.isnan(full).all(), (k, bad, full.item())
            assert torch.isnan(value).all(), (k, bad, value.item())


# ------------------------------------------------------------------------------------------------ C: online evaluation
@pytest.mark.parametrize("b,k,dims", EVAL_CASES)
def test_online_evaluation_counts_are_exact(b, k, dims):
    """e2e_online_eval_counts against the reference's torch expressions for all K classes, counts pre-filled with -1: every class
    block, a shape of several workgroups, an exact two-way tie at the maximum (the lower index wins) and labels -1 and K (false
    positives of the predicted class, no false negatives).  The preconditions on the inputs are asserted again here."""
    from e2enet_medical_amd._lib import lib
    logits, target, tie, bad = online_eval_case(b, k, dims)
    spatial = int(np.prod(dims))
    gap = top2_gap(logits).view(b, spatial)
    assert float(gap[tie]) == 0.0
    gap[tie] = float("inf")
    assert float(gap.min()) >= 1e-4
    assert float(target.view(b, spatial)[bad[0]]) == -1.0 and float(target.view(b, spatial)[bad[1]]) == float(k)
    want = hard_counts_torch(logits, target)
    counts = torch.full((k, 3), -1, dtype=torch.int64, device="cuda")
    lg, tg = logits.cuda(), target.cuda()
    lib().online_eval_counts(lg.data_ptr(), tg.data_ptr(), counts.data_ptr(), b, k, spatial, _stream())
    torch.cuda.synchronize()
    got = counts.cpu().numpy()
    assert np.array_equal(got, want), (k, got - want)
    assert int((got[:, 0] + got[:, 1]).sum()) == b * spatial         # every voxel is a tp or an fp of its prediction


# ------------------------------------------------------------------------------------------------ D: heads
HEAD_CASES = [
    # (B, C, K, dims, normed source)     spatial % 4 == 0: float4 kernels, else the scalar ones
    (1, 1, 1, (3, 5, 7), True),
    (2, 7, 2, (2, 4, 6), False),
    (1, 16, 5, (4, 6, 8), True),
    (2, 17, 8, (3, 5, 7), False),
    (1, 33, 9, (2, 4, 6), True),
    (2, 12, 16, (3, 5, 7), True),
    (2, 7, 17, (2, 4, 6), True),
    (1, 17, 17, (3, 5, 7), False),
    (2, 33, 20, (4, 6, 8), True),
    (1, 16, 32, (3, 5, 7), True),
    (1, 9, 33, (2, 4, 6), False),
]


def _head_inputs(B, C, K, spatial, normed, seed):
    """x [B,C,S], per-(n,c) scale / shift (None for a raw source), w [K,C], dlogits [B,K,S]"""
    x = seeded_input((B, C, spatial), seed=seed)
    scale = shift = None
    if normed:
        scale = 0.5 + torch.rand(B * C, generator=torch.Generator().manual_seed(seed + 1))
        scale[::3] *= -1.0                                            # negative gamma happens in trained nets
        shift = seeded_input((B * C,), seed=seed + 2) * 0.3
    w = seeded_input((K, C), seed=seed + 3) * 0.3
    dl = seeded_input((B, K, spatial), seed=seed + 4)
    return x, scale, shift, w, dl


def _head_value_fp64(x, scale, shift):
    """what the head reads: lrelu(scale * x + shift) of a normalised source, x of a raw one, in float64"""
    z = x.double()
    if scale is not None:
        b, c = x.shape[:2]
        z = F.leaky_relu(z * scale.double().view(b, c, 1) + shift.double().view(b, c, 1), LRELU_SLOPE)
    return z


def _ptr(t):
    return None if t is None else t.data_ptr()


def _head_wgrad(x, scale, shift, dl, B, C, K, spatial):
    from e2enet_medical_amd._lib import lib
    L = lib()
    ws = torch.empty(L.head1x1_wgrad_ws_bytes(B, C, K, spatial) // 8, dtype=torch.float64, device="cuda")
    dw = torch.full((K, C), float("nan"), dtype=torch.float32, device="cuda")
    L.head1x1_wgrad(x.data_ptr(), _ptr(scale), _ptr(shift), LRELU_SLOPE, dl.data_ptr(), dw.data_ptr(), ws.data_ptr(), B, C, K,
                    spatial, _stream())
    torch.cuda.synchronize()
    return dw.cpu()


@pytest.mark.parametrize("B,C,K,dims,normed", HEAD_CASES)
def test_heads_against_float64_across_class_blocks(B, C, K, dims, normed):
    """Every class block of the head kernels (KB = 4, 8, 16) and the second and third pass over the classes (K = 17, 20, 32, 33)
    in the float4 form (spatial % 4 == 0) and the scalar form; C on both sides of the 16-channel summation block and of the
    8-channel groups of the float4 weight gradient (C = 1, 7, 9, 12, 17, 33); raw sources (no scale) beside normalised ones.
    Forward, data gradient written into NaN (accumulate = 0) and added onto a prefill (accumulate = 1), weight gradient; bars of
    test_head_fwd_bwd against float64, scaled by max(1, max |ref|): 1e-5, 1e-5, 2e-4."""
    from e2enet_medical_amd._lib import lib
    L = lib()
    spatial = int(np.prod(dims))
    x, scale, shift, w, dl = _head_inputs(B, C, K, spatial, normed, 700 + 10 * K + C)
    z = _head_value_fp64(x, scale, shift).requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    ref = F.conv1d(z, w64.view(K, C, 1))                              # a 1x1x1 convolution over flattened voxels
    ref.backward(dl.double())
    ref = ref.detach()
    xd, wd, dld = x.cuda(), w.cuda(), dl.cuda()
    sd, td = (None, None) if scale is None else (scale.cuda(), shift.cuda())

    out = torch.full((B, K, spatial), float("nan"), device="cuda")
    L.head1x1_fwd(xd.data_ptr(), _ptr(sd), _ptr(td), LRELU_SLOPE, wd.data_ptr(), out.data_ptr(), B, C, K, spatial, _stream())
    err = float((out.cpu().double() - ref).abs().max())
    print("fwd err %.3g of max %.3g" % (err, float(ref.abs().max())))
    assert err < 1e-5 * max(1.0, float(ref.abs().max())), ("forward", err)

    bar = 1e-5 * max(1.0, float(z.grad.abs().max()))
    dx = torch.full((B, C, spatial), float("nan"), device="cuda")
    L.head1x1_dgrad(dld.data_ptr(), wd.data_ptr(), dx.data_ptr(), 0, B, C, K, spatial, _stream())
    err = float((dx.cpu().double() - z.grad).abs().max())
    print("dgrad err %.3g of max %.3g" % (err, float(z.grad.abs().max())))
    assert err < bar, ("data gradient", err)                          # (NaN left anywhere fails the comparison)
    prefill = seeded_input((B, C, spatial), seed=5)
    dx = prefill.cuda()
    L.head1x1_dgrad(dld.data_ptr(), wd.data_ptr(), dx.data_ptr(), 1, B, C, K, spatial, _stream())
    err = float((dx.cpu().double() - (prefill.double() + z.grad)).abs().max())
    print("dgrad (accumulate) err %.3g" % err)
    assert err < 1e-5 * max(1.0, float((prefill.double() + z.grad).abs().max())), ("accumulated data gradient", err)

    dw = _head_wgrad(xd, sd, td, dld, B, C, K, spatial)
    err = float((dw.double() - w64.grad).abs().max())
    print("wgrad err %.3g of max %.3g" % (err, float(w64.grad.abs().max())))
    assert err < 2e-4 * max(1.0, float(w64.grad.abs().max())), ("weight gradient", err)


# ------------------------------------------------------------------------------------------------ E: long volumes
LONG_LOSS = 512 * 256 * 33 + 37       # voxels of one sample: a thread of the 512-block loss grid makes a 33rd iteration
LONG_HEAD = 128 * 256 * 65 + 3        # a thread of the 128-block scalar weight-gradient grid makes a 65th


def _assert_long_loss(got_loss, got_grad, ref_loss, ref_grad, what):
    """loss bar of the short shapes; the gradients scale with 1 / (B S), so the bar is relative only: 1e-4 of the largest"""
    want = WEIGHT * ref_grad
    lerr = abs(got_loss.item() - WEIGHT * ref_loss.item())
    gerr = float((got_grad.double() - want).abs().max())
    print("%s: loss err %.3g | grad err %.3g of max %.3g" % (what, lerr, gerr, float(want.abs().max())))
    assert torch.isfinite(got_grad).all()
    assert lerr < 2e-6, (what, got_loss.item(), WEIGHT * ref_loss.item())
    assert gerr < 1e-4 * float(want.abs().max()), (what, gerr)


def test_softmax_loss_partial_sum_flush_on_a_long_volume():
    """K = 3 on 4 325 413 voxels: every thread of dc_ce_reduce_kernel passes the `& 31` flush of its fp32 partial sums into fp64"""
    s = LONG_LOSS
    assert s % 4 != 0 and s > 32 * 512 * 256
    logits = seeded_input((1, 3, s), seed=801).mul(2.0)
    target = seeded_labels((1, 1, s), 3, seed=802)
    ref_loss, ref_grad = softmax_loss_fp64(logits, target, False, 1e-5)
    la, ga, _ = softmax_loss(logits.cuda(), target.cuda(), False, 1e-5)
    _assert_long_loss(la, ga, ref_loss, ref_grad, "softmax, S = %d" % s)


def test_region_loss_partial_sum_flush_on_a_long_volume():
    """R = 1 in label form on the same length: 1 081 354 groups of four voxels, threads of dc_bce_reduce_kernel pass the `& 7` flush"""
    from tests.test_gpu_regions import kernel_loss
    from tests.test_regions_cpu import multihot_np
    s = LONG_LOSS
    assert (s + 3) // 4 > 8 * 512 * 256
    logits = seeded_input((1, 1, s), seed=803).mul(2.0)
    labels = seeded_labels((1, 1, s), 4, seed=804)
    sets = [(2, 3)]
    y = torch.from_numpy(multihot_np(labels.numpy(), sets))
    ref_loss, ref_grad = region_loss_fp64(logits, y, False, 1e-5)
    la, ga = kernel_loss(logits.cuda(), labels.cuda(), (0b1100,), False, 1e-5, WEIGHT)
    _assert_long_loss(la, ga, ref_loss, ref_grad, "region, S = %d" % s)


def test_head_weight_gradient_partial_sum_flush_on_a_long_volume():
    """C = 3, K = 17 on 2 129 923 voxels (odd: the scalar kernel, two passes over the classes): its threads pass the `& 63` flush"""
    s, B, C, K = LONG_HEAD, 1, 3, 17
    assert s % 4 != 0 and s > 64 * 128 * 256
    x, scale, shift, _, _ = _head_inputs(B, C, K, s, True, 805)
    dl = seeded_input((B, K, s), seed=806)
    ref = torch.einsum("bks,bcs->kc", dl.double(), _head_value_fp64(x, scale, shift))
    dw = _head_wgrad(x.cuda(), scale.cuda(), shift.cuda(), dl.cuda(), B, C, K, s)
    err = float((dw.double() - ref).abs().max())
    print("wgrad err %.3g of max %.3g" % (err, float(ref.abs().max())))
    assert err < 2e-4 * max(1.0, float(ref.abs().max())), err


# ------------------------------------------------------------------------------------------------ F: whole chain
@pytest.mark.parametrize("k", [7, 20])
def test_tiny_engine_fastpath_matches_oracle_with_more_classes(k):
    """head -> softmax Dice+CE -> backward of the tiny network at k = 7 (KB = 8) and k = 20 (loss KB = 32, two head passes) at
    the bars of test_tiny_engine_fastpath_matches_oracle_all_grads, and Engine.online_eval_counts against torch on the batch.
    A network's logits cannot be nudged apart: where the two largest of a voxel are closer than 1e-6 (16 ulp of a float32 below
    1; the exponentials of both implementations are good to a few ulp) either of the two may be the prediction, everywhere else
    the counts are exact.  No voxel is left out.  Measured: one such voxel at k = 20 (gap 9.98e-7), none at k = 7 (6.4e-6)."""
    import itertools
    from tests.test_gpu_net import engine_fastpath_vs_oracle
    eng, target = engine_fastpath_vs_oracle(k)
    logits = eng.heads[0].out.data.cpu()
    gap = top2_gap(logits)
    close = torch.nonzero(gap < 1e-6).tolist()
    print("k %d: smallest top-2 gap of the network's logits %.3g, %d voxel(s) below 1e-6" % (k, float(gap.min()), len(close)))
    assert len(close) <= 4
    seg = F.softmax(logits, 1).argmax(1)
    top2 = logits.topk(2, dim=1).indices
    candidates = []
    for choice in itertools.product((0, 1), repeat=len(close)):
        s = seg.clone()
        for (n, z, y, x), c in zip(close, choice):
            s[n, z, y, x] = top2[n, c, z, y, x]
        candidates.append(hard_counts_torch(logits, target, s))
    got = eng.online_eval_counts(target.cuda()).cpu().numpy()
    assert any(np.array_equal(got, c) for c in candidates), got - candidates[0]


# ------------------------------------------------------------------------------------------------ G: refusals
def test_class_counts_outside_the_limits_are_refused_before_any_launch():
    """K = 33 and K = 1 through DC_and_CE_loss raise the library's error that names the limit; K = 33 through online_eval_counts
    too; the arguments are checked before the workspace is zeroed or a kernel is launched, so every buffer keeps its fill."""
    from e2enet_medical_amd._lib import lib, E2EError
    from e2enet_medical_amd.training.loss_functions.dice_loss import DC_and_CE_loss
    L = lib()
    fn = DC_and_CE_loss({'batch_dice': False, 'smooth': 1e-5, 'do_bg': False}, {})
    for k in (33, 1):
        logits = seeded_input((1, k, 2, 3, 4), seed=k).cuda()
        target = torch.zeros((1, 1, 2, 3, 4), device="cuda")
        with pytest.raises(E2EError, match="2 <= K <= 32"):
            fn(logits, target)
        ws = torch.full((3 * k + 1,), 7.0, dtype=torch.float64, device="cuda")
        dl = torch.full_like(logits, 7.0)
        loss = torch.full((1,), 7.0, device="cuda")
        with pytest.raises(E2EError, match="2 <= K <= 32"):
            L.dc_ce_reduce(logits.data_ptr(), target.data_ptr(), ws.data_ptr(), 1, k, 24, _stream())
        with pytest.raises(E2EError, match="2 <= K <= 32"):
            L.dc_ce_grad(logits.data_ptr(), target.data_ptr(), ws.data_ptr(), 1.0, 0, 1e-5, dl.data_ptr(), loss.data_ptr(), 1, k, 24,
                         _stream())
        torch.cuda.synchronize()
        assert bool((ws == 7.0).all()) and bool((dl == 7.0).all()) and loss.item() == 7.0
    logits = seeded_input((1, 33, 2, 3, 4), seed=33).cuda()
    target = torch.zeros((1, 1, 2, 3, 4), device="cuda")
    counts = torch.full((33, 3), -1, dtype=torch.int64, device="cuda")
    with pytest.raises(E2EError, match="2 <= K <= 32"):
        L.online_eval_counts(logits.data_ptr(), target.data_ptr(), counts.data_ptr(), 1, 33, 24, _stream())
    torch.cuda.synchronize()
    assert bool((counts == -1).all())
