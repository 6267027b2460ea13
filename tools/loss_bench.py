#!/usr/bin/env python
"""Loss-kernel micro-benchmark on the GPU (diagnostic): the two launches of the softmax Dice+CE loss (K8, K classes) beside the
two launches of the region Dice+BCE loss (K8r, R regions, both target forms) at one full-resolution shape.  Prints time per
launch and achieved bytes per second over the algorithmic bytes (every logit read once per pass, the target once per pass,
every gradient written once).   python tools/loss_bench.py [B] [D] [K] [R]     (default 2 128 4 3)"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from e2enet_medical_amd._lib import lib          # noqa: E402


def algorithmic_bytes(B, C, S, target_channels):
    """(reduce, grad): reduce reads the logits and the target; grad reads both again and writes the gradient"""
    logits, target = 4 * B * C * S, 4 * B * target_channels * S
    return logits + target, 2 * logits + target


def main(argv):
    B, D, K, R = [int(a) if i < len(argv) else d for i, (a, d) in enumerate(zip(argv + [None] * 4, (2, 128, 4, 3)))]
    assert torch.cuda.is_available(), "loss_bench needs a GPU"
    L, dev, S = lib(), torch.device("cuda"), D * D * D
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(0)
    labels = torch.randint(0, min(K, R + 1), (B, 1, D, D, D), generator=g).float().to(dev)
    words = torch.tensor([((1 << (R + 1)) - 1) & ~((1 << (r + 1)) - 1) for r in range(R)], dtype=torch.int32, device=dev)   # nested regions
    multihot = torch.empty((B, R, D, D, D), dtype=torch.float32, device=dev)
    L.seg_to_regions(labels.data_ptr(), words.data_ptr(), multihot.data_ptr(), B, R, S, st)
    loss = torch.zeros(1, dtype=torch.float32, device=dev)
    cases = {}
    lk = torch.randn((B, K, D, D, D), generator=g).to(dev)
    dk, wk = torch.empty_like(lk), torch.empty(L.loss_ws_bytes(B, K) // 8, dtype=torch.float64, device=dev)
    cases["dc_ce_reduce"] = (lambda: L.dc_ce_reduce(lk.data_ptr(), labels.data_ptr(), wk.data_ptr(), B, K, S, st), algorithmic_bytes(B, K, S, 1)[0])
    cases["dc_ce_grad"] = (lambda: L.dc_ce_grad(lk.data_ptr(), labels.data_ptr(), wk.data_ptr(), 1.0, 0, 1e-5, dk.data_ptr(), loss.data_ptr(),
                                                B, K, S, st), algorithmic_bytes(B, K, S, 1)[1])
    lr = torch.randn((B, R, D, D, D), generator=g).to(dev)
    dr, wr = torch.empty_like(lr), torch.empty(L.loss_ws_bytes(B, R) // 8, dtype=torch.float64, device=dev)
    for tag, tgt, wp, ch in (("labels", labels, words.data_ptr(), 1), ("multihot", multihot, None, R)):
        cases["dc_bce_reduce[%s]" % tag] = (lambda tgt=tgt, wp=wp: L.dc_bce_reduce(lr.data_ptr(), tgt.data_ptr(), wp, wr.data_ptr(), B, R, S, st),
                                            algorithmic_bytes(B, R, S, ch)[0])
        cases["dc_bce_grad[%s]" % tag] = (lambda tgt=tgt, wp=wp: L.dc_bce_grad(lr.data_ptr(), tgt.data_ptr(), wp, wr.data_ptr(), 1.0, 0, 0.0,
                                                                               dr.data_ptr(), loss.data_ptr(), B, R, S, st),
                                          algorithmic_bytes(B, R, S, ch)[1])
    for fn, _ in cases.values():                 # warm-up: code objects, caches
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    rounds, iters = 5, 40                        # the cases alternate round by round; the best round of each is reported
    best = {n: float("inf") for n in cases}
    for _ in range(rounds):
        for n, (fn, _) in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            best[n] = min(best[n], e0.elapsed_time(e1) / iters)
    out = {"shape": [B, D, D, D], "K": K, "R": R, "kernels": {}}
    for n, (_, nbytes) in cases.items():
        out["kernels"][n] = {"ms": round(best[n], 4), "bytes": nbytes, "GB_per_s": round(nbytes / best[n] / 1e6, 1)}
        print("%-26s %8.4f ms  %7.1f MB  %7.1f GB/s" % (n, best[n], nbytes / 1e6, nbytes / best[n] / 1e6))
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1:])
