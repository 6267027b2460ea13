#!/usr/bin/env python
"""Surface-distance scoring benchmark (diagnostic, not gated): one synthetic case of K labels at the shape predict_3D is benchmarked
at, scored for HD / HD95 / ASD / ASSD / NSD by the device path (evaluation/surface_distance.py, csrc/surface.hip) and by the host
restatement of medpy's algorithm (tests/surface_oracle.py: one scipy distance_transform_edt per label and direction).

   python tools/surface_bench.py device [D H W K]      device time per label pair (events; inside the label's bounding box, and one
                                                       pair over the whole volume) and for the whole case with the upload
   python tools/surface_bench.py host [D H W K] [N]    host time of the first N label pairs (default 2) and the case extrapolated
(default 220 400 400 16).  The two modes are separate commands so that each runs under its own time limit; each prints one JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SPACING, TOLERANCE = (2.0, 0.8, 0.8), 2.0


def synthetic_case(D, H, W, K):
    """(prediction, ground truth): K - 1 ellipsoidal organs on a grid of centres, the prediction's offset and rescaled, plus
    0.2 % of stray voxels of the label in the prediction, within twice the organ's radii"""
    rng = np.random.RandomState(0)
    z, y, x = [(np.arange(n, dtype=np.float32) + 0.5) / n for n in (D, H, W)]
    out = []
    for side in range(2):
        m = np.zeros((D, H, W), np.uint8)
        for l in range(1, K):
            c = (0.2 + 0.6 * ((l * 7) % 5) / 4, 0.15 + 0.7 * ((l * 3) % 4) / 3, 0.15 + 0.7 * (l % 4) / 3)
            r = (0.08 + 0.01 * (l % 3) + 0.01 * side, 0.07 + 0.005 * side, 0.08 - 0.01 * side)
            sl = [slice(max(0, int((cc - rr) * n)), min(n, int((cc + rr) * n) + 2)) for cc, rr, n in zip(c, r, (D, H, W))]
            q = (((z[sl[0]] - c[0] - 0.01 * side) / r[0]) ** 2)[:, None, None] + (((y[sl[1]] - c[1]) / r[1]) ** 2)[None, :, None] + \
                (((x[sl[2]] - c[2] + 0.01 * side) / r[2]) ** 2)[None, None, :]
            m[sl[0], sl[1], sl[2]][q <= 1.0] = l
            if side == 0:
                wide = tuple(slice(max(0, int((cc - 2 * rr) * n)), min(n, int((cc + 2 * rr) * n))) for cc, rr, n in zip(c, r, (D, H, W)))
                box = m[wide]
                box[(rng.rand(*box.shape) < 0.002) & (box == 0)] = l
        out.append(m)
    return out[0], out[1]


def main(argv):
    mode = argv[0] if argv else "device"
    nums = [int(a) for a in argv[1:]]
    D, H, W, K = (nums + [220, 400, 400, 16][len(nums):])[:4]
    test, ref = synthetic_case(D, H, W, K)
    labels = list(range(K))
    rec = {"mode": mode, "shape": [D, H, W], "labels": K, "spacing": SPACING, "nsd_tolerance": TOLERANCE}
    if mode == "host":
        from tests import surface_oracle as so
        n = nums[4] if len(nums) > 4 else 2
        times = []
        for l in labels[1:1 + n]:
            t0 = time.perf_counter()
            m = so.metrics(test == l, ref == l, SPACING, TOLERANCE)
            times.append(time.perf_counter() - t0)
            print("host label %d: %.2f s  HD95 %.4f" % (l, times[-1], m["Hausdorff Distance 95"]), flush=True)
        rec.update(label_pairs_timed=n, s_per_label_pair=round(float(np.mean(times)), 3), s_per_case_extrapolated=round(float(np.mean(times)) * K, 1))
    else:
        import torch
        from e2enet_medical_amd.evaluation.surface_distance import SurfaceScorer, surface_distance_metrics
        assert torch.cuda.is_available(), "surface_bench device needs a GPU"
        surface_distance_metrics(test[:8], ref[:8], labels[:2], SPACING, TOLERANCE)                 # code objects, allocator
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = surface_distance_metrics(test, ref, labels, SPACING, TOLERANCE)
        torch.cuda.synchronize()
        case_s = time.perf_counter() - t0
        sc = SurfaceScorer(test, ref, SPACING)
        per = []
        for l in labels:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            sc.metrics(l, TOLERANCE)
            e1.record()
            torch.cuda.synchronize()
            per.append(e0.elapsed_time(e1))
        whole = SurfaceScorer(test, ref, SPACING, crop=False)          # the kernels' own rate: one label pair over the whole volume
        whole.metrics(1, TOLERANCE)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        whole.metrics(2, TOLERANCE)
        e1.record()
        torch.cuda.synchronize()
        rec.update(ms_per_label_pair_whole_volume=round(e0.elapsed_time(e1), 2))
        rec.update(ms_per_label_pair=round(float(np.median(per)), 2), ms_per_label_pair_max=round(float(max(per)), 2),
                   s_per_case_with_upload=round(case_s, 3), hd95={str(l): round(res[l]["Hausdorff Distance 95"], 4) for l in labels[:4]})
    print(json.dumps(rec))


if __name__ == "__main__":
    main(sys.argv[1:])
