#!/usr/bin/env python
"""Connected-component post-processing benchmark (diagnostic, not gated): "remove all but the largest connected component" on the
synthetic case tools/surface_bench.py builds (K - 1 ellipsoidal organs plus 0.2 % stray voxels per label), by the device path
(postprocessing/connected_components.py, csrc/components.hip) and by the host restatement of the reference's function
(tests/cc_oracle.py: one scipy.ndimage.label over the whole volume per class entry).

   python tools/postprocessing_bench.py device [D H W K]      device time per class entry (events, the volume resident) and for the
                                                              whole case: every class separately, with the upload and the download
   python tools/postprocessing_bench.py host [D H W K] [N]    host time of the first N class entries (default 2), single-threaded,
                                                              and the case extrapolated
(default 220 400 400 16).  The two modes are separate commands so that each runs under its own time limit; each prints one JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.surface_bench import synthetic_case          # noqa: E402

VOLUME_PER_VOXEL = 2.0 * 0.8 * 0.8


def main(argv):
    mode = argv[0] if argv else "device"
    nums = [int(a) for a in argv[1:]]
    D, H, W, K = (nums + [220, 400, 400, 16][len(nums):])[:4]
    pred, _ = synthetic_case(D, H, W, K)
    classes = list(range(1, K))
    rec = {"mode": mode, "shape": [D, H, W], "labels": K, "foreground_share": round(float((pred > 0).mean()), 4)}
    if mode == "host":
        from tests import cc_oracle as co
        n = nums[4] if len(nums) > 4 else 2
        times = []
        for c in classes[:n]:
            vol = pred.copy()
            t0 = time.perf_counter()
            _, removed, kept = co.remove_all_but_the_largest_connected_component(vol, [c], VOLUME_PER_VOXEL)
            times.append(time.perf_counter() - t0)
            print("host class %d: %.2f s  kept %.1f  largest removed %s" % (c, times[-1], kept[c], removed[c]), flush=True)
        t0 = time.perf_counter()
        co.remove_all_but_the_largest_connected_component(pred.copy(), [classes], VOLUME_PER_VOXEL)
        rec.update(entries_timed=n, s_per_class_entry=round(float(np.mean(times)), 3), s_joint_region_entry=round(time.perf_counter() - t0, 3),
                   s_per_case_extrapolated=round(float(np.mean(times)) * len(classes), 1))
    else:
        import torch
        from e2enet_medical_amd.postprocessing.connected_components import remove_all_but_the_largest_connected_component as remove
        assert torch.cuda.is_available(), "postprocessing_bench device needs a GPU"
        remove(pred[:8].copy(), classes[:2], VOLUME_PER_VOXEL)                       # code objects, allocator
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, removed, kept = remove(pred.copy(), classes, VOLUME_PER_VOXEL)
        torch.cuda.synchronize()
        case_s = time.perf_counter() - t0
        dev = torch.from_numpy(pred).cuda()
        per = []
        for c in classes + [classes]:                                                  # every class, then all as one region
            work = dev.clone()
            remove(work, [c], VOLUME_PER_VOXEL)                                        # (allocations of this shape)
            work = dev.clone()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            remove(work, [c], VOLUME_PER_VOXEL)
            e1.record()
            torch.cuda.synchronize()
            per.append(e0.elapsed_time(e1))
        rec.update(ms_per_class_entry=round(float(np.median(per[:-1])), 2), ms_per_class_entry_max=round(float(max(per[:-1])), 2),
                   ms_joint_region_entry=round(per[-1], 2), s_per_case_with_upload_and_download=round(case_s, 3),
                   kept={str(c): kept[c] for c in classes[:3]}, largest_removed={str(c): removed[c] for c in classes[:3]})
    print(json.dumps(rec))


if __name__ == "__main__":
    main(sys.argv[1:])
