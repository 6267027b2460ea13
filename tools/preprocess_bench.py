#!/usr/bin/env python
"""Preprocessing benchmark (diagnostic, not gated): crop, resample, normalise of one synthetic raw case by the device path
(e2enet_medical_amd/preprocessing, csrc/preprocess.hip) and by its host restatement (tests/preprocess_oracle.py, fp64 scipy).

   python tools/preprocess_bench.py device brats|ct     device time per stage (events, the case resident) and for the whole
                                                        preprocess_test_case with the upload and the download; per streaming
                                                        kernel the algorithmic bytes over its time
   python tools/preprocess_bench.py host brats|ct       host time per stage of the restatement
brats: 4 x 155 x 240 x 240, isotropic at the plans' spacing (no resampling), every modality normalised inside the non-zero mask.
ct:    1 x 90 x 512 x 512 at (5, 0.8, 0.8) mm -> plans spacing (2.5, 0.7, 0.7): the anisotropy makes z a separate axis; CT scheme.
The two modes are separate commands so that each runs under its own time limit; each prints one JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IP = {0: {'mean': 80.0, 'sd': 40.0, 'percentile_00_5': -100.0, 'percentile_99_5': 300.0}}


def synthetic_case(kind):
    """(data, properties, target spacing, schemes, use_mask): an ellipsoidal head / body inside a zero (brats) or air (ct) margin"""
    rng = np.random.default_rng(5)
    if kind == "brats":
        shape, c, spacing, target = (155, 240, 240), 4, (1.0, 1.0, 1.0), (1.0, 1.0, 1.0)
    else:
        shape, c, spacing, target = (90, 512, 512), 1, (5.0, 0.8, 0.8), (2.5, 0.7, 0.7)
    grid = np.meshgrid(*[np.linspace(-1, 1, s, dtype=np.float32) for s in shape], indexing="ij", sparse=True)
    inside = (grid[0] / 0.85) ** 2 + (grid[1] / 0.7) ** 2 + (grid[2] / 0.6) ** 2 < 1
    data = np.zeros((c,) + shape, dtype=np.float32)
    for m in range(c):
        tex = rng.normal(100.0 + 30 * m, 25.0, shape).astype(np.float32)
        data[m] = np.where(inside, tex, 0.0)
    data[:, shape[0] // 2 - 3:shape[0] // 2 + 3, shape[1] // 2 - 9:shape[1] // 2 + 9, shape[2] // 2 - 9:shape[2] // 2 + 9] = 0      # a cavity
    props = {"original_spacing": np.array(spacing), "original_size_of_raw_data": np.array(shape)}
    schemes = {m: ("nonCT" if kind == "brats" else "CT") for m in range(c)}
    return data, props, np.array(target), schemes, {m: kind == "brats" for m in range(c)}


def main(argv):
    mode, kind = (argv + ["device", "brats"][len(argv):])[:2]
    data, props, target, schemes, use_mask = synthetic_case(kind)
    rec = {"mode": mode, "case": kind, "shape": list(data.shape), "target_spacing": [float(v) for v in target]}
    if mode == "host":
        from tests import preprocess_oracle as po
        t = [time.perf_counter()]
        d, s, p = po.crop(data.copy(), dict(props), None)
        t.append(time.perf_counter())
        d = np.where(np.isnan(d), 0, d)
        new_shape = po.resampled_shape(d[0].shape, props["original_spacing"], target)
        do, axis = po.separate_z_plan(props["original_spacing"], target)
        d2, _ = po.resample_data_or_seg(d, new_shape, False, axis, 3, do)
        d2 = np.asarray(d2, dtype=np.float32)
        t.append(time.perf_counter())
        s2, _ = po.resample_data_or_seg(s, new_shape, True, axis, 1, do)
        t.append(time.perf_counter())
        po.normalize(d2, s2, schemes, use_mask, IP)
        t.append(time.perf_counter())
        rec.update(cropped=list(d.shape), resampled=list(d2.shape), threads=os.environ.get("OMP_NUM_THREADS"),
                   **{"s_" + k: round(b - a, 3) for k, a, b in zip(("crop", "resize_data", "resize_seg", "normalize"), t, t[1:])},
                   s_total=round(t[-1] - t[0], 3))
        print(json.dumps(rec))
        return
    import torch
    from e2enet_medical_amd.preprocessing import GenericPreprocessor, ImageCropper
    from e2enet_medical_amd.preprocessing.preprocessing import resample_patient
    assert torch.cuda.is_available(), "preprocess_bench device needs a GPU"
    pre = GenericPreprocessor(schemes, use_mask, [0, 1, 2], IP)

    def timed(fn, reps=3):
        fn()                                                     # code objects, allocations of this shape
        torch.cuda.synchronize()
        out = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            res = fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1))
        return float(np.median(out)), res

    dev = torch.from_numpy(data).cuda()
    ms_crop, (d, s, p) = timed(lambda: ImageCropper.crop(dev, dict(props), None))
    ms_resize, (d2, s2) = timed(lambda: resample_patient(d, s, props["original_spacing"], target, 3, 1, force_separate_z=None))
    ms_norm, _ = timed(lambda: pre.resample_and_normalize(d2.clone(), target, dict(props, original_spacing=target), s2.clone()))
    t0 = time.perf_counter()
    out = pre.preprocess_test_case((data, dict(props)), target)
    torch.cuda.synchronize()
    case_s = time.perf_counter() - t0
    rec.update(cropped=list(d.shape), resampled=list(d2.shape), ms_crop=round(ms_crop, 2), ms_resample=round(ms_resize, 2),
               ms_normalize_incl_clone=round(ms_norm, 2), ms_device_total=round(ms_crop + ms_resize + ms_norm, 2),
               s_case_with_upload_and_download=round(case_s, 3), out_shape=list(out[0].shape))
    print(json.dumps(rec))


if __name__ == "__main__":
    main(sys.argv[1:])
