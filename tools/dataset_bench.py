#!/usr/bin/env python
"""Training-folder preprocessing benchmark (diagnostic, not gated).

   python tools/dataset_bench.py select small|large   class locations of one label volume: device time of the count and of the
                                                      selection (events, ranks resident), wall time of class_locations with the
                                                      host's draw and the transfers, and the host time of the reference's method
                                                      (np.argwhere + RandomState.choice per class) on the same downloaded volume
   python tools/dataset_bench.py run [threads]        GenericPreprocessor.run over a synthetic cropped folder: wall time per case,
                                                      the share of the device half and of the compression + writing
small: 128 x 160 x 160 with 3 classes; large: 256 x 400 x 400 with 15 classes.  Each mode prints one JSON line."""
import json
import os
import pickle
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def label_volume(shape, num_classes, seed=11):
    """blocks of 4^3 voxels: 25% outside the mask (-1), 45% background, the rest shared by the classes"""
    rng = np.random.default_rng(seed)
    coarse = tuple(-(-s // 4) for s in shape)
    p = [0.25, 0.45] + [0.30 / num_classes] * num_classes
    lab = rng.choice(np.arange(-1, num_classes + 1).astype(np.float32), size=coarse, p=p)
    for a in range(3):
        lab = np.repeat(lab, 4, axis=a)
    return np.ascontiguousarray(lab[tuple(slice(0, s) for s in shape)])


def reference_method(seg, all_classes):
    rndst = np.random.RandomState(1234)
    out = {}
    for c in all_classes:
        all_locs = np.argwhere(seg == c)
        if len(all_locs) == 0:
            out[c] = []
            continue
        t = max(min(10000, len(all_locs)), int(np.ceil(len(all_locs) * 0.01)))
        out[c] = all_locs[rndst.choice(len(all_locs), t, replace=False)]
    return out


def median_ms(fn, reps=5, inner=50):
    """ms per call: median over `reps` event windows of `inner` back-to-back calls each (one call is tens of microseconds)"""
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / inner)
    return float(np.median(out))


def bench_select(kind):
    import torch
    from e2enet_medical_amd._lib import lib
    from e2enet_medical_amd.preprocessing import class_locations
    from e2enet_medical_amd.preprocessing.class_sampling import draw_ranks, sort_ranks
    shape, k = ((128, 160, 160), 3) if kind == "small" else ((256, 400, 400), 15)
    classes = list(range(1, k + 1))
    seg = label_volume(shape, k)
    dev = torch.from_numpy(seg).cuda()
    L, st = lib(), torch.cuda.current_stream().cuda_stream
    n = seg.size
    cls = np.asarray(classes, dtype=np.float32)
    ws = torch.empty(L.pp_select_ws_bytes(n, k), dtype=torch.uint8, device="cuda")
    counts = torch.empty(k, dtype=torch.int64, device="cuda")
    ms_count = median_ms(lambda: L.pp_select_count(dev.data_ptr(), n, cls.ctypes.data, k, counts.data_ptr(), ws.data_ptr(), st))
    t0 = time.perf_counter()
    drawn = draw_ranks(counts.cpu().numpy())
    pairs = [sort_ranks(r) for r in drawn]
    s_draw = time.perf_counter() - t0
    offs = np.zeros(k + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(p[0]) for p in pairs])
    ranks = torch.from_numpy(np.concatenate([p[0] for p in pairs])).cuda()
    slots = torch.from_numpy(np.concatenate([p[1] for p in pairs])).cuda()
    out = torch.empty((int(offs[-1]), 3), dtype=torch.int64, device="cuda")
    ms_select = median_ms(lambda: L.pp_select_coords(dev.data_ptr(), shape[0], shape[1], shape[2], cls.ctypes.data, k, ranks.data_ptr(),
                                                     slots.data_ptr(), offs.ctypes.data, out.data_ptr(), ws.data_ptr(), st))
    class_locations(dev, classes)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = class_locations(dev, classes)
    s_whole = time.perf_counter() - t0
    host = dev.cpu().numpy()
    t0 = time.perf_counter()
    want = reference_method(host, classes)
    s_host = time.perf_counter() - t0
    assert all(np.array_equal(got[c], want[c]) for c in classes)
    print(json.dumps({"mode": "select", "case": kind, "shape": list(shape), "classes": k, "rows": int(offs[-1]),
                      "voxels_per_class": [int(v) for v in counts.cpu().numpy()], "ms_count": round(ms_count, 3),
                      "ms_select": round(ms_select, 3), "gbps_count": round(n * 4 / ms_count / 1e6, 1),
                      "s_host_draw_and_sort": round(s_draw, 4), "s_class_locations_wall": round(s_whole, 4),
                      "s_reference_method_host": round(s_host, 4), "threads": os.environ.get("OMP_NUM_THREADS")}))


def bench_run(threads):
    import torch
    from e2enet_medical_amd.preprocessing import GenericPreprocessor
    shape, spacing, target, n_cases, classes = (64, 256, 256), (5.0, 0.8, 0.8), (2.5, 0.8, 0.8), 3, [1, 2, 3]
    rng = np.random.default_rng(3)
    with tempfile.TemporaryDirectory() as tmp:
        cropped, out = os.path.join(tmp, "cropped"), os.path.join(tmp, "out")
        os.makedirs(cropped)
        for ci in range(n_cases):
            seg = label_volume(shape, len(classes), seed=20 + ci)
            data = (rng.normal(100.0, 25.0, (2,) + shape).astype(np.float32) + 40 * seg) * (seg >= 0)
            np.savez_compressed(os.path.join(cropped, "case_%d.npz" % ci), data=np.vstack((data, seg[None])))
            with open(os.path.join(cropped, "case_%d.pkl" % ci), "wb") as f:
                pickle.dump({"original_spacing": np.array(spacing), "crop_bbox": [[0, s] for s in shape]}, f)
        with open(os.path.join(cropped, "dataset_properties.pkl"), "wb") as f:
            pickle.dump({"all_classes": classes}, f)
        pre = GenericPreprocessor({0: "nonCT", 1: "nonCT"}, {0: True, 1: True}, [0, 1, 2])
        pre._preprocess_cropped(np.array(target), "case_0", cropped, None, classes)          # code objects
        torch.cuda.synchronize()
        os.makedirs(out)
        s_load = s_dev = s_write = 0.0
        for ci in range(n_cases):
            t0 = time.perf_counter()
            pre.load_cropped(cropped, "case_%d" % ci)
            t1 = time.perf_counter()
            done = pre._preprocess_cropped(np.array(target), "case_%d" % ci, cropped, None, classes)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            pre._write_case(*done, out, "case_%d" % ci)
            t3 = time.perf_counter()
            s_load += t1 - t0
            s_dev += t2 - t1 - (t1 - t0)                         # (_preprocess_cropped loads the case again)
            s_write += t3 - t2
        walls = {}
        for th in threads:
            t0 = time.perf_counter()
            pre.run([np.array(target)], cropped, os.path.join(tmp, "run%d" % th), "bench", th)
            walls[str(th)] = round((time.perf_counter() - t0) / n_cases, 3)
        print(json.dumps({"mode": "run", "cases": n_cases, "cropped_shape": [3] + list(shape), "resampled_shape": list(done[0].shape),
                          "s_per_case_read_cropped_npz": round(s_load / n_cases, 3),
                          "s_per_case_device_half_incl_transfers": round(s_dev / n_cases, 3),
                          "s_per_case_savez_and_pickle": round(s_write / n_cases, 3), "s_per_case_run_by_threads": walls,
                          "threads_env": os.environ.get("OMP_NUM_THREADS")}))


def main(argv):
    mode = argv[0] if argv else "select"
    if mode == "select":
        bench_select(argv[1] if len(argv) > 1 else "small")
    else:
        bench_run([int(v) for v in argv[1:]] or [1, 8])


if __name__ == "__main__":
    main(sys.argv[1:])
