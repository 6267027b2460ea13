#!/usr/bin/env python
"""Training-folder preprocessing benchmark (diagnostic, not gated).

   python tools/dataset_bench.py select small|large   class locations of one label volume: device time of the count and of the
                                                      selection (events, ranks resident), wall time of class_locations with the
                                                      host's draw and the transfers, and the host time of the reference's method
                                                      (np.argwhere + RandomState.choice per class) on the same downloaded volume
   python tools/dataset_bench.py run [threads] [--device_deflate | --dynamic_huffman]
                                                      GenericPreprocessor.run over a synthetic cropped folder: wall time per case,
                                                      the share of the device half and of the compression + writing, the bytes of
                                                      the .npz files; with a switch the .npz is deflated on the device
                                                      (run(device_deflate=True or "dynamic"))
   python tools/dataset_bench.py fingerprint          the dataset fingerprint of one 256 x 400 x 400 CT-like case (two modalities, about
                                                      30 % foreground): device time of the two sample passes, of the statistics over
                                                      the case's sample and over 100 copies of it behind one another, wall time of
                                                      DatasetAnalyzer.collect_intensity_properties over a synthetic cropped folder, and
                                                      the host time of the reference's method on the same arrays (modality[mask][::10]
                                                      as a list, list concatenation, the seven numpy calls)
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


def bench_run(threads, device_deflate=False):
    import torch
    from e2enet_medical_amd import deflate
    from e2enet_medical_amd.preprocessing import GenericPreprocessor
    from e2enet_medical_amd.preprocessing.preprocessing import DeflatedCase
    codes = deflate.codes_of(device_deflate)
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
        warm = pre._preprocess_cropped(np.array(target), "case_0", cropped, None, classes, keep_on_device=codes is not None)
        if codes is not None:
            DeflatedCase(warm[0], codes)                                                     # code objects
        del warm
        torch.cuda.synchronize()
        os.makedirs(out)
        s_load = s_dev = s_write = 0.0
        for ci in range(n_cases):
            t0 = time.perf_counter()
            pre.load_cropped(cropped, "case_%d" % ci)
            t1 = time.perf_counter()
            done = pre._preprocess_cropped(np.array(target), "case_%d" % ci, cropped, None, classes, keep_on_device=codes is not None)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            shape_out = list(done[0].shape)
            if codes is not None:                                # (the device's deflate counts as compression + writing)
                done = (DeflatedCase(done[0], codes), done[1])
            pre._write_case(*done, out, "case_%d" % ci)
            t3 = time.perf_counter()
            s_load += t1 - t0
            s_dev += t2 - t1 - (t1 - t0)                         # (_preprocess_cropped loads the case again)
            s_write += t3 - t2
        walls = {}
        for th in threads:
            t0 = time.perf_counter()
            pre.run([np.array(target)], cropped, os.path.join(tmp, "run%d" % th), "bench", th, device_deflate=device_deflate)
            walls[str(th)] = round((time.perf_counter() - t0) / n_cases, 3)
        npz_bytes = sum(os.path.getsize(os.path.join(out, "case_%d.npz" % ci)) for ci in range(n_cases)) // n_cases
        print(json.dumps({"mode": "run", "device_deflate": device_deflate, "cases": n_cases, "cropped_shape": [3] + list(shape),
                          "resampled_shape": shape_out, "npz_bytes_per_case": npz_bytes,
                          "s_per_case_read_cropped_npz": round(s_load / n_cases, 3),
                          "s_per_case_device_half_incl_transfers": round(s_dev / n_cases, 3),
                          "s_per_case_savez_and_pickle": round(s_write / n_cases, 3), "s_per_case_run_by_threads": walls,
                          "threads_env": os.environ.get("OMP_NUM_THREADS")}))


def ct_like_case(shape, seed):
    """[3, *shape] fp32: two modalities of whole-number intensities that follow the labels, and the label volume of label_volume"""
    rng = np.random.default_rng(seed)
    seg = label_volume(shape, 3, seed=seed)
    out = np.empty((3,) + tuple(shape), dtype=np.float32)
    for c in range(2):
        out[c] = np.rint(rng.standard_normal(shape, dtype=np.float32) * (25.0 + 10.0 * c) + 100.0)
        out[c] += 40.0 * seg
        out[c] *= seg >= 0
    out[2] = seg
    return out


def reference_stats(voxels):
    """DatasetAnalyzer._compute_stats of the reference, on the list it is handed"""
    if len(voxels) == 0:
        return (np.nan,) * 7
    return (np.median(voxels), np.mean(voxels), np.std(voxels), np.min(voxels), np.max(voxels), np.percentile(voxels, 99.5),
            np.percentile(voxels, 00.5))


def reference_intensity_properties(folder, cases, num_modalities):
    """collect_intensity_properties of the reference without its process pool: one read of every case per modality"""
    out = []
    for mod in range(num_modalities):
        v = []
        for c in cases:
            all_data = np.load(os.path.join(folder, c + ".npz"))['data']
            v.append(list(all_data[mod][all_data[-1] > 0][::10]))
        w = []
        for iv in v:
            w += iv
        out.append((reference_stats(w), [reference_stats(iv) for iv in v]))
    return out


def bench_fingerprint():
    import torch
    from e2enet_medical_amd._lib import lib
    from e2enet_medical_amd.experiment_planning import DatasetAnalyzer
    from e2enet_medical_amd.experiment_planning.DatasetAnalyzer import foreground_sample
    from e2enet_medical_amd.experiment_planning.intensity_stats import requested_ranks
    from e2enet_medical_amd.preprocessing.preprocessing import save_npz
    shape, copies = (256, 400, 400), 100
    case = ct_like_case(shape, 31)
    dev = torch.from_numpy(case).cuda()
    L, st = lib(), torch.cuda.current_stream().cuda_stream
    n = int(np.prod(shape))
    ws = torch.empty(L.fingerprint_sample_ws_bytes(n), dtype=torch.uint8, device="cuda")
    n_fg = torch.empty(1, dtype=torch.int64, device="cuda")
    ms_count = median_ms(lambda: L.fingerprint_sample_count(dev[2].data_ptr(), n, n_fg.data_ptr(), ws.data_ptr(), st))
    fg = int(n_fg.item())
    m = -(-fg // 10)
    out = torch.empty((2, m), dtype=torch.float32, device="cuda")
    ms_gather = median_ms(lambda: L.fingerprint_sample_gather(dev.data_ptr(), dev[2].data_ptr(), 2, n, 10, out.data_ptr(), m, ws.data_ptr(), st))
    sample = foreground_sample(dev)
    assert torch.equal(sample, out)

    def stats_ms(x, inner):
        ranks = np.asarray(requested_ranks(x.numel()), dtype=np.int64)
        sws = torch.empty(L.fingerprint_stats_ws_bytes(), dtype=torch.uint8, device="cuda")
        res = torch.empty(16, dtype=torch.float64, device="cuda")
        return median_ms(lambda: L.fingerprint_stats(x.data_ptr(), x.numel(), ranks.ctypes.data, len(ranks), res.data_ptr(), sws.data_ptr(), st),
                         inner=inner)
    ms_stats_case = stats_ms(sample[0], 20)
    big = sample[0].repeat(copies)
    ms_stats_big = stats_ms(big, 3)
    got_case, got_big = DatasetAnalyzer._compute_stats(sample[0]), DatasetAnalyzer._compute_stats(big)
    # the reference's method on the same arrays, one modality of the case, then the seven numbers of the list
    host = case
    t0 = time.perf_counter()
    voxels = list(host[0][host[-1] > 0][::10])
    t1 = time.perf_counter()
    want_case = reference_stats(voxels)
    t2 = time.perf_counter()
    assert len(voxels) == m and got_case[0] == want_case[0] and got_case[3] == want_case[3] and got_case[4] == want_case[4]
    del dev, big, out
    # a folder of smaller cases: the whole of collect_intensity_properties against the reference's loop over the same files
    fshape, n_cases = (128, 200, 200), 4
    with tempfile.TemporaryDirectory() as tmp:
        names = ["case_%d" % i for i in range(n_cases)]
        for i, c in enumerate(names):
            save_npz(os.path.join(tmp, c + ".npz"), ct_like_case(fshape, 50 + i))
        with open(os.path.join(tmp, "dataset.json"), "w") as f:
            json.dump({"modality": {"0": "CT", "1": "CT"}, "labels": {"0": "bg", "1": "a", "2": "b", "3": "c"}}, f)
        walls = {}
        for th in (1, 8):
            an = DatasetAnalyzer(tmp, overwrite=True, num_processes=th)
            t3 = time.perf_counter()
            got = an.collect_intensity_properties(2)
            torch.cuda.synchronize()
            walls[str(th)] = round(time.perf_counter() - t3, 3)
        t3 = time.perf_counter()
        want = reference_intensity_properties(tmp, names, 2)
        s_ref_folder = time.perf_counter() - t3
        ulps = []
        for mod in range(2):
            assert got[mod]['median'] == want[mod][0][0] and got[mod]['mn'] == want[mod][0][3]
            for k, i in (('percentile_99_5', 5), ('percentile_00_5', 6), ('mean', 1), ('sd', 2)):
                ulps.append(abs(float(got[mod][k]) - float(want[mod][0][i])) / float(np.spacing(np.float32(abs(want[mod][0][i])))))
    print(json.dumps({"mode": "fingerprint", "shape": list(shape), "modalities": 2, "foreground_voxels": fg, "sample_per_modality": m,
                      "ms_sample_count": round(ms_count, 3), "ms_sample_gather": round(ms_gather, 3),
                      "gbps_count": round(n * 4 / ms_count / 1e6, 1), "ms_stats_case": round(ms_stats_case, 3),
                      "values_100_copies": m * copies, "ms_stats_100_copies": round(ms_stats_big, 3),
                      "gbps_stats_100_copies_6_sweeps": round(6 * m * copies * 4 / ms_stats_big / 1e6, 1),
                      "stats_100_copies_equal_case": [bool(a == b) for a, b in zip(got_big, got_case)],
                      "s_reference_sample_as_list_one_modality": round(t1 - t0, 3), "s_reference_seven_numpy_calls": round(t2 - t1, 3),
                      "folder": {"cases": n_cases, "shape": list(fshape), "s_collect_intensity_properties_by_threads": walls,
                                 "s_reference_method_host": round(s_ref_folder, 3),
                                 "max_fp32_ulp_from_reference_pct_mean_sd": round(max(ulps), 2)},
                      "threads_env": os.environ.get("OMP_NUM_THREADS")}))


def main(argv):
    mode = argv[0] if argv else "select"
    if mode == "select":
        bench_select(argv[1] if len(argv) > 1 else "small")
    elif mode == "fingerprint":
        bench_fingerprint()
    else:
        flag = "dynamic" if "--dynamic_huffman" in argv else "--device_deflate" in argv
        bench_run([int(v) for v in argv[1:] if not v.startswith("--")] or [1, 8], flag)


if __name__ == "__main__":
    main(sys.argv[1:])
