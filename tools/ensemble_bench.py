#!/usr/bin/env python
"""Ensembling benchmark (diagnostic, not gated) on an AMOS-sized case (default 220 x 400 x 400, K = 16).

   python tools/ensemble_bench.py device [D H W K]        e2e_merge_softmax_f16 for N = 2 and N = 5 resident fp16 volumes (labels only,
                                                          and labels + fp16 mean) and e2e_softmax_to_f16 of one fp32 volume: device
                                                          events, median of 5 windows of 5 calls after a warm-up; the algorithmic
                                                          bytes (2*N*K + 1 per voxel, + 2*K with the mean; 6*K for the conversion)
                                                          over that time, beside the 6.29 TB/s a device copy reaches
   python tools/ensemble_bench.py host [D H W K]          what the merge replaces, on arrays of the same shape: np.vstack, np.mean,
                                                          argmax and the crop-box placement, for N = 2 and N = 5
   python tools/ensemble_bench.py folder OUT [D H W K] [CASES]   whole-folder wall time of merge() over CASES cases x 2 folders of
                                                          .npz files written under OUT first, with threads = 1 and 8
Each mode prints one JSON line."""
import json
import os
import pickle
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOWS, CALLS = 5, 5
COPY_TBS = 6.29


def _props(D, H, W):
    return {'size_after_cropping': np.array([D, H, W]), 'original_size_of_raw_data': np.array([D + 6, H + 12, W + 12]),
            'crop_bbox': [[3, 3 + D], [6, 6 + H], [6, 6 + W]], 'itk_spacing': (1.0, 1.0, 2.0)}


def _timed(call):
    import torch
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    per_call = []
    for _ in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            call()
        e1.record()
        torch.cuda.synchronize()
        per_call.append(e0.elapsed_time(e1) / CALLS)
    return float(np.median(per_call)), min(per_call), max(per_call)


def _rate(rec, name, ms, nbytes):
    rec[name + "_ms"], rec[name + "_ms_min"], rec[name + "_ms_max"] = (round(v, 3) for v in ms)
    rec[name + "_bytes"] = int(nbytes)
    tbs = nbytes / (ms[0] * 1e-3) / 1e12
    rec[name + "_tb_per_s"] = round(tbs, 3)
    rec[name + "_share_of_copy_rate"] = round(tbs / COPY_TBS, 3)


def device(D, H, W, K):
    import ctypes
    import torch
    from e2enet_medical_amd._lib import lib
    assert torch.cuda.is_available(), "ensemble_bench device needs a GPU"
    L, n = lib(), D * H * W
    st = torch.cuda.current_stream().cuda_stream
    rec = {"mode": "device", "shape": [D, H, W], "classes": K, "copy_rate_tb_per_s": COPY_TBS}
    g = torch.Generator(device="cuda").manual_seed(0)
    srcs = [torch.rand((K, D, H, W), generator=g, device="cuda", dtype=torch.float32).half() for _ in range(5)]
    p = _props(D, H, W)
    OA, OB, OC = (int(v) for v in p['original_size_of_raw_data'])
    seg = torch.zeros((OA, OB, OC), dtype=torch.uint8, device="cuda")
    mean = torch.empty((K, D, H, W), dtype=torch.float16, device="cuda")
    for N in (2, 5):
        arr = ctypes.cast((ctypes.c_void_p * N)(*[s.data_ptr() for s in srcs[:N]]), ctypes.c_void_p)
        for tag, mp, extra in (("labels", None, 0), ("labels_mean", mean.data_ptr(), 2 * K)):
            call = lambda: L.merge_softmax_f16(arr, N, K, D, H, W, seg.data_ptr(), OA, OB, OC, 3, 6, 6, None, 0, mp, st)
            _rate(rec, "merge_n%d_%s" % (N, tag), _timed(call), n * (2 * N * K + 1 + extra))
    del srcs[1:]
    soft = torch.rand((K, D, H, W), generator=g, device="cuda", dtype=torch.float32)
    call = lambda: L.softmax_to_f16(soft.data_ptr(), mean.data_ptr(), K, n, D, H, W, H * W, W, 1, st)
    _rate(rec, "to_f16", _timed(call), n * 6 * K)
    call = lambda: L.softmax_to_f16(soft.data_ptr(), mean.data_ptr(), K, n, W, D, H, 1, H * W, W, st)          # transpose_backward [2, 0, 1]
    _rate(rec, "to_f16_transposed_201", _timed(call), n * 6 * K)
    return rec


def host_merge(srcs, p):
    """the reference's array expressions (ensemble_predictions.py:28-30, segmentation_export.py:124-140)"""
    softmax = [s[None] for s in srcs]
    softmax = np.vstack(softmax)
    softmax = np.mean(softmax, 0)
    seg = softmax.argmax(0)
    out = np.zeros(p['original_size_of_raw_data'], dtype=np.uint8)
    b = p['crop_bbox']
    out[b[0][0]:b[0][1], b[1][0]:b[1][1], b[2][0]:b[2][1]] = seg
    return out


def host(D, H, W, K):
    rng = np.random.RandomState(0)
    base = rng.rand(K, D, H, W).astype(np.float16)
    srcs = [base] + [np.roll(base, i, axis=0) for i in range(1, 5)]
    rec = {"mode": "host", "shape": [D, H, W], "classes": K, "cpus": len(os.sched_getaffinity(0))}
    for N in (2, 5):
        times = []
        for _ in range(2):
            t0 = time.perf_counter()
            host_merge(srcs[:N], _props(D, H, W))
            times.append(time.perf_counter() - t0)
        rec["host_merge_n%d_s" % N] = round(min(times), 2)
        rec["host_merge_n%d_all" % N] = [round(t, 2) for t in times]
    return rec


def folder(out, D, H, W, K, cases):
    import torch
    from concurrent.futures import ThreadPoolExecutor
    from e2enet_medical_amd.inference.ensemble_predictions import merge
    assert torch.cuda.is_available(), "ensemble_bench folder needs a GPU"
    rec = {"mode": "folder", "shape": [D, H, W], "classes": K, "cases": cases, "folders": 2}
    folders = [os.path.join(out, "f%d" % i) for i in range(2)]
    g = torch.Generator(device="cuda").manual_seed(1)
    zz, yy, xx = torch.meshgrid(*[torch.arange(s, device="cuda", dtype=torch.float32) for s in (D, H, W)], indexing="ij")
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=8) as pool:
        jobs = []
        for fi, f in enumerate(folders):
            os.makedirs(f, exist_ok=True)
            for c in range(cases):
                # confident probabilities over smooth regions, as a trained network leaves them: most values are 0 or 1 in fp16
                field = torch.sin(zz * 0.031 + c) + torch.sin(yy * 0.023 + fi * 0.1) + torch.sin(xx * 0.019)
                logits = torch.stack([-(field * K / 6.0 + K / 2.0 - k) ** 2 for k in range(K)]) * 8.0
                logits += torch.rand(logits.shape, generator=g, device="cuda")
                soft = torch.softmax(logits, 0).half().cpu().numpy()
                del logits
                jobs.append(pool.submit(np.savez_compressed, os.path.join(f, "case_%02d.npz" % c), softmax=soft))
                with open(os.path.join(f, "case_%02d.pkl" % c), "wb") as fh:
                    pickle.dump(_props(D, H, W), fh)
        for j in jobs:
            j.result()
    rec["setup_s"] = round(time.perf_counter() - t0, 1)
    rec["npz_bytes_per_case"] = os.path.getsize(os.path.join(folders[0], "case_00.npz"))
    t0 = time.perf_counter()
    np.load(os.path.join(folders[0], "case_00.npz"))['softmax']
    rec["one_npz_read_s"] = round(time.perf_counter() - t0, 2)
    for threads in (1, 8):
        dst = os.path.join(out, "merged_t%d" % threads)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        merge(folders, dst, threads, writer=lambda seg, path, props: np.save(path[:-7] + ".npy", seg))
        rec["merge_threads%d_s" % threads] = round(time.perf_counter() - t0, 2)
    same = all(open(os.path.join(out, "merged_t1", n), "rb").read() == open(os.path.join(out, "merged_t8", n), "rb").read()
               for n in sorted(os.listdir(os.path.join(out, "merged_t1"))))
    rec["outputs_identical"] = same
    return rec


def main(argv):
    mode = argv[0] if argv else "device"
    rest = argv[1:]
    out = rest.pop(0) if mode == "folder" else None
    nums = [int(a) for a in rest]
    D, H, W, K, cases = (nums + [220, 400, 400, 16, 3][len(nums):])[:5]
    if mode == "device":
        rec = device(D, H, W, K)
    elif mode == "host":
        rec = host(D, H, W, K)
    elif mode == "folder":
        rec = folder(out, D, H, W, K, cases)
    else:
        raise SystemExit("unknown mode %r" % mode)
    print(json.dumps(rec))


if __name__ == "__main__":
    main(sys.argv[1:])
