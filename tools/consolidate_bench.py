#!/usr/bin/env python
"""Component-table benchmark (diagnostic, not gated) on the synthetic case of tools/postprocessing_bench.py (K - 1 ellipsoidal organs
plus 0.2 % stray voxels per label).

   python tools/consolidate_bench.py table [D H W K]        one component table of the resident case (e2e_ct_label + e2e_ct_emit, the
                                                            record counts read in between) against the K - 1 per-class
                                                            e2e_cc_remove_all_but_largest calls it replaces in a sweep: device events,
                                                            median and range of 5 windows each, alternating; and component_table()
                                                            as the folder search calls it (census, allocations and reads included)
   python tools/consolidate_bench.py search [D H W K] [N]   the search over N copies of the case (default 3): the folder form over .npy
                                                            files (read twice, tables, final removal, files written) against the
                                                            in-memory search on the same arrays (host clocks around synchronised work)
(default 220 400 400 16).  Separate commands so that each runs under its own time limit; each prints one JSON line."""
import ctypes
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.surface_bench import synthetic_case          # noqa: E402

VOLUME_PER_VOXEL = 2.0 * 0.8 * 0.8
WINDOWS = 5


def _stats(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(min(ms)), 3), "max_ms": round(float(max(ms)), 3)}


def bench_table(pred, gt, classes, rec):
    import torch
    from e2enet_medical_amd._lib import lib
    from e2enet_medical_amd.postprocessing.component_table import component_table
    from e2enet_medical_amd.postprocessing.connected_components import _class_words
    L = lib()
    D, H, W = pred.shape
    st = torch.cuda.current_stream().cuda_stream
    x, g = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    ws = torch.empty(L.ct_ws_bytes(D, H, W), dtype=torch.uint8, device="cuda")
    cc_ws = torch.empty(L.cc_ws_bytes(D, H, W), dtype=torch.uint8, device="cuda")
    res = torch.zeros(4, dtype=torch.int64, device="cuda")
    cc_res = torch.zeros((len(classes), 4), dtype=torch.int64, device="cuda")
    words = lambda members: ctypes.cast((ctypes.c_uint * 8)(*_class_words(members)), ctypes.c_void_p)
    all_words, one_words = words(classes), [words([c]) for c in classes]

    def table():
        L.ct_label(x.data_ptr(), g.data_ptr(), D, H, W, all_words, ws.data_ptr(), res.data_ptr(), st)
        n_class, n_fg, gave_up, _ = res.cpu().tolist()
        assert not gave_up
        class_rec = torch.empty((n_class, 5), dtype=torch.int32, device="cuda")
        fg_rec = torch.empty((n_fg, 2), dtype=torch.int32, device="cuda")
        L.ct_emit(x.data_ptr(), D, H, W, ws.data_ptr(), class_rec.data_ptr(), n_class, n_class, fg_rec.data_ptr(), n_fg, n_fg, st)
        return n_class, n_fg

    def per_class(work):
        for k, w in enumerate(one_words):
            L.cc_remove_all_but_largest(work.data_ptr(), D, H, W, w, VOLUME_PER_VOXEL, -1.0, cc_ws.data_ptr(), cc_res[k].data_ptr(), st)

    def timed(fn, *a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = fn(*a)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    table()
    per_class(x.clone())                                           # code objects, allocations of this shape
    t_table, t_calls = [], []
    for _ in range(WINDOWS):                                       # alternating, so that both see the same machine
        ms, counts = timed(table)
        t_table.append(ms)
        t_calls.append(timed(per_class, x.clone())[0])
    component_table(x, g, classes)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    t = component_table(x, g, classes)
    torch.cuda.synchronize()
    rec.update(class_components=counts[0], foreground_components=counts[1], table=_stats(t_table),
               per_class_removal_calls=dict(_stats(t_calls), calls=len(classes)),
               component_table_call_ms=round(1e3 * (time.perf_counter() - t0), 2), table_bytes=int(sum(a.nbytes for a in t[2:9])),
               workspace_bytes_per_voxel=20)


def bench_search(pred, gt, classes, n, rec):
    import torch
    from e2enet_medical_amd.evaluator import evaluate_folder
    from e2enet_medical_amd.postprocessing.connected_components import determine_postprocessing
    with tempfile.TemporaryDirectory() as base:
        raw, gts = os.path.join(base, "validation_raw"), os.path.join(base, "gt")
        os.makedirs(raw)
        os.makedirs(gts)
        names = ["case%d.npy" % k for k in range(n)]
        for name in names:
            np.save(os.path.join(raw, name), pred)
            np.save(os.path.join(gts, name), gt)
        evaluate_folder(gts, raw, tuple([0] + classes), num_threads=8)           # summary.json; also code objects and allocator
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = determine_postprocessing(base, gts, final_subf_name="validation_final", processes=8)
        torch.cuda.synchronize()
        folder_s = time.perf_counter() - t0
        mem = os.path.join(base, "mem")
        os.makedirs(mem)
        cases = [(pred, gt, os.path.join(raw, name), os.path.join(gts, name), None) for name in names]
        t0 = time.perf_counter()
        # (the folder form takes the classes in the order of summary.json's sorted keys, "1", "10", ..., "2", as the reference does)
        want, _ = determine_postprocessing(cases, sorted(classes, key=str), mem, "validation_raw", final_subf_name="validation_final",
                                           writer=lambda vol, path, i: np.save(path, vol))
        torch.cuda.synchronize()
        memory_s = time.perf_counter() - t0
        assert json.loads(json.dumps(got)) == json.loads(json.dumps(want)), "the two searches disagree"
    rec.update(cases=n, folder_search_s=round(folder_s, 2), in_memory_search_s=round(memory_s, 2),
               for_which_classes=got['for_which_classes'])


def main(argv):
    import torch
    mode = argv[0] if argv else "table"
    nums = [int(a) for a in argv[1:]]
    D, H, W, K = (nums + [220, 400, 400, 16][len(nums):])[:4]
    assert torch.cuda.is_available(), "consolidate_bench needs a GPU"
    pred, gt = synthetic_case(D, H, W, K)
    classes = list(range(1, K))
    rec = {"mode": mode, "shape": [D, H, W], "labels": K}
    if mode == "search":
        bench_search(pred, gt, classes, nums[4] if len(nums) > 4 else 3, rec)
    else:
        bench_table(pred, gt, classes, rec)
    print(json.dumps(rec))


if __name__ == "__main__":
    main(sys.argv[1:])
