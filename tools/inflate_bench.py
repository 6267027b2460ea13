#!/usr/bin/env python
"""Device inflate against the host read it can replace (diagnostic, not gated).

   python tools/inflate_bench.py OUT                      every step below as a child process of its own, each under a time limit;
                                                          the first step that fails or runs out of time ends the run
   python tools/inflate_bench.py OUT kernels CASE CODES   the three kernels on a resident stream (device events, median of 5 windows
                                                          of 3 calls after a warm-up), and the host's share (candidates, chain)
   python tools/inflate_bench.py OUT load CASE CODES      wall time of deflate.load_npz against np.load + upload of the same file on one
                                                          host thread (warm page cache; one warm-up, then 3 alternating repeats)
   python tools/inflate_bench.py OUT merge CODES          wall time of ensemble_predictions.merge over 3 cases x 2 folders of the probs
                                                          case, threads 1 and 8, with and without device_inflate

   CASE   probs   fp16 class probabilities 16 x 220 x 400 x 400 (tools/deflate_bench.py's)
          stage   fp32 3 x 128 x 256 x 256: two noisy modalities and a label map, as a preprocessed stage case
   CODES  fixed | dynamic: what deflate.savez wrote the file with

Each step prints one JSON line.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

STEP_LIMIT_S = 420
WINDOWS, CALLS = 5, 3


def _tensor(case):
    import torch
    if case == "probs":
        from deflate_bench import synthetic_probs
        return synthetic_probs((220, 400, 400), 16)
    g = torch.Generator(device="cuda").manual_seed(2)
    zz, yy, xx = torch.meshgrid(*[torch.arange(s, device="cuda", dtype=torch.float32) for s in (128, 256, 256)], indexing="ij")
    field = torch.sin(zz * 0.031) + torch.sin(yy * 0.023) + torch.sin(xx * 0.019)
    body = (field > -1.0).float()                                   # zero outside the body, as a cropped and normalised case is
    mods = [(field * (1 + m) + torch.randn(field.shape, generator=g, device="cuda") * 0.1) * body for m in range(2)]
    seg = torch.clamp((field - 0.6) * 2.0, 0, 3).floor() * body
    return torch.stack(mods + [seg]).contiguous()


def _windows(call):
    """median and range (ms per call) of WINDOWS windows of CALLS back-to-back calls, after one warm-up call"""
    import torch
    call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / CALLS)
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def _wall(routes, repeats=3):
    import torch
    for call in routes.values():
        call()
    times = {name: [] for name in routes}
    for _ in range(repeats):
        for name, call in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    return {name: {"median_s": round(float(np.median(t)), 4), "min_s": round(min(t), 4), "max_s": round(max(t), 4)}
            for name, t in times.items()}


def kernels(out, case, codes):
    import torch
    from e2enet_medical_amd import deflate
    from e2enet_medical_amd._lib import lib
    dev = _tensor(case)
    stream, crc, nbytes = deflate.raw_deflate(dev, None, codes)
    body = np.frombuffer(stream[:-2], dtype=np.uint8).copy()
    L, st = lib(), torch.cuda.current_stream().cuda_stream
    comp = torch.from_numpy(body).cuda()
    t0 = time.perf_counter()
    cands = np.asarray(deflate.candidate_starts(body, nbytes), dtype=np.int64)
    t_cand = time.perf_counter() - t0
    cands_d = torch.from_numpy(cands).cuda()
    records = torch.empty((len(cands), deflate.RECORD_WORDS), dtype=torch.int32, device="cuda")
    scan = lambda: L.inflate_scan(comp.data_ptr(), comp.numel(), cands_d.data_ptr(), len(cands), records.data_ptr(), st)
    rec = {"step": "kernels", "case": case, "codes": codes, "input_bytes": nbytes, "stream_bytes": len(stream),
           "candidates": int(len(cands)), "host_candidates_s": round(t_cand, 4), "scan": _windows(scan)}
    table = records.cpu().numpy().view(np.uint32)
    t0 = time.perf_counter()
    starts, tails, _ = deflate.inflate_plan(body, nbytes, lambda s, c: table)
    rec["host_candidates_and_chain_s"] = round(time.perf_counter() - t0, 4)
    rec["records"] = int(len(starts))
    kinds = np.array([int(table[i][1]) & 0xFF for i in np.searchsorted(cands, starts)])
    rec["record_share"] = {n: round(float((kinds == k).mean()), 4) for k, n in enumerate(("stored", "fixed", "dynamic"))}
    starts_d, tails_d = torch.from_numpy(starts).cuda(), torch.from_numpy(tails).cuda()
    outbuf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    status = torch.empty(1, dtype=torch.int32, device="cuda")
    chunks = lambda: L.inflate_chunks(comp.data_ptr(), comp.numel(), starts_d.data_ptr(), tails_d.data_ptr(), len(starts),
                                      outbuf.data_ptr(), nbytes, status.data_ptr(), st)
    rec["chunks"] = _windows(chunks)
    rec["chunks_output_gb_per_s"] = round(nbytes / (rec["chunks"]["median_ms"] * 1e-3) / 1e9, 2)
    work, word = torch.empty(-(-nbytes // deflate.CHUNK), dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")
    rec["crc32"] = _windows(lambda: L.crc32(outbuf.data_ptr(), nbytes, work.data_ptr(), word.data_ptr(), st))
    rec["same_content"] = bool(int(status.item()) == 0 and (int(word.item()) & 0xFFFFFFFF) == crc
                               and torch.equal(outbuf, dev.view(torch.uint8).reshape(-1)))
    return rec


def load(out, case, codes):
    import torch
    from e2enet_medical_amd import deflate
    dev = _tensor(case)
    path = os.path.join(out, "%s_%s.npz" % (case, codes))
    deflate.savez(path, codes=codes, data=dev)
    want = dev.cpu().numpy().tobytes()
    del dev
    torch.cuda.empty_cache()
    stats, parts = {}, {}

    def device():
        t0 = time.perf_counter()
        raw = deflate.read_npz_raw(path)
        parts["read_npz_raw_s"] = round(time.perf_counter() - t0, 4)
        return deflate.load_npz(raw, stats=stats)["data"]

    def host():
        return torch.from_numpy(np.load(path)["data"]).cuda()
    rec = {"step": "load", "case": case, "codes": codes, "file_bytes": os.path.getsize(path), "input_bytes": len(want)}
    rec.update(_wall({"load_npz": device, "np_load_and_upload": host}))
    rec["load_npz"].update(parts)
    rec["member"] = stats["data"]
    rec["same_content"] = device().cpu().numpy().tobytes() == want == host().cpu().numpy().tobytes()
    return rec


def merge(out, codes):
    import torch
    from deflate_bench import synthetic_probs
    from e2enet_medical_amd.inference.ensemble_predictions import merge as merge_folders
    from e2enet_medical_amd.inference.predict import save_softmax_npz
    shape = (220, 400, 400)
    props = {"itk_spacing": (0.8, 0.8, 2.0), "itk_origin": (0., 0., 0.), "itk_direction": (1., 0., 0., 0., 1., 0., 0., 0., 1.),
             "size_after_cropping": shape, "original_size_of_raw_data": np.array(shape), "crop_bbox": [[0, s] for s in shape]}
    dev = synthetic_probs(shape, 16)
    folders = [os.path.join(out, "merge_%s_f%d" % (codes, f)) for f in range(2)]
    for folder in folders:
        os.makedirs(folder, exist_ok=True)
        for c in range(3):
            save_softmax_npz(dev, os.path.join(folder, "case%d.npz" % c), dict(props, name="case%d" % c),
                             device_deflate="dynamic" if codes == "dynamic" else True)
    del dev
    torch.cuda.empty_cache()
    rec = {"step": "merge", "codes": codes, "cases": 3, "folders": 2,
           "npz_bytes": os.path.getsize(os.path.join(folders[0], "case0.npz"))}
    kept = []
    writer = lambda seg, path, properties: kept.append(seg.tobytes()) if path.endswith("case0.nii.gz") else None
    for threads in (1, 8):
        for flag in (False, True):
            target = os.path.join(out, "merged_%s_t%d_%d" % (codes, threads, flag))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            merge_folders(folders, target, threads, writer=writer, device_inflate=flag)
            torch.cuda.synchronize()
            rec["threads_%d_%s_s" % (threads, "device_inflate" if flag else "default")] = round(time.perf_counter() - t0, 3)
    rec["same_content"] = len(kept) == 4 and all(k == kept[0] for k in kept)
    return rec


STEPS = [["kernels", "probs", "fixed"], ["kernels", "probs", "dynamic"], ["kernels", "stage", "fixed"], ["kernels", "stage", "dynamic"],
         ["load", "probs", "fixed"], ["load", "probs", "dynamic"], ["load", "stage", "fixed"], ["load", "stage", "dynamic"],
         ["merge", "dynamic"]]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("out", help="folder for the files the steps write")
    ap.add_argument("step", nargs="*", help="kernels CASE CODES | load CASE CODES | merge CODES; default: all of them, one child each")
    args = ap.parse_args(argv)
    os.makedirs(args.out, exist_ok=True)
    if not args.step:
        for step in STEPS:                       # a fresh process per step, each under its own limit; nothing follows a failure
            done = subprocess.run([sys.executable, os.path.abspath(__file__), args.out] + step, timeout=STEP_LIMIT_S)
            if done.returncode != 0:
                raise SystemExit("inflate_bench: step %s ended with status %d; the steps behind it were not run"
                                 % (" ".join(step), done.returncode))
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("inflate_bench needs a GPU: it times device kernels and the device route of load_npz")
    run = {"kernels": kernels, "load": load, "merge": merge}[args.step[0]]
    print(json.dumps(dict(run(args.out, *args.step[1:]), cpus=len(os.sched_getaffinity(0)))), flush=True)


if __name__ == "__main__":
    main()
