#!/usr/bin/env python
"""Device inflate of zlib's streams against the host inflate it can replace (diagnostic, not gated).

   python tools/inflate_any_bench.py OUT                    every step below as a child process of its own, each under a time limit;
                                                            the first step that fails or runs out of time ends the run
   python tools/inflate_any_bench.py OUT kernels CASE [S]   the five kernels on a resident stream (device events, median of 5 windows
                                                            of 3 calls after a warm-up) and the host's share, at segment size S
   python tools/inflate_any_bench.py OUT segments CASE      end to end inflate_any of the resident stream at S = 16, 32 and 64 KiB
   python tools/inflate_any_bench.py OUT nifti CASE         wall time of read_raw + decode_f32 on the device route against the host
                                                            route, same session (warm page cache; one warm-up, 3 alternating repeats)
   python tools/inflate_any_bench.py OUT load CASE          wall time of load_npz(foreign="device") against np.load + upload

   CASE   ct      int16 300 x 512 x 512, a smooth field plus noise, as .nii.gz through gzip level 6          (kernels, segments, nifti)
          labels  its uint8 label file                                                                        (kernels, segments, nifti)
          probs   fp16 class probabilities 16 x 220 x 400 x 400 (tools/deflate_bench.py's), np.savez_compressed (kernels, segments, load)
          stage   fp32 3 x 128 x 256 x 256 (tools/inflate_bench.py's), np.savez_compressed                   (kernels, segments, load)

Each step prints one JSON line.  Needs a GPU: there is no fallback."""
import argparse
import gzip
import json
import os
import subprocess
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from inflate_bench import _tensor, _wall, _windows                  # noqa: E402  (the same cases, windows and wall-clock rule)

STEP_LIMIT_S = 540
SEGMENTS = (16384, 32768, 65536)


def _volume(case):
    """the ct case and its labels as host arrays [300, 512, 512]"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(4)
    zz, yy, xx = torch.meshgrid(*[torch.arange(s, device="cuda", dtype=torch.float32) for s in (300, 512, 512)], indexing="ij")
    field = torch.sin(zz * 0.021) + torch.sin(yy * 0.013) + torch.sin(xx * 0.017)
    if case == "labels":
        return torch.clamp((field - 0.4) * 2.0, 0, 3).floor().to(torch.uint8).cpu().numpy()
    body = field > -1.2
    hu = (field * 300 + torch.randn(field.shape, generator=g, device="cuda") * 12).round()
    return torch.where(body, hu, torch.full_like(hu, -1024)).to(torch.int16).cpu().numpy()


def _nii_path(out, case):
    """<out>/<case>.nii.gz, written once with gzip level 6"""
    from e2enet_medical_amd import nifti
    path = os.path.join(out, case + ".nii.gz")
    if not os.path.isfile(path):
        vol = _volume(case)
        hdr = bytearray(nifti.build_header(vol.shape, (0.8, 0.8, 2.0), (0., 0., 0.), (1., 0., 0., 0., 1., 0., 0., 0., 1.)))
        if vol.dtype == np.int16:
            hdr[70:74] = np.array([4, 16], dtype="<i2").tobytes()          # datatype int16, bitpix 16
        with open(path, "wb") as fh, gzip.GzipFile(filename="", mode="wb", compresslevel=6, fileobj=fh, mtime=0) as gz:
            gz.write(bytes(hdr) + b"\0\0\0\0")
            gz.write(vol.tobytes())
    return path


def _npz_path(out, case):
    path = os.path.join(out, case + "_zlib.npz")
    if not os.path.isfile(path):
        np.savez_compressed(path, data=_tensor(case).cpu().numpy())
    return path


def _stream(out, case):
    """(raw DEFLATE stream as a uint8 array, inflated length, crc32) of a case's file"""
    from e2enet_medical_amd import deflate, nifti
    if case in ("ct", "labels"):
        data = np.fromfile(_nii_path(out, case), dtype=np.uint8)
        at, crc, isize = nifti.gzip_member(data)
        return data[at:data.size - 8].copy(), isize, crc
    m = deflate.read_npz_raw(_npz_path(out, case)).members["data"]
    return m.stream.copy(), m.size, m.crc


def kernels(out, case, seg=None):
    import torch
    from e2enet_medical_amd import deflate
    from e2enet_medical_amd._lib import lib
    S = deflate.SEGMENT_BYTES if seg is None else int(seg)
    cap = 8 * S
    stream, total, crc = _stream(out, case)
    L, st = lib(), torch.cuda.current_stream().cuda_stream
    comp = torch.from_numpy(stream).cuda()
    n, nseg = comp.numel(), -(-comp.numel() // S)
    starts_d = torch.full((nseg,), -1, dtype=torch.int64, device="cuda")
    rec = {"step": "kernels", "case": case, "segment_bytes": S, "stream_bytes": n, "inflated_bytes": total,
           "find": _windows(lambda: L.inflate_find(comp.data_ptr(), n, S, nseg, starts_d.data_ptr(), st))}
    t0 = time.perf_counter()
    found = starts_d.cpu().numpy()
    found[0] = 0
    starts = found[found >= 0]
    gaps = deflate.span_gaps(starts, n)
    rec.update(spans=int(len(starts)), largest_gap_bytes=int(gaps.max()) // 8, served=bool(gaps.max() <= 8 * cap))
    if not rec["served"]:
        return rec
    b_d = torch.from_numpy(starts).cuda()
    m = len(starts)
    records = torch.empty((m, 8), dtype=torch.int32, device="cuda")
    rec["host_compact_s"] = round(time.perf_counter() - t0, 4)
    rec["count"] = _windows(lambda: L.inflate_spans_count(comp.data_ptr(), n, b_d.data_ptr(), m, cap, records.data_ptr(), st))
    status, final, _, lengths = deflate.unpack_span_records(records.cpu().numpy().view(np.uint32))
    rec["statuses"] = sorted(set(status.tolist()))
    if status.any() or int(lengths.sum()) != total:
        return rec
    offs_d = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)).cuda()
    sym = torch.empty(total, dtype=torch.int16, device="cuda")
    wins = torch.empty(max(m, 2) * deflate.WINDOW, dtype=torch.uint8, device="cuda")
    outbuf = torch.empty(total, dtype=torch.uint8, device="cuda")
    word = torch.empty(3, dtype=torch.int32, device="cuda")
    rec["write"] = _windows(lambda: L.inflate_spans_write(comp.data_ptr(), n, b_d.data_ptr(), offs_d.data_ptr(), m, cap, sym.data_ptr(),
                                                          total, word[0:].data_ptr(), st))
    rec["windows"] = _windows(lambda: L.inflate_windows(sym.data_ptr(), offs_d.data_ptr(), m, total, wins.data_ptr(),
                                                        word[1:].data_ptr(), st))
    rec["resolve"] = _windows(lambda: L.inflate_resolve(sym.data_ptr(), offs_d.data_ptr(), m, wins.data_ptr(), outbuf.data_ptr(), total,
                                                        word[2:].data_ptr(), st))
    rec["markers"] = int((sym < 0).sum().item())
    rec["sym_bytes"], rec["window_bytes"] = 2 * total, m * deflate.WINDOW
    rec["same_content"] = bool(not word.any().item() and deflate.device_crc32(outbuf) == crc
                               and outbuf.cpu().numpy().tobytes() == zlib.decompress(stream.tobytes(), -15))
    return rec


def segments(out, case):
    import torch
    from e2enet_medical_amd import deflate
    stream, total, crc = _stream(out, case)
    comp = torch.from_numpy(stream).cuda()
    rec = {"step": "segments", "case": case, "stream_bytes": int(stream.size), "inflated_bytes": total}
    for S in SEGMENTS:
        stats = {}
        got = deflate.inflate_any(comp, total, segment_bytes=S, stats=stats)
        rec["S_%d" % S] = dict(stats, served=got is not None)
        if got is not None:
            rec["S_%d" % S].update(_windows(lambda: deflate.inflate_any(comp, total, segment_bytes=S)),
                                   same_content=deflate.device_crc32(got) == crc)
    return rec


def nifti_step(out, case):
    import torch
    from e2enet_medical_amd import nifti
    path = _nii_path(out, case)
    parts = {}

    def device():
        t0 = time.perf_counter()
        raw = nifti.read_raw(path, inflate="device")
        parts["read_raw_device_s"] = round(time.perf_counter() - t0, 4)
        return nifti.decode_f32(raw)

    def host():
        t0 = time.perf_counter()
        raw = nifti.read_raw(path)
        parts["read_raw_host_s"] = round(time.perf_counter() - t0, 4)
        return nifti.decode_f32(raw)
    rec = {"step": "nifti", "case": case, "file_bytes": os.path.getsize(path)}
    rec.update(_wall({"device_route": device, "host_route": host}))
    rec.update(parts)
    rec["deferred"] = isinstance(nifti.read_raw(path, inflate="device").payload, nifti.DeferredPayload)
    rec["same_content"] = bool(torch.equal(device(), host()))
    return rec


def load(out, case):
    import torch
    from e2enet_medical_amd import deflate
    path = _npz_path(out, case)
    stats = {}

    def device():
        return deflate.load_npz(path, stats=stats, foreign="device")["data"]

    def host():
        return torch.from_numpy(np.load(path)["data"]).cuda()
    rec = {"step": "load", "case": case, "file_bytes": os.path.getsize(path)}
    rec.update(_wall({"load_npz_foreign_device": device, "np_load_and_upload": host}))
    rec["member"] = stats["data"]
    rec["same_content"] = bool(torch.equal(device(), host()))
    return rec


STEPS = [["kernels", "ct"], ["kernels", "labels"], ["kernels", "stage"], ["kernels", "probs"],
         ["segments", "ct"], ["segments", "labels"], ["segments", "stage"], ["segments", "probs"],
         ["nifti", "ct"], ["nifti", "labels"], ["load", "stage"], ["load", "probs"]]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("out", help="folder for the files the steps write")
    ap.add_argument("step", nargs="*", help="kernels CASE [S] | segments CASE | nifti CASE | load CASE; default: all, one child each")
    args = ap.parse_args(argv)
    os.makedirs(args.out, exist_ok=True)
    if not args.step:
        for step in STEPS:                       # a fresh process per step, each under its own limit; nothing follows a failure
            done = subprocess.run([sys.executable, os.path.abspath(__file__), args.out] + step, timeout=STEP_LIMIT_S)
            if done.returncode != 0:
                raise SystemExit("inflate_any_bench: step %s ended with status %d; the steps behind it were not run"
                                 % (" ".join(step), done.returncode))
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("inflate_any_bench needs a GPU: it times device kernels and the device routes of the readers")
    run = {"kernels": kernels, "segments": segments, "nifti": nifti_step, "load": load}[args.step[0]]
    print(json.dumps(dict(run(args.out, *args.step[1:]), cpus=len(os.sched_getaffinity(0)))), flush=True)


if __name__ == "__main__":
    main()
