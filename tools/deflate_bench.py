#!/usr/bin/env python
"""Device deflate against the host route it can replace (diagnostic, not gated): time to a finished file and the file's size.

   python tools/deflate_bench.py OUT [--shape D H W] [--classes K] [--repeats R] [--npz FILE ...] [--skip labels|probs]

   labels   a synthetic uint8 label volume (blobs of K - 1 classes in background, shape + (6, 12, 12) as an uncropped case has):
            nifti.write (download, gzip level 6 on the host)   against   nifti.write(device_deflate=True)  and  (device_deflate="dynamic")
   probs    synthetic fp16 class probabilities [K, D, H, W] (confident over smooth regions, noisy at the borders):
            download + np.savez_compressed (what save_softmax_npz does)   against   deflate.savez  and  deflate.savez(codes="dynamic")
   --npz    the first array of a real .npz (a saved prediction), uploaded once before the clock starts: the same three routes

Every route starts from the tensor resident on the device and ends with the closed file, so the time includes the download and the
write.  Host clock around work that ends in a device synchronise; one warm-up of each route, then R repeats with the three routes
alternating; median, minimum and maximum are reported.  The device routes are also split: the two encoder passes and the CRC (device
events), the bytes that cross the link, and for the dynamic codes the share of chunks per form (stored, fixed, dynamic).  Each case
prints one JSON line.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(times):
    return {"median_s": round(float(np.median(times)), 4), "min_s": round(min(times), 4), "max_s": round(max(times), 4),
            "n": len(times)}


def _alternate(routes, repeats):
    """routes: name -> callable that leaves a file and returns its path.  One warm-up each, then alternating repeats."""
    import torch
    sizes = {}
    for name, call in routes.items():
        sizes[name] = os.path.getsize(call())
    times = {name: [] for name in routes}
    for _ in range(repeats):
        for name, call in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    return {name: dict(_stats(times[name]), file_bytes=sizes[name]) for name in routes}


def _device_split(dev, repeats, codes="fixed"):
    """a device route's own parts: encoder + CRC kernels and the gather (device events), compressed bytes downloaded, and the share
    of chunks per form"""
    import torch
    from e2enet_medical_amd import deflate
    kinds = deflate.chunk_kinds(dev, None, codes)
    ms, nbytes = [], 0
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        stream, _, _ = deflate.raw_deflate(dev, None, codes)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
        nbytes = len(stream)
    raw = dev.numel() * dev.element_size()
    return {"raw_deflate_ms_median": round(float(np.median(ms)), 3), "raw_deflate_ms_min": round(min(ms), 3),
            "raw_deflate_ms_max": round(max(ms), 3), "input_bytes": raw, "stream_bytes": nbytes,
            "input_gb_per_s": round(raw / (float(np.median(ms)) * 1e-3) / 1e9, 2),
            "chunk_share": {name: round(float((kinds == k).mean()), 4) if kinds.size else 0.0
                            for k, name in enumerate(("stored", "fixed", "dynamic"))}}


def labels(out, shape, classes, repeats):
    import torch
    from e2enet_medical_amd import nifti
    D, H, W = (shape[0] + 6, shape[1] + 12, shape[2] + 12)
    zz, yy, xx = torch.meshgrid(*[torch.arange(s, device="cuda", dtype=torch.float32) for s in (D, H, W)], indexing="ij")
    field = torch.sin(zz * 0.031) + torch.sin(yy * 0.023) + torch.sin(xx * 0.019)            # smooth regions, as organs are
    seg = torch.clamp((field - 0.6) * (classes - 1) / 2.4, 0, classes - 1).to(torch.uint8).contiguous()
    del zz, yy, xx, field
    props = {"itk_spacing": (0.8, 0.8, 2.0), "itk_origin": (0., 0., 0.), "itk_direction": (1., 0., 0., 0., 1., 0., 0., 0., 1.)}
    a, b, c = (os.path.join(out, "labels_%s.nii.gz" % n) for n in ("host", "device", "dynamic"))

    def host():
        nifti.write(seg, a, props)
        return a

    def device():
        nifti.write(seg, b, props, device_deflate=True)
        return b

    def dynamic():
        nifti.write(seg, c, props, device_deflate="dynamic")
        return c
    rec = {"case": "labels", "shape": [D, H, W], "foreground_share": round(float((seg != 0).float().mean().item()), 3)}
    rec.update(_alternate({"host_gzip6": host, "device_deflate": device, "device_dynamic": dynamic}, repeats))
    rec["device_parts"] = _device_split(seg, repeats)
    rec["dynamic_parts"] = _device_split(seg, repeats, "dynamic")
    import gzip
    rec["same_content"] = gzip.decompress(open(a, "rb").read()) == gzip.decompress(open(b, "rb").read()) == \
        gzip.decompress(open(c, "rb").read())
    return rec


def _probs_routes(out, tag, dev, repeats):
    from e2enet_medical_amd import deflate
    a, b, c = (os.path.join(out, tag + "_%s.npz" % n) for n in ("host", "device", "dynamic"))
    downloads = []

    def host():
        t0 = time.perf_counter()
        arr = dev.cpu().numpy()
        downloads.append(time.perf_counter() - t0)
        np.savez_compressed(a, softmax=arr)
        return a

    def device():
        deflate.savez(b, softmax=dev)
        return b

    def dynamic():
        deflate.savez(c, codes="dynamic", softmax=dev)
        return c
    rec = _alternate({"host_savez_compressed": host, "device_deflate": device, "device_dynamic": dynamic}, repeats)
    rec["host_savez_compressed"]["of_which_download_s_median"] = round(float(np.median(downloads[1:])), 4)
    rec["device_parts"] = _device_split(dev, repeats)
    rec["dynamic_parts"] = _device_split(dev, repeats, "dynamic")
    x = np.load(a)["softmax"]
    rec["same_content"] = all(bool(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes())
                              for y in (np.load(b)["softmax"], np.load(c)["softmax"]))
    return rec


def synthetic_probs(shape, classes):
    """the fp16 class probabilities [K, D, H, W] of the ``probs`` case on the device (tools/inflate_bench.py reads them back)"""
    import torch
    D, H, W = shape
    K = classes
    g = torch.Generator(device="cuda").manual_seed(1)
    zz, yy, xx = torch.meshgrid(*[torch.arange(s, device="cuda", dtype=torch.float32) for s in (D, H, W)], indexing="ij")
    # confident probabilities over smooth regions, as a trained network leaves them: most values are 0 or 1 in fp16
    field = torch.sin(zz * 0.031) + torch.sin(yy * 0.023) + torch.sin(xx * 0.019)
    del zz, yy, xx
    dev = torch.empty((K, D, H, W), dtype=torch.float16, device="cuda")
    logits = torch.stack([-(field * K / 6.0 + K / 2.0 - k) ** 2 for k in range(K)]) * 8.0
    logits += torch.rand(logits.shape, generator=g, device="cuda")
    dev.copy_(torch.softmax(logits, 0))
    return dev


def probs(out, shape, classes, repeats):
    D, H, W = shape
    K = classes
    dev = synthetic_probs(shape, classes)
    rec = {"case": "probs", "shape": [K, D, H, W], "dtype": "float16",
           "share_exactly_0_or_1": round(float(((dev == 0) | (dev == 1)).float().mean().item()), 3)}
    rec.update(_probs_routes(out, "probs", dev, repeats))
    return rec


def real_npz(out, path, repeats):
    import torch
    with np.load(path) as f:
        key = "softmax" if "softmax" in f.files else f.files[0]
        arr = np.ascontiguousarray(f[key])
    dev = torch.from_numpy(arr).cuda()
    rec = {"case": "npz", "file": os.path.basename(path), "key": key, "shape": list(arr.shape), "dtype": str(arr.dtype),
           "file_bytes_as_given": os.path.getsize(path)}
    rec.update(_probs_routes(out, "real_" + os.path.splitext(os.path.basename(path))[0], dev, repeats))
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("out", help="folder for the files the routes write")
    ap.add_argument("--shape", type=int, nargs=3, default=[220, 400, 400], metavar=("D", "H", "W"))
    ap.add_argument("--classes", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--npz", nargs="*", default=[])
    ap.add_argument("--skip", nargs="*", default=[], choices=["labels", "probs"])
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("deflate_bench needs a GPU: both routes start from a tensor on the device")
    os.makedirs(args.out, exist_ok=True)
    cpus = len(os.sched_getaffinity(0))
    if "labels" not in args.skip:
        print(json.dumps(dict(labels(args.out, args.shape, args.classes, args.repeats), cpus=cpus)), flush=True)
    if "probs" not in args.skip:
        print(json.dumps(dict(probs(args.out, args.shape, args.classes, args.repeats), cpus=cpus)), flush=True)
    for path in args.npz:
        print(json.dumps(dict(real_npz(args.out, path, args.repeats), cpus=cpus)), flush=True)


if __name__ == "__main__":
    main()
