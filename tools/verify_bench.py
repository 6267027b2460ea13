"""What the dataset integrity check costs: the scan kernel against the bytes it must read, the nearest routes to
the same facts without it, and ``verify_dataset_integrity`` on a folder.

Two synthetic volumes of 300 x 512 x 512 (tools/nifti_bench.py's generator): an int16 label-like one (labels 0..3 in 8^3 blocks inside
a body) and a float32 image.
  scan      e2e_nifti_scan on the payload already on the device: device events, median of --windows windows of --calls calls after 3
            warm-up calls, min and max beside it; bytes = the stored payload (all the kernel reads; it writes 260 words)
  device    the same facts with the kernels the package had before: e2e_nifti_decode_f32 + torch.isnan(...).any() for the image,
            e2e_nifti_decode_u8 + torch.bincount for the label; payload on the device, host clock around calls that end with the
            answer on the host, like ``scan_call`` (the scan with its 260 words copied back)
  host      the reference's route on the converted host array: np.isnan(...).any() for both, np.unique for the label
Folder: --cases cases of one int16 image and one uint8 label, written as .nii.gz (gzip level 1); the wall time of
``verify_dataset_integrity`` at 1 and 8 threads, and its three terms summed over the files: inflate (nifti.read_raw, one thread),
upload (pageable host memory), scan.
Usage: python tools/verify_bench.py [--windows 5] [--calls 5] [--cases 3] [--json FILE]"""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time
from collections import OrderedDict

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from nifti_bench import synthetic, write_volume                                 # noqa: E402

SHAPE = (300, 512, 512)
STREAM_TBS, COPY_TBS = 5.3, 6.29          # the streaming rate of the norm / pooling passes, a device copy


def label_like(shape, seed):
    """labels 0..3 in 8^3 blocks inside the body of ``synthetic``, 0 outside"""
    return (np.abs(synthetic(shape, np.int16, seed)).astype(np.int32) // 400).clip(0, 3)


def event_windows_ms(fn, windows, calls):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / calls)
    return float(np.median(times)), float(min(times)), float(max(times))


def host_clock_ms(fn, repeats, warm=1):
    times = []
    for _ in range(warm + repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    times = times[warm:]
    return float(np.median(times)), float(min(times)), float(max(times))


def bench_volume(name, vol, code, is_label, args):
    from e2enet_medical_amd._lib import lib
    L, st = lib(), torch.cuda.current_stream().cuda_stream
    n, nbytes = vol.size, vol.nbytes
    dev = torch.from_numpy(vol.reshape(-1).view(np.uint8)).cuda()
    words = torch.empty(260, dtype=torch.int64, device="cuda")
    f32 = torch.empty(n, dtype=torch.float32, device="cuda")
    u8 = torch.empty(n, dtype=torch.uint8, device="cuda")
    rejected = torch.zeros(1, dtype=torch.int64, device="cuda")
    scan = lambda: L.nifti_scan(dev.data_ptr(), n, code, 0, 0, 1.0, 0.0, words.data_ptr(), st)
    r = OrderedDict(shape=list(vol.shape), dtype=str(vol.dtype), payload_mb=nbytes / 1e6)
    r["scan_ms"], r["scan_ms_min"], r["scan_ms_max"] = event_windows_ms(scan, args.windows, args.calls)
    r["scan_tb_per_s"] = nbytes / (r["scan_ms"] * 1e-3) / 1e12
    r["scan_share_of_stream_rate"] = r["scan_tb_per_s"] / STREAM_TBS
    r["scan_share_of_copy_rate"] = r["scan_tb_per_s"] / COPY_TBS

    def scan_call():
        scan()
        return words.cpu()

    def device_image():
        L.nifti_decode_f32(dev.data_ptr(), n, code, 0, 0, 1.0, 0.0, f32.data_ptr(), st)
        return bool(torch.isnan(f32).any().item())

    def device_label():
        rejected.zero_()
        L.nifti_decode_u8(dev.data_ptr(), n, code, 0, 0, 1.0, 0.0, u8.data_ptr(), rejected.data_ptr(), st)
        return torch.bincount(u8, minlength=256).cpu(), int(rejected.item())
    r["scan_call_ms"], r["scan_call_ms_min"], r["scan_call_ms_max"] = host_clock_ms(scan_call, args.windows * args.calls, warm=3)
    device = device_label if is_label else device_image
    r["device_route_ms"], r["device_route_ms_min"], r["device_route_ms_max"] = host_clock_ms(device, args.windows * args.calls, warm=3)
    host = (lambda: (np.isnan(vol).any(), np.unique(vol))) if is_label else (lambda: np.isnan(vol).any())
    r["host_route_ms"], r["host_route_ms_min"], r["host_route_ms_max"] = host_clock_ms(host, 3, warm=0)
    # the answers agree
    w = scan_call().numpy()
    if is_label:
        counts, bad = device_label()
        assert bad == w[0] + w[2] == 0 and np.array_equal(counts.numpy(), w[4:]) and list(np.unique(vol)) == list(np.nonzero(w[4:])[0])
    else:
        assert (w[0] > 0) == device_image() == bool(np.isnan(vol).any())
    return r


def bench_folder(tmp, args):
    from e2enet_medical_amd import nifti
    from e2enet_medical_amd.preprocessing.sanity_checks import verify_dataset_integrity
    folder = os.path.join(tmp, "Task990_VerifyBench")
    for sub in ("imagesTr", "labelsTr"):
        os.makedirs(os.path.join(folder, sub))
    cases = ["vb_%02d" % i for i in range(args.cases)]
    for i, c in enumerate(cases):
        write_volume(os.path.join(folder, "imagesTr", c + "_0000.nii.gz"), synthetic(SHAPE, np.int16, 10 + i), 4)
        write_volume(os.path.join(folder, "labelsTr", c + ".nii.gz"), label_like(SHAPE, 20 + i).astype(np.uint8), 2)
        print("wrote case", c, flush=True)
    with open(os.path.join(folder, "dataset.json"), "w") as f:
        json.dump({"modality": {"0": "CT"}, "labels": {str(k): "l%d" % k for k in range(4)}, "test": [],
                   "training": [{"image": "./imagesTr/%s.nii.gz" % c, "label": "./labelsTr/%s.nii.gz" % c} for c in cases]}, f)
    files = [os.path.join(folder, "labelsTr", c + ".nii.gz") for c in cases] + \
            [os.path.join(folder, "imagesTr", c + "_0000.nii.gz") for c in cases]
    r = OrderedDict(cases=args.cases, files=len(files), file_mib=sum(os.path.getsize(f) for f in files) / 2.0 ** 20)
    from e2enet_medical_amd._lib import lib
    L, words = lib(), torch.empty(260, dtype=torch.int64, device="cuda")
    inflate = upload = scan = 0.0
    payload = 0
    for f in files:
        for k in range(2):                                          # (the second pass is the one that counts: warm page cache)
            t0 = time.perf_counter()
            raw = nifti.read_raw(f)
            t1 = time.perf_counter()
            dev = torch.from_numpy(raw.payload).cuda()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            L.nifti_scan(dev.data_ptr(), dev.numel() // raw.elsize, raw.datatype, int(raw.swap), int(raw.scale), raw.slope, raw.inter,
                         words.data_ptr(), torch.cuda.current_stream().cuda_stream)
            words.cpu()
            t3 = time.perf_counter()
        inflate, upload, scan, payload = inflate + t1 - t0, upload + t2 - t1, scan + t3 - t2, payload + raw.payload.nbytes
        del dev, raw
    r["payload_mib"] = payload / 2.0 ** 20
    r["inflate_ms"], r["upload_ms"], r["scan_and_readback_ms"] = inflate * 1e3, upload * 1e3, scan * 1e3
    for threads in (1, 8):
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                verify_dataset_integrity(folder, threads)
            times.append((time.perf_counter() - t0) * 1e3)
        r["verify_tf%d_ms" % threads] = float(np.median(times[1:]))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--cases", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "verify_bench needs a GPU"
    res = OrderedDict()
    res["label_int16"] = bench_volume("label_int16", label_like(SHAPE, 1).astype(np.int16), 4, True, args)
    print(json.dumps(res["label_int16"]), flush=True)
    image = synthetic(SHAPE, np.float32, 2)
    res["image_float32"] = bench_volume("image_float32", image, 16, False, args)
    print(json.dumps(res["image_float32"]), flush=True)
    image[150, 256, 256] = np.nan
    res["image_float32_one_nan"] = bench_volume("image_float32_one_nan", image, 16, False, args)
    del image
    with tempfile.TemporaryDirectory() as tmp:
        res["folder"] = bench_folder(tmp, args)
    for name, r in res.items():
        for k, v in r.items():
            print("%-22s %-28s %s" % (name, k, ("%.3f" % v) if isinstance(v, float) else v))
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
