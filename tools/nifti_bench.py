"""What a raw case costs between its .nii.gz files and the device tensor the cropping takes.

Two synthetic cases written to a temporary folder: one int16 CT volume of 300 x 512 x 512, and four float32 modalities of
155 x 240 x 240 (BraTS).  For each case, the median over --repeats of
  (a) inflate_ms: nifti.read_raw of every file -- gzip and header on the host, shared by both paths below;
  (b) host_path_ms: what the SimpleITK loader's last line does with the inflated arrays -- np.vstack([...]).astype(np.float32) on the
      host -- and the upload of that fp32 copy, 4 bytes per voxel over the link;
  (c) device_path_ms: the stored bytes uploaded as they are (elsize bytes per voxel) and decoded by e2e_nifti_decode_f32 into the
      channels of the case tensor.
(b) and (c) start from the same inflated payloads and end synchronised with the case on the device.  The two tensors are compared.
Usage: python tools/nifti_bench.py [--repeats 5] [--json FILE]"""
import argparse
import gzip
import json
import os
import struct
import sys
import tempfile
import time
from collections import OrderedDict

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = OrderedDict([("ct_int16", dict(shape=(300, 512, 512), dtype=np.int16, code=4, files=1)),
                     ("brats_4x_float32", dict(shape=(155, 240, 240), dtype=np.float32, code=16, files=4))])


def synthetic(shape, dtype, seed):
    """blocks of 8 x 8 x 8 voxels with one level each plus a little noise inside a body, zero outside: compresses like an image,
    not like noise"""
    rs = np.random.RandomState(seed)
    coarse = rs.randint(-1000, 1500, [(s + 7) // 8 for s in shape]).astype(np.float32)
    vol = np.repeat(np.repeat(np.repeat(coarse, 8, 0), 8, 1), 8, 2)[:shape[0], :shape[1], :shape[2]]
    vol = vol + rs.randint(-15, 16, shape)
    zz, yy, xx = np.ogrid[:shape[0], :shape[1], :shape[2]]
    body = ((yy - shape[1] / 2) / (0.42 * shape[1])) ** 2 + ((xx - shape[2] / 2) / (0.45 * shape[2])) ** 2 < 1
    vol = vol * body
    return (vol if np.dtype(dtype).kind == "f" else np.rint(vol)).astype(dtype)


def write_volume(path, vol, code):
    from e2enet_medical_amd import nifti
    hdr = bytearray(nifti.build_header(vol.shape, (0.8, 0.8, 2.5), (0., 0., 0.), (1., 0., 0., 0., 1., 0., 0., 0., 1.)))
    struct.pack_into("<hh", hdr, 70, code, 8 * vol.dtype.itemsize)
    with open(path, "wb") as fh, gzip.GzipFile(filename="", mode="wb", compresslevel=1, fileobj=fh, mtime=0) as gz:
        gz.write(bytes(hdr) + b"\0\0\0\0")
        gz.write(memoryview(np.ascontiguousarray(vol)).cast("B"))


def median_ms(fn, repeats):
    out, times = None, []
    for _ in range(repeats + 1):                                    # (the first run warms allocators and is dropped)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times[1:])), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "nifti_bench needs a GPU"
    from e2enet_medical_amd import nifti
    res = OrderedDict()
    with tempfile.TemporaryDirectory() as tmp:
        for name, case in CASES.items():
            files = []
            for m in range(case["files"]):
                files.append(os.path.join(tmp, "%s_%04d.nii.gz" % (name, m)))
                write_volume(files[-1], synthetic(case["shape"], case["dtype"], m), case["code"])
                print("wrote", files[-1], os.path.getsize(files[-1]) >> 20, "MiB", flush=True)
            r = res[name] = OrderedDict(shape=list(case["shape"]), files=case["files"],
                                        file_mib=sum(os.path.getsize(f) for f in files) / 2.0 ** 20)
            r["inflate_ms"], raws = median_ms(lambda: [nifti.read_raw(f) for f in files], args.repeats)
            r["payload_mib"] = sum(raw.payload.nbytes for raw in raws) / 2.0 ** 20

            def host_path():
                arrays = [np.frombuffer(raw.payload, dtype=case["dtype"]).reshape(raw.shape) for raw in raws]
                return torch.from_numpy(np.vstack([a[None] for a in arrays]).astype(np.float32)).cuda()

            def device_path():
                data = torch.empty((len(raws),) + raws[0].shape, dtype=torch.float32, device="cuda")
                for c, raw in enumerate(raws):
                    nifti.decode_f32(raw, data[c])
                return data
            r["host_path_ms"], a = median_ms(host_path, args.repeats)
            r["device_path_ms"], b = median_ms(device_path, args.repeats)
            r["equal"] = bool(torch.equal(a, b))
            del a, b, raws
    for name, r in res.items():
        for k, v in r.items():
            print("%-18s %-16s %s" % (name, k, ("%.2f" % v) if isinstance(v, float) else v))
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
