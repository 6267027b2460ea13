#!/usr/bin/env python
"""The cascade's device kernels against what they replace (diagnostic, not gated).  Each case prints one JSON line.

   python tools/cascade_bench.py [--size 128] [--repeats 20] [--skip closing|handover|augmenter ...]

   closing    one binary closing with ball(7.99) (a 16^3 footprint, 172 x-runs) of a [S, S, S] channel of smoothed-noise blobs:
              device = pack + two passes + unpack (device events around the four launches) against scipy.ndimage
              (binary_dilation, then binary_erosion with border_value=True) -- one call on one host thread, and 16 calls at once in
              16 worker processes, which is how the reference's augmentation workers would run them.  The host side runs first,
              before this process touches the GPU.  The two results are compared.
   handover   e2e_resample_argmax_u8 against resample_softmax + e2e_export_argmax_u8 for a [K, S, S, S] softmax resized to
              [2S, 2S, 2S], K = 3 and 16 (device events); the bytes each route moves are computed from the shapes.
   augmenter  DeviceAugmenter per batch (2 samples, 1 modality, patch S^3 cut from (S + S // 4)^3) with the cascade trainer's
              parameters, with the same parameters and every cascade transform forced to fire, and without the cascade (host clock
              around calls that end in a device synchronise; the same seed for all three).

Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(min(ms)), 3), "max_ms": round(float(max(ms)), 3),
            "n": len(ms)}


def _blobs(shape, seed):
    from scipy import ndimage
    f = ndimage.gaussian_filter(np.random.RandomState(seed).standard_normal(shape), 3.0, mode="wrap")
    return (f > 0).astype(np.float32)


def _host_closing(args):
    x, fp = args
    from scipy import ndimage
    t0 = time.perf_counter()
    y = ndimage.binary_erosion(ndimage.binary_dilation(x, structure=fp), structure=fp, border_value=True)
    return time.perf_counter() - t0, y


def host_closing(x, fp, workers=16, repeats=3):
    """(seconds of one call on one thread, wall seconds of `workers` calls in `workers` processes, the result)"""
    import multiprocessing as mp
    single = []
    for _ in range(repeats):
        dt, ref = _host_closing((x != 0, fp))
        single.append(dt)
    with mp.get_context("fork").Pool(workers) as pool:
        pool.map(_host_closing, [(x != 0, fp)] * workers)                  # (start the workers, touch the pages)
        walls = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            pool.map(_host_closing, [(x != 0, fp)] * workers)
            walls.append(time.perf_counter() - t0)
    return single, walls, ref


def closing(size, repeats, host):
    import torch
    from e2enet_medical_amd.training.data_augmentation import pyramid_augmentations as pa
    x, fp, (single, walls, ref) = host
    table = pa.run_table(fp)
    dev = torch.from_numpy(x[None].copy()).cuda()
    work = dev.clone()
    scratch = pa.binary_operation(work, 0, pa.CLOSING, table)
    torch.cuda.synchronize()
    same = bool(np.array_equal(work.cpu().numpy()[0], ref.astype(np.float32)))
    ms = []
    for _ in range(repeats):
        work.copy_(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        pa.binary_operation(work, 0, pa.CLOSING, table, (), scratch)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    workers = 16
    rec = {"case": "closing", "shape": [size] * 3, "radius": 7.99, "footprint": list(fp.shape), "runs": int(len(table[0])),
           "footprint_voxels": int(fp.sum()), "device": _stats(ms),
           "scipy_one_thread": _stats([1e3 * t for t in single]),
           "scipy_16_processes_wall_for_16": _stats([1e3 * t for t in walls]),
           "scipy_16_processes_per_closing_ms": round(1e3 * float(np.median(walls)) / workers, 3),
           "same_result": same,
           # what the device route moves: the channel read once, written once (fp32), the packed volume four times
           "device_bytes": int(2 * 4 * size ** 3 + 6 * (size ** 3 // 8))}
    rec["speedup_vs_one_thread"] = round(rec["scipy_one_thread"]["median_ms"] / rec["device"]["median_ms"], 1)
    rec["speedup_vs_16_processes"] = round(rec["scipy_16_processes_per_closing_ms"] / rec["device"]["median_ms"], 1)
    return rec


def handover(size, repeats, K):
    import torch
    from e2enet_medical_amd._lib import lib
    from e2enet_medical_amd.inference.predict import resample_softmax
    from e2enet_medical_amd.training.cascade_stuff.predict_next_stage import resample_argmax
    g = torch.Generator(device="cuda").manual_seed(K)
    p = torch.softmax(4.0 * torch.rand((K, size, size, size), generator=g, device="cuda"), 0).contiguous()
    out = (2 * size,) * 3
    st = torch.cuda.current_stream().cuda_stream

    def pair():
        r = resample_softmax(p, out)
        seg = torch.zeros(out, dtype=torch.uint8, device="cuda")
        lib().export_argmax_u8(r.data_ptr(), seg.data_ptr(), K, int(r.stride(0)), out[0], out[1], out[2], int(r.stride(1)),
                               int(r.stride(2)), int(r.stride(3)), out[0], out[1], out[2], 0, 0, 0, None, 0, st)
        return seg

    def fused():
        return resample_argmax(p, out)
    same = bool(torch.equal(pair(), fused()))
    times = {"pair": [], "fused": []}
    for _ in range(repeats):
        for name, fn in (("pair", pair), ("fused", fused)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1))
    vin, vout = K * size ** 3 * 4, int(np.prod(out))
    return {"case": "handover", "classes": K, "in": [K] + [size] * 3, "out": list(out), "same_result": same,
            "pair": dict(_stats(times["pair"]), bytes=int(vin + 2 * K * vout * 4 + 2 * vout)),      # (+ the zero fill of the label volume)
            "fused": dict(_stats(times["fused"]), bytes=int(vin + vout)),
            "speedup": round(float(np.median(times["pair"]) / np.median(times["fused"])), 2)}


def augmenter(size, repeats):
    import torch
    from e2enet_medical_amd.training.data_augmentation.data_augmentation_moreDA import DeviceAugmenter
    from e2enet_medical_amd.training.data_augmentation.default_data_augmentation import default_3D_augmentation_params
    big = size + size // 4
    rng = np.random.RandomState(0)
    data = torch.from_numpy(rng.standard_normal((2, 1, big, big, big)).astype(np.float32)).cuda()
    lab = np.stack([np.stack([_blobs((big,) * 3, 10 * b + c) + 2 * _blobs((big,) * 3, 10 * b + c + 5) for c in range(2)]) for b in range(2)])
    seg = torch.from_numpy(np.minimum(lab, 3).astype(np.float32)).cuda()
    ang = (-30. / 360 * 2. * np.pi, 30. / 360 * 2. * np.pi)
    base = dict(default_3D_augmentation_params, do_elastic=False, scale_range=(0.7, 1.4), rotation_x=ang, rotation_y=ang, rotation_z=ang)
    cascade = dict(base, selected_seg_channels=[0, 1], move_last_seg_chanel_to_data=True, all_segmentation_labels=[1, 2, 3],
                   cascade_do_cascade_augmentations=True, cascade_random_binary_transform_p=0.4,
                   cascade_random_binary_transform_p_per_label=1, cascade_random_binary_transform_size=(1, 8),
                   cascade_remove_conn_comp_p=0.2, cascade_remove_conn_comp_max_size_percent_threshold=0.15,
                   cascade_remove_conn_comp_fill_with_other_class_p=0.0)
    # forced: every operator and every removal fires; the size threshold (handed over swapped) is 15 % so that the labelling runs
    forced = dict(cascade, cascade_random_binary_transform_p=1.0, cascade_remove_conn_comp_p=1.0,
                  cascade_remove_conn_comp_fill_with_other_class_p=0.15)
    rec = {"case": "augmenter", "batch": [2, 1, size, size, size], "loaded_patch": [big] * 3, "labels": 3}
    for name, params, s in (("without_cascade", dict(base, selected_seg_channels=[0]), seg[:, :1].contiguous()),
                            ("cascade_trainer_defaults", cascade, seg), ("cascade_every_transform_fires", forced, seg)):
        aug = DeviceAugmenter((size,) * 3, params, seed=1, deep_supervision_scales=[[1, 1, 1], [0.5, 0.5, 0.5]])
        aug(data, s)
        torch.cuda.synchronize()
        ms, fired = [], 0
        for _ in range(repeats):
            t0 = time.perf_counter()
            aug(data, s)
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0))
            fired += sum(len(t) for t in aug.last_draws.get("cascade_binop", []))
        rec[name] = dict(_stats(ms), mean_ms=round(float(np.mean(ms)), 3), binary_operations_per_batch=round(fired / repeats, 2))
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--skip", nargs="*", default=[], choices=["closing", "handover", "augmenter"])
    args = ap.parse_args(argv)
    cpus = len(os.sched_getaffinity(0))
    host = None
    if "closing" not in args.skip:                                           # host side first: worker processes are forked before the
        from e2enet_medical_amd.training.data_augmentation.pyramid_augmentations import ball      # GPU is initialised
        x = _blobs((args.size,) * 3, 0)
        fp = ball(7.99)
        host = (x, fp, host_closing(x, fp))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("cascade_bench needs a GPU")
    if host is not None:
        print(json.dumps(dict(closing(args.size, args.repeats, host), cpus=cpus)), flush=True)
    if "handover" not in args.skip:
        for K in (3, 16):
            print(json.dumps(handover(args.size, args.repeats, K)), flush=True)
    if "augmenter" not in args.skip:
        print(json.dumps(augmenter(args.size, args.repeats)), flush=True)


if __name__ == "__main__":
    main()
