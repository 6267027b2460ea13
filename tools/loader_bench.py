"""What the training step waits for in front of the augmenter: the host loader against the resident loader.

Eight synthetic BraTS-shaped preprocessed cases ([5, 138..145, 170, 140] fp32 as .npy, written to a temporary folder), the trainer's
loader patch for a 128^3 training patch (default rotation and scale ranges), batch 2.  Prints
  (a) ms per batch of DataLoader3D plus the upload of its page-locked batch, synchronised -- the parent behaviour, the baseline;
  (b) ms per batch of ResidentDataLoader3D in steady state (every case on the device);
  (c) ms per batch of ResidentDataLoader3D with budget 0 (every sample staged through page-locked memory);
  the bytes/s of e2e_loader_crop alone (device events);
  ms per nnUNetTrainer_simple.run_iteration over --steps steps with feed (a) and with feed (b), shiftConvPP at bench.py's shape.
Usage: python tools/loader_bench.py [--steps 20] [--batches 10] [--json FILE]"""
import argparse
import json
import os
import pickle
import random
import sys
import tempfile
import time
from collections import OrderedDict

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PLANS = {'plans_per_stage': {0: {'batch_size': 2, 'patch_size': [128, 128, 128], 'num_pool_per_axis': [5, 5, 5],
                                 'pool_op_kernel_sizes': [[2, 2, 2]] * 5, 'conv_kernel_sizes': [[3, 3, 3]] * 6,
                                 'do_dummy_2D_data_aug': False}},
         'base_num_features': 32, 'num_modalities': 4, 'num_classes': 3, 'all_classes': [1, 2, 3],
         'transpose_forward': [0, 1, 2], 'transpose_backward': [0, 1, 2], 'conv_per_stage': 2,
         'data_identifier': "nnUNetData_plans_v2.1"}


def write_cases(folder, n_cases=8):
    os.makedirs(folder, exist_ok=True)
    rs = np.random.RandomState(0)
    base = rs.standard_normal((4, 145, 170, 140)).astype(np.float32)
    zz, yy, xx = np.meshgrid(np.arange(145), np.arange(170), np.arange(140), indexing="ij")
    for ci in range(n_cases):
        d = 138 + ci
        r2 = (zz[:d] - d // 2) ** 2 + (yy[:d] - 85 - ci) ** 2 + (xx[:d] - 70 + ci) ** 2
        seg = (r2 < 30 ** 2).astype(np.float32) + (r2 < 18 ** 2) + (r2 < 8 ** 2)
        seg[(np.abs(base[0, :d]) < 0.02)] = -1                       # voxels outside the nonzero mask
        arr = np.concatenate([np.roll(base[:, :d], ci, axis=3), seg[None]]).astype(np.float32)
        np.save(os.path.join(folder, "case_%02d.npy" % ci), arr)
        locs = OrderedDict()
        for c in (1, 2, 3):
            v = np.argwhere(seg == c)
            locs[c] = v[rs.choice(len(v), min(len(v), 10000), replace=False)]
        with open(os.path.join(folder, "case_%02d.pkl" % ci), "wb") as f:
            pickle.dump(OrderedDict(class_locations=locs, name="case_%02d" % ci), f)


def trainer(root, out, gib):
    from e2enet_medical_amd.training.network_training.nnUNetTrainer_simple import nnUNetTrainer_simple
    from e2enet_medical_amd.training.network_training.sparselearning.core_channel import Masking, CosineDecay
    tr = nnUNetTrainer_simple(PLANS, 'all', output_folder=out, dataset_directory=root, batch_dice=True, Tconv='shiftConvPP',
                              max_num_epochs=1, num_batches_per_epoch=1)
    tr.base_num_features_override = 32
    tr.resident_data_gib = gib
    torch.manual_seed(0)
    np.random.seed(0)
    net, opt = tr.initialize(True)

    class A:
        adv = False
        fix = False
        update_frequency = 1200
        final_density = 0.05
    random.seed(0)
    mask = Masking(opt, death_rate=0.5, death_mode='magnitude', death_rate_decay=CosineDecay(0.5, 1000), growth_mode='random',
                   redistribution_mode='none', args=A())
    mask.add_module(net, sparse_init='uniform', density=0.2)
    return tr, mask


def time_batches(fn, n, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batches", type=int, default=10)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "loader_bench needs a GPU"
    from e2enet_medical_amd.training.dataloading.dataset_loading import DataLoader3D
    from e2enet_medical_amd.training.dataloading.resident_loading import DeviceCaseCache, ResidentDataLoader3D, device_crop
    res = OrderedDict()
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, "Task999")
        write_cases(os.path.join(root, PLANS['data_identifier'] + "_stage0"))
        host_tr, host_mask = trainer(root, os.path.join(tmp, "host"), None)
        patch, final = tuple(int(v) for v in host_tr.basic_generator_patch_size), tuple(int(v) for v in host_tr.patch_size)
        res["loader_patch"], res["batch"] = list(patch), int(host_tr.batch_size)
        ds = host_tr.dataset_tr
        kw = dict(oversample_foreground_percent=host_tr.oversample_foreground_percent, pad_mode="constant", memmap_mode='r')

        np.random.seed(1)
        host = DataLoader3D(ds, patch, final, host_tr.batch_size, False, **kw)

        def feed_a():
            b = next(host)
            d, s = b['data_pinned'].cuda(non_blocking=True), b['seg_pinned'].cuda(non_blocking=True)
            torch.cuda.synchronize()
            return d, s
        res["a_host_loader_plus_upload_ms"] = time_batches(feed_a, args.batches)

        np.random.seed(1)
        cache = DeviceCaseCache(None, "cuda")
        resident = ResidentDataLoader3D(ds, patch, final, host_tr.batch_size, False, cache=cache, **kw)
        for _ in range(40):                                             # until every case has been drawn
            next(resident)
            if len(cache) == len(ds):
                break
        res["b_resident_ms"] = time_batches(lambda: next(resident), args.batches)
        res["resident_cases"], res["resident_gib"] = len(cache), cache.resident_bytes / 2.0 ** 30

        np.random.seed(1)
        staged = ResidentDataLoader3D(ds, patch, final, host_tr.batch_size, False, cache=DeviceCaseCache(0, "cuda"), **kw)
        res["c_staged_ms"] = time_batches(lambda: next(staged), args.batches)

        # the kernel alone: two resident cases, a corner that leaves the case on both sides like the loader's draws do
        srcs = [cache.fetch(ds[k])[0] for k in list(ds.keys())[:host_tr.batch_size]]
        offs = [[(s.shape[1 + a] - patch[a]) // 2 for a in range(3)] for s in srcs]
        C = srcs[0].shape[0] - 1
        for _ in range(3):
            device_crop(srcs, offs, C, patch, 0, 0.0, -1.0, "cuda")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            device_crop(srcs, offs, C, patch, 0, 0.0, -1.0, "cuda")
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 20
        written = len(srcs) * (C + 1) * int(np.prod(patch)) * 4
        read = sum((C + 1) * int(np.prod([min(s.shape[1 + a], patch[a]) for a in range(3)])) * 4 for s in srcs)
        res["kernel_ms"], res["kernel_bytes_written"], res["kernel_bytes_read"] = ms, written, read
        res["kernel_gb_per_s"] = (written + read) / ms / 1e6
        del staged, resident, host, srcs

        def steps(tr, mask):
            for _ in range(3):
                tr.run_iteration(tr.tr_gen, True, False, mask)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                tr.run_iteration(tr.tr_gen, True, False, mask)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / args.steps * 1e3
        res["step_ms_feed_a"] = steps(host_tr, host_mask)
        del host_tr, host_mask
        torch.cuda.empty_cache()
        res_tr, res_mask = trainer(root, os.path.join(tmp, "resident"), -1)
        for _ in range(40):
            next(res_tr.dl_tr)
            if len(res_tr.dl_tr.cache) == len(ds):
                break
        res["step_ms_feed_b"] = steps(res_tr, res_mask)
        res["log_line"] = res_tr.dl_tr.residency_report()
    for k, v in res.items():
        print("%-32s %s" % (k, ("%.3f" % v) if isinstance(v, float) else v))
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
