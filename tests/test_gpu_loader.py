"""The resident training loader on the device: e2e_loader_crop (csrc/loader.hip) against np.pad + slice, ResidentDataLoader3D against
the reference's batches (tests/golden/dataloader.npz), and the trainer switch.  Nothing is computed, so every comparison is bit for
bit."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests.helpers import golden, synthetic_cases

pytestmark = pytest.mark.gpu

FILL = 7.5


def _expect(src, off, patch, mode, fill):
    """src [K, d, h, w] padded by np.pad (mode 0 'constant' with fill, 1 'edge') as far as the patch at `off` reaches, then sliced"""
    lo = [max(0, -off[a]) for a in range(3)]
    hi = [max(0, off[a] + patch[a] - src.shape[1 + a]) for a in range(3)]
    pad = ((0, 0),) + tuple(zip(lo, hi))
    padded = np.pad(src, pad, "edge") if mode == 1 else np.pad(src, pad, "constant", constant_values=fill)
    return padded[(slice(None),) + tuple(slice(off[a] + lo[a], off[a] + lo[a] + patch[a]) for a in range(3))]


def _crop(srcs, offs, patch, mode):
    from e2enet_medical_amd.training.dataloading.resident_loading import device_crop
    dev = [torch.from_numpy(np.ascontiguousarray(s)).cuda() for s in srcs]
    data, seg = device_crop(dev, offs, srcs[0].shape[0] - 1, patch, mode, FILL, -1.0, "cuda")
    return data.cpu().numpy(), seg.cpu().numpy()


def _check(srcs, offs, patch, mode):
    data, seg = _crop(srcs, offs, patch, mode)
    for j, (s, o) in enumerate(zip(srcs, offs)):
        want_d, want_s = _expect(s[:-1], o, patch, mode, FILL), _expect(s[-1:], o, patch, 0, -1.0)
        assert data[j].tobytes() == np.ascontiguousarray(want_d).tobytes(), ("data", j, o, mode)
        assert seg[j].tobytes() == np.ascontiguousarray(want_s).tobytes(), ("seg", j, o, mode)
    return data, seg


def _box(shape, C, seed=0):
    """[C + 1, *shape]: distinct data values, whole-number labels"""
    rs = np.random.RandomState(seed)
    a = rs.standard_normal((C + 1,) + tuple(shape)).astype(np.float32)
    a[-1] = rs.randint(0, 4, shape)
    return a


GEOMETRY = [
    # box, patch, offset
    ((3, 4, 5), (8, 9, 11), (-2, -3, -3)),            # the patch is larger than the box on every axis
    ((20, 21, 23), (8, 9, 13), (5, 6, 7)),            # wholly inside; odd row length, odd source column
    ((20, 21, 23), (8, 9, 13), (-3, 0, 0)),           # low side only
    ((20, 21, 23), (8, 9, 13), (15, 0, 0)),           # high side only
    ((20, 21, 23), (8, 9, 13), (0, -4, 18)),          # mixed: rows in front of the box, columns behind it
    ((4, 5, 1), (6, 7, 9), (-1, -1, -4)),             # a box one voxel wide
    ((20, 21, 23), (17, 19, 23), (-2, 3, -5)),        # more than one workgroup per volume, volumes on every 4-byte phase
    ((2, 4, 140), (3, 5, 249), (0, -1, -54)),         # a long odd row: fill / copy / fill
    ((6, 7, 8), (4, 5, 6), (0, 0, 20)),               # wholly outside along w
    ((6, 7, 8), (4, 5, 6), (-10, 1, 1)),              # wholly outside along d
]


@pytest.mark.parametrize("mode", [0, 1], ids=["constant", "edge"])
@pytest.mark.parametrize("C", [1, 5])
@pytest.mark.parametrize("box,patch,off", GEOMETRY)
def test_crop_equals_np_pad_and_slice(box, patch, off, C, mode):
    _check([_box(box, C, seed=C)], [off], patch, mode)


@pytest.mark.parametrize("mode", [0, 1], ids=["constant", "edge"])
def test_a_patch_outside_the_box_is_fill_or_the_border_plane(mode):
    src = _box((6, 7, 8), 2, seed=3)
    data, seg = _check([src], [(0, 0, 20)], (4, 5, 6), mode)
    assert (seg == -1.0).all()
    if mode == 0:
        assert (data == FILL).all()
    else:
        assert np.array_equal(data[0], np.broadcast_to(src[:2, 0:4, 0:5, 7:8], (2, 4, 5, 6)))


@pytest.mark.parametrize("mode", [0, 1], ids=["constant", "edge"])
@pytest.mark.parametrize("full", [False, True], ids=["B1", "Bmax"])
def test_every_sample_has_its_own_box_and_offset(full, mode):
    from e2enet_medical_amd._lib import lib
    B = lib().loader_crop_max_batch() if full else 1
    assert B >= 16 or not full
    rs = np.random.RandomState(11)
    patch = (7, 9, 10)
    srcs, offs = [], []
    for j in range(B):
        shape = tuple(int(v) for v in rs.randint(1, 14, 3))
        srcs.append(_box(shape, 3, seed=100 + j))
        offs.append(tuple(int(rs.randint(-patch[a] - 1, shape[a] + 2)) for a in range(3)))
    _check(srcs, offs, patch, mode)


@pytest.mark.parametrize("mode", [0, 1], ids=["constant", "edge"])
def test_nan_payloads_and_negative_zero_come_out_as_bytes(mode):
    rs = np.random.RandomState(5)
    bits = rs.randint(0, 2 ** 32, (3, 9, 10, 11), dtype=np.uint64).astype(np.uint32)
    bits[:, ::2] |= 0x7F800000                                       # exponent all ones: infinities and NaNs of every payload
    bits[0, 1, 1, :] = 0x80000000                                    # -0.0
    bits[2, 3, :, 4] = 0xFFC00001
    src = bits.view(np.float32)
    assert np.isnan(src).sum() > 100
    _check([src], [(-2, 1, -3)], (12, 8, 16), mode)
    _check([src], [(1, 2, 3)], (5, 6, 7), mode)


def test_source_behind_two_to_the_31():
    """[2, 1, 2, 2^30 + 2^15] fp32 (17 GiB): element 2^31 of the array is data voxel (0, 1, 2^30 - 2^15), and the seg channel begins at
    element 2^31 + 2^16"""
    from e2enet_medical_amd.training.dataloading.resident_loading import device_crop
    W = 2 ** 30 + 2 ** 15
    x0 = 2 ** 31 - W
    src = torch.zeros((2, 1, 2, W), dtype=torch.float32, device="cuda")
    assert src.numel() > 2 ** 32 and src[0, 0, 1].storage_offset() + x0 == 2 ** 31
    src[0, 0, 1, x0 - 1], src[0, 0, 1, x0], src[0, 0, 1, x0 + 5], src[0, 0, 0, x0 + 2] = 11.0, 12.0, 13.0, 14.0
    src[1, 0, 1, x0 - 1], src[1, 0, 1, x0], src[1, 0, 0, x0 + 3] = 1.0, 2.0, 3.0
    data, seg = device_crop([src], [(0, 0, x0 - 8)], 1, (1, 2, 16), 0, FILL, -1.0, "cuda")
    data, seg = data.cpu().numpy(), seg.cpu().numpy()
    del src
    torch.cuda.empty_cache()
    want_d, want_s = np.zeros((1, 1, 1, 2, 16), np.float32), np.zeros((1, 1, 1, 2, 16), np.float32)
    want_d[0, 0, 0, 1, 7], want_d[0, 0, 0, 1, 8], want_d[0, 0, 0, 1, 13], want_d[0, 0, 0, 0, 10] = 11.0, 12.0, 13.0, 14.0
    want_s[0, 0, 0, 1, 7], want_s[0, 0, 0, 1, 8], want_s[0, 0, 0, 0, 11] = 1.0, 2.0, 3.0
    assert np.array_equal(data, want_d) and np.array_equal(seg, want_s)


def test_refusals():
    from e2enet_medical_amd._lib import lib, E2EError, LoaderRec
    L = lib()
    mx = L.loader_crop_max_batch()
    src = torch.zeros((2, 3, 4, 5), device="cuda")
    out_d, out_s = torch.zeros((mx + 1, 1, 2, 2, 2), device="cuda"), torch.zeros((mx + 1, 1, 2, 2, 2), device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(recs, B, mode=0, patch=(2, 2, 2), data=out_d.data_ptr(), seg=out_s.data_ptr()):
        L.loader_crop(ctypes.addressof(recs), B, 1, patch[0], patch[1], patch[2], data, seg, mode, 0.0, -1.0, st)
    good = (LoaderRec * (mx + 1))(*[LoaderRec(src.data_ptr(), 3, 4, 5, 0, 0, 0) for _ in range(mx + 1)])
    call(good, mx)
    with pytest.raises(E2EError, match="batch %d" % (mx + 1)):
        call(good, mx + 1)
    with pytest.raises(E2EError, match="data_mode 2"):
        call(good, 1, mode=2)
    zero = (LoaderRec * 1)(LoaderRec(src.data_ptr(), 3, 0, 5, 0, 0, 0))
    with pytest.raises(E2EError, match="extent"):
        call(zero, 1)
    with pytest.raises(E2EError, match="extent"):
        call(good, 1, patch=(2, 0, 2))
    with pytest.raises(E2EError, match="null"):
        call(good, 1, data=None)
    with pytest.raises(E2EError, match="null"):
        call((LoaderRec * 1)(LoaderRec(None, 3, 4, 5, 0, 0, 0)), 1)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ the loader
def _loader(ds, mode, kw, cache):
    from e2enet_medical_amd.training.dataloading.resident_loading import ResidentDataLoader3D
    return ResidentDataLoader3D(ds, (16, 18, 20), (12, 14, 16), 4, False, oversample_foreground_percent=0.33, pad_mode=mode,
                                pad_kwargs_data=kw, cache=cache)


@pytest.mark.parametrize("budget", ["all", "none", "first_case"])
@pytest.mark.parametrize("tag,mode,kw", [("edge", "edge", None), ("const", "constant", {'constant_values': 0})])
def test_batches_equal_the_reference_whatever_the_budget(tmp_path, tag, mode, kw, budget):
    from e2enet_medical_amd.training.dataloading.resident_loading import DeviceCaseCache
    g = golden("dataloader.npz")
    ds = synthetic_cases(str(tmp_path))
    first = str(g[tag + "_keys0"][0])
    first_bytes = np.load(ds[first]['data_file'][:-4] + ".npy", "r").nbytes
    cache = DeviceCaseCache({"all": None, "none": 0, "first_case": first_bytes}[budget], "cuda")
    np.random.seed(1234)
    loader = _loader(ds, mode, kw, cache)
    assert loader.data_shape == (4, 2, 16, 18, 20) and loader.seg_shape == (4, 1, 16, 18, 20)
    kept = []
    for it in range(3):
        b = next(loader)
        kept.append(b)
        assert [str(k) for k in b['keys']] == [str(k) for k in g["%s_keys%d" % (tag, it)]]
        assert b['data'].is_cuda and b['seg'].is_cuda and b['data'].dtype == torch.float32 and "data_pinned" not in b
        assert np.array_equal(b['data'].cpu().numpy(), g["%s_data%d" % (tag, it)]), "data of batch %d" % it
        assert np.array_equal(b['seg'].cpu().numpy(), g["%s_seg%d" % (tag, it)].astype(np.float32)), "seg of batch %d" % it
        assert [p['name'] for p in b['properties']] == [str(k) for k in b['keys']]
    assert np.array_equal(np.random.randint(0, 2 ** 31 - 1, 4), g[tag + "_rng_after"])
    assert np.array_equal(kept[0]['data'].cpu().numpy(), g[tag + "_data0"])             # a batch outlives the two calls after it
    if budget == "all":
        assert len(cache) == 3 and loader.staged_samples == 0
    elif budget == "none":
        assert len(cache) == 0 and loader.staged_samples == 12
    else:
        assert len(cache) == 1 and ds[first]['data_file'] in cache and cache.resident_bytes == first_bytes
        assert 0 < loader.staged_samples < 12


@pytest.mark.parametrize("budget", [None, 0])
def test_a_resident_case_is_read_from_the_host_once(tmp_path, monkeypatch, budget):
    from e2enet_medical_amd.training.dataloading import dataset_loading
    from e2enet_medical_amd.training.dataloading.resident_loading import DeviceCaseCache
    ds = synthetic_cases(str(tmp_path))
    np.random.seed(3)
    loader = _loader(ds, "constant", None, DeviceCaseCache(budget, "cuda"))
    calls = []
    real = dataset_loading._load_case
    monkeypatch.setattr(dataset_loading, "_load_case", lambda *a, **k: calls.append(a[0]['data_file']) or real(*a, **k))
    drawn = []
    for _ in range(8):
        drawn += [str(k) for k in next(loader)['keys']]
    torch.cuda.synchronize()
    assert len(set(drawn)) == 3
    if budget is None:
        assert sorted(calls) == sorted(ds[k]['data_file'] for k in set(drawn))            # once per distinct case, then never again
    else:
        assert calls == [ds[k]['data_file'] for k in drawn]                               # once per drawn sample


# ----------------------------------------------------------------------------------------------------------------- the trainer
PLANS = {'plans_per_stage': {0: {'batch_size': 2, 'patch_size': [16, 32, 32], 'num_pool_per_axis': [3, 5, 5],
                                 'pool_op_kernel_sizes': [[2, 2, 2]] * 3 + [[1, 2, 2]] * 2,
                                 'conv_kernel_sizes': [[3, 3, 3]] * 6, 'do_dummy_2D_data_aug': False}},
         'base_num_features': 32, 'num_modalities': 1, 'num_classes': 2, 'all_classes': [1, 2],
         'transpose_forward': [0, 1, 2], 'transpose_backward': [0, 1, 2], 'conv_per_stage': 2,
         'data_identifier': "nnUNetData_plans_v2.1"}


def _write_cases(folder, n_cases=6, shape=(20, 44, 40)):
    """preprocessed cases in the reference's on-disk form: <case>.npy ([modality, seg]) + <case>.pkl (properties with
    class_locations), closed forms"""
    import pickle
    from collections import OrderedDict
    os.makedirs(folder, exist_ok=True)
    for ci in range(n_cases):
        shp = tuple(s + 2 * (ci % 3) for s in shape)
        j = np.arange(int(np.prod(shp)), dtype=np.float64).reshape(shp)
        data = np.sin(0.21 * j + 0.7 * ci).astype(np.float32)
        zz, yy, xx = np.meshgrid(*[np.arange(s) for s in shp], indexing="ij")
        seg = (((zz // 3 + yy // 5 + xx // 4 + ci) % 5) < 2).astype(np.float32) + (((zz + yy + xx) % 17) == 0).astype(np.float32)
        seg = np.minimum(seg, 2.0)
        seg[:2] = -1                                           # nnU-Net marks voxels outside the nonzero mask with -1
        np.save(os.path.join(folder, "case_%02d.npy" % ci), np.stack([data, seg]).astype(np.float32))
        locs = OrderedDict((c, np.argwhere(seg == c)) for c in (1, 2))
        with open(os.path.join(folder, "case_%02d.pkl" % ci), "wb") as f:
            pickle.dump(OrderedDict(class_locations=locs, name="case_%02d" % ci), f)


def test_trainer_feeds_are_equal_bit_for_bit_and_the_parser_takes_the_switch(tmp_path):
    from e2enet_medical_amd.simple_main import build_parser
    from e2enet_medical_amd.training.dataloading.dataset_loading import DataLoader3D
    from e2enet_medical_amd.training.dataloading.resident_loading import ResidentDataLoader3D
    from e2enet_medical_amd.training.network_training.nnUNetTrainer_simple import nnUNetTrainer_simple
    root = tmp_path / "Task998"
    _write_cases(str(root / "nnUNetData_plans_v2.1_stage0"))

    def feed(gib, out):
        tr = nnUNetTrainer_simple(PLANS, 0, output_folder=str(tmp_path / out), dataset_directory=str(root), batch_dice=False,
                                  Tconv='shiftConvPP', max_num_epochs=1, num_batches_per_epoch=2)
        tr.base_num_features_override = 8
        assert tr.resident_data_gib is None
        tr.resident_data_gib = gib
        torch.manual_seed(0)
        tr.initialize(True)
        tr.tr_gen.fn.rs = np.random.RandomState(5)             # the augmenter's draws
        np.random.seed(7)                                      # the loaders' draws
        got = []
        for _ in range(3):
            for gen in (tr.tr_gen, tr.val_gen):
                b = next(gen)
                got.append([b["data"].cpu()] + [t.cpu() for t in b["target"]])
        return tr, got
    host_tr, host = feed(None, "host")
    res_tr, res = feed(-1, "resident")
    assert type(host_tr.dl_tr) is DataLoader3D and type(host_tr.dl_val) is DataLoader3D
    assert isinstance(res_tr.dl_tr, ResidentDataLoader3D) and res_tr.dl_tr.cache is res_tr.dl_val.cache
    assert res_tr.dl_tr.cache.budget_bytes is None and res_tr.dl_tr.staged_samples == 0
    for a, b in zip(host, res):
        assert len(a) == len(b) == 1 + res_tr._num_ds_outputs()
        for x, y in zip(a, b):
            assert x.shape == y.shape and x.numpy().tobytes() == y.numpy().tobytes()
    assert np.isfinite(float(res_tr.run_iteration(res_tr.tr_gen, True)))
    assert "cases (" in res_tr.dl_tr.residency_report()

    zero = nnUNetTrainer_simple(PLANS, 0, output_folder=str(tmp_path / "zero"), dataset_directory=str(root), Tconv='shiftConvPP')
    zero.base_num_features_override = 8
    zero.resident_data_gib = 0
    zero.initialize(True)
    assert zero.dl_tr.cache.budget_bytes == 0
    next(zero.tr_gen)
    assert len(zero.dl_tr.cache) == 0 and zero.dl_tr.staged_samples == zero.batch_size

    p = build_parser()
    assert p.parse_args(["--resident_data", "1.5"]).resident_data == 1.5 and p.parse_args([]).resident_data is None
    old = p.parse_args(["--network", "3d_fullres", "--task", "998", "--fold", "all", "--Tconv", "shiftConvPP", "--max_num_epochs", "2",
                        "--num_batches_per_epoch", "3", "--fp32", "--deterministic", "-c", "--density", "0.2", "--redistribution",
                        "none", "--base_num_features", "8", "--synthetic_data", "--disable_saving"])
    assert old.redistribution == "none" and old.resident_data is None and old.fold == "all"
