"""Ensembling of saved class probabilities on the device (csrc/ensemble.hip, inference/ensemble_predictions.py) against numpy making
the reference's calls (tests/ensemble_oracle.py).  The contract is numpy's own arithmetic, so every comparison is for equal bits."""
import ctypes
import functools
import json
import os
import pickle

import numpy as np
import pytest
import torch

from tests import cc_oracle as co
from tests import ensemble_oracle as eo

pytestmark = pytest.mark.gpu

SHAPES = [(5, 7, 9), (12, 13, 17)]          # 315 voxels: under one 8-wide vector per lane, no multiple of 8; 2652: odd, two workgroups


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def _merge(srcs, props, regions=None, postprocessing=None, **kw):
    from e2enet_medical_amd.inference.ensemble_predictions import merge_softmax
    return merge_softmax(srcs, props, regions, postprocessing, **kw)


# ---- conversion ---------------------------------------------------------------------------------------------------------------

def _conversion_values(shape, seed):
    """fp32 [4, *shape]: random probabilities with, in front, 0, 1, exact halfway points between two fp16 values (ties to even both
    ways), values in and below the fp16 subnormal range (halfway points there, the largest value that rounds to 0) and a NaN"""
    rng = np.random.RandomState(seed)
    x = rng.rand(4, *shape).astype(np.float32)
    x[1] *= np.float32(1e-6)                                 # a plane of fp16 subnormals and underflows
    x[2] *= np.float32(6e-5)                                 # around the smallest normal, 2^-14
    special = np.array([0.0, 1.0, -0.0,
                        1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11,          # halfway: down to 1 (even), up to 1 + 2^-9
                        0.5 + 2.0 ** -12, 0.5 + 3 * 2.0 ** -12, 0.5 + 2.0 ** -12 + 2.0 ** -24,
                        2.0 ** -24, 2.0 ** -25, 2.0 ** -25 + 2.0 ** -40, 3 * 2.0 ** -25, 2.0 ** -26,     # subnormal: steps of 2^-24
                        2.0 ** -14 - 2.0 ** -25, 2.0 ** -14 - 2.0 ** -26, 1023.5 * 2.0 ** -24, 1022.5 * 2.0 ** -24,
                        65504.0, 1e-30, np.nan], dtype=np.float32)
    flat = x.reshape(4, -1)
    for k in range(4):
        flat[k, k:k + len(special)] = special
    flat[3, -1] = np.nan                                     # the last voxel of the last plane: the partial vector
    return x


@pytest.mark.parametrize("tb", [[0, 1, 2], [2, 0, 1]], ids=["identity", "201"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_softmax_to_f16_equals_astype(shape, tb):
    from e2enet_medical_amd.inference.predict import softmax_to_f16
    x = _conversion_values(shape, seed=sum(shape))
    want = eo.softmax_to_f16(x, tb)
    dev = torch.from_numpy(x).cuda()
    dims = [x.shape[1 + i] for i in tb]
    strides = [dev.stride(1 + i) for i in tb]
    got = softmax_to_f16(dev, dims, strides).cpu().numpy()
    assert got.dtype == np.float16 and got.shape == want.shape
    assert np.isnan(want).sum() >= 5 and (want == 0).any() and ((want != 0) & (np.abs(want) < 6.1e-5)).any()
    assert np.array_equal(_bits(got), _bits(want)), int((_bits(got) != _bits(want)).sum())


# ---- merge --------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _sources(k, n, shape):
    """N fp16 volumes [K, *shape], half of them near-uniform softmax, the others plain random; one NaN voxel"""
    srcs = eo.near_uniform(n, k, shape, seed=1000 * k + n)
    rng = np.random.RandomState(k + n)
    for i in range(1, n, 2):
        srcs[i] = rng.rand(k, *shape).astype(np.float16)
    srcs[n // 2][k - 1, 1, 2, 3] = np.nan
    srcs[0][0, -1, -1, -1] = np.float16(6e-8)                # a subnormal in the partial vector
    for s in srcs:
        s.setflags(write=False)
    return tuple(srcs)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("n", [1, 2, 3, 5, 16])
@pytest.mark.parametrize("k", [2, 3, 16])
def test_merge_equals_np_mean_and_argmax(k, n, shape):
    srcs = list(_sources(k, n, shape))
    props = eo.properties(shape)
    want, want_mean = eo.merge_softmax(srcs, props, return_mean=True)
    got, got_mean = _merge(srcs, props, return_mean=True)
    assert want[1, 2, 3] == k - 1 and np.isnan(want_mean[k - 1, 1, 2, 3])                # the NaN is the maximum
    assert got_mean.dtype == np.float16 and np.array_equal(_bits(got_mean), _bits(want_mean))
    assert got.dtype == np.uint8 and np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(_merge(srcs, props), want)                                    # without the mean output
    # device tensors in, the same out
    assert np.array_equal(_merge([torch.from_numpy(s.copy()).cuda() for s in srcs], props), want)


def test_decisions_are_taken_on_the_fp16_mean():
    """near-uniform probabilities: fp16 means tie (the first maximum wins) and order differently from the fp32 means; both are
    conditions on this input, checked on the oracle side, so that a kernel comparing fp32 means cannot pass"""
    srcs = eo.near_uniform(2, 3, (20, 20, 20), seed=0)
    ties, flips = eo.tie_and_flip_counts(srcs)
    print("ties", ties, "labels that differ from the fp32 mean's", flips)
    assert ties >= 1 and flips >= 1
    props = eo.properties((20, 20, 20))
    want, want_mean = eo.merge_softmax(srcs, props, return_mean=True)
    got, got_mean = _merge(srcs, props, return_mean=True)
    assert np.array_equal(_bits(got_mean), _bits(want_mean)) and np.array_equal(got, want)


def test_placement_into_the_crop_box_and_clipping():
    shape = (12, 13, 17)
    # no background anywhere: what stays 0 was not written
    srcs = [np.concatenate([np.zeros_like(s[:1]), s[1:]]) for s in _sources(3, 2, shape)]
    props = eo.properties(shape, (14, 15, 20), (1, 2, 3))
    want = eo.merge_softmax(srcs, props)
    got = _merge(srcs, props)
    assert got.shape == (14, 15, 20) and np.array_equal(got, want)
    inside = np.zeros(got.shape, bool)
    inside[1:13, 2:15, 3:20] = True
    assert (got[inside] > 0).all() and (got[~inside] == 0).all()
    # a box that runs past the original size along the middle axis: clipped there (segmentation_export.py:137)
    props = eo.properties(shape, (14, 12, 20), (1, 2, 3))
    want = eo.merge_softmax(srcs, props)
    got = _merge(srcs, props)
    assert got.shape == (14, 12, 20) and np.array_equal(got, want) and (got[1:13, 2:12, 3:20] > 0).all() and int((got > 0).sum()) == 12 * 10 * 17
    # no crop box: the volume itself
    props = {'size_after_cropping': np.array(shape), 'itk_spacing': (1.0, 1.0, 1.0)}
    assert np.array_equal(_merge(srcs, props), eo.merge_softmax(srcs, props))


def test_regions_are_thresholded_on_the_fp16_mean():
    shape = (5, 7, 9)
    rng = np.random.RandomState(4)
    srcs = [rng.rand(3, *shape).astype(np.float16) for _ in range(2)]
    # fp16 0.5 and the next value but one above it: the fp32 mean 0.500244140625 exceeds 0.5, the fp16 mean is 0.5 (tie to even)
    a, b = np.float16(0.5), np.float16(0.50048828125)
    for k in range(3):
        srcs[0][k, 2, 3, 4], srcs[1][k, 2, 3, 4] = a, b
    assert (np.float32(a) + np.float32(b)) / np.float32(2) > np.float32(0.5) and eo.mean_softmax(srcs)[0, 2, 3, 4] == np.float16(0.5)
    props = eo.properties(shape, (6, 9, 12), (1, 2, 3))
    for order in ((1, 2, 3), (2, 3, 1)):
        want = eo.merge_softmax(srcs, props, order)
        got = _merge(srcs, props, order)
        assert want[3, 5, 7] == 0 and set(np.unique(want)) == {0, 1, 2, 3}
        assert np.array_equal(got, want)


def test_refused_arguments():
    from e2enet_medical_amd._lib import lib, E2EError
    L = lib()
    st = torch.cuda.current_stream().cuda_stream
    src = torch.zeros((2, 2, 2, 2), dtype=torch.float16, device="cuda")
    seg = torch.full((8,), 9, dtype=torch.uint8, device="cuda")

    def call(n, seg_ptr, mean_ptr, k=2):
        arr = ctypes.cast((ctypes.c_void_p * max(n, 1))(*([src.data_ptr()] * n)), ctypes.c_void_p)
        L.merge_softmax_f16(arr, n, k, 2, 2, 2, seg_ptr, 2, 2, 2, 0, 0, 0, None, 0, mean_ptr, st)
    with pytest.raises(E2EError, match="17 sources, at most 16"):
        call(17, seg.data_ptr(), None)
    with pytest.raises(E2EError):
        call(0, seg.data_ptr(), None)
    with pytest.raises(E2EError, match="neither"):
        call(2, None, None)
    with pytest.raises(E2EError):
        call(2, seg.data_ptr(), None, k=0)
    with pytest.raises(E2EError, match="at most 16"):
        _merge([src] * 17, eo.properties((2, 2, 2)))
    with pytest.raises(ValueError):
        _merge([src, src[:, :1].contiguous()], eo.properties((2, 2, 2)))
    torch.cuda.synchronize()
    assert int(seg.min()) == int(seg.max()) == 9
    call(16, seg.data_ptr(), None)
    torch.cuda.synchronize()
    assert int(seg.max()) == 0


def test_other_shape_than_the_case_grid_goes_through_the_engines_resampling():
    """sources that are not on the case's grid: the fp16 mean (the kernel's) as fp32 through export_segmentation"""
    from e2enet_medical_amd.inference.predict import export_segmentation
    shape, grid = (8, 9, 10), (10, 11, 13)
    srcs = eo.near_uniform(3, 3, shape, seed=7, scale=1.0)
    props = eo.properties(grid, (12, 13, 16), (1, 2, 3), spacing=(1.0, 1.0, 1.0))
    props.update(original_spacing=np.array([1.0, 1.0, 1.0]), spacing_after_resampling=np.array([1.25, 1.25, 1.25]))
    got, mean = _merge(srcs, props, return_mean=True)
    want_mean = eo.mean_softmax(srcs)
    assert np.array_equal(_bits(mean), _bits(want_mean))
    want = export_segmentation(torch.from_numpy(want_mean.astype(np.float32)).cuda(), props)
    assert got.shape == (12, 13, 16) and np.array_equal(got, want) and got.any()


# ---- end to end ---------------------------------------------------------------------------------------------------------------

def _model_folder(root, ddir, plans, seed):
    from e2enet_medical_amd.training.network_training.nnUNetTrainer_simple import nnUNetTrainer_simple
    model = os.path.join(root, "model_%d" % seed)
    tr = nnUNetTrainer_simple(plans, 0, output_folder=model, dataset_directory=ddir, batch_dice=False, Tconv='shiftConvPP',
                              max_num_epochs=1, num_batches_per_epoch=2)
    tr.base_num_features_override = 8
    torch.manual_seed(seed)
    np.random.seed(seed)
    tr.initialize(True)
    tr.save_checkpoint(os.path.join(tr.output_folder, "shiftConvPP_model_final_checkpoint.model"))
    with open(os.path.join(model, "plans.pkl"), "wb") as f:
        pickle.dump(tr.plans, f)
    return model


def test_predict_with_save_npz_then_merge_the_folders(tmp_path):
    from tests.helpers import write_synthetic_task
    from tests.test_gpu_trainer import PLANS
    from e2enet_medical_amd.inference.predict import predict_from_folder
    from e2enet_medical_amd.inference.ensemble_predictions import merge
    from e2enet_medical_amd.postprocessing.connected_components import load_postprocessing
    ddir, plans = write_synthetic_task(str(tmp_path / "pre"), plans=dict(PLANS, transpose_forward=[0, 1, 2], transpose_backward=[0, 1, 2]),
                                       n_cases=3)
    stage = os.path.join(ddir, plans['data_identifier'] + "_stage0")
    cases = sorted(f[:-4] for f in os.listdir(stage) if f.endswith(".pkl"))
    folders = []
    for seed in (0, 1):
        model = _model_folder(str(tmp_path), ddir, plans, seed)
        out = str(tmp_path / ("pred_%d" % seed))
        labels = {}
        predict_from_folder(model, stage, out, [0], True, 1, 1, None, 0, 1, False, checkpoint_name="shiftConvPP_model_final_checkpoint",
                            writer=lambda seg, path, props: labels.__setitem__(os.path.basename(path)[:-7], seg.copy()))
        for c in cases:
            props = pickle.load(open(os.path.join(stage, c + ".pkl"), "rb"))
            soft = np.load(os.path.join(out, c + ".npz"))['softmax']
            assert soft.dtype == np.float16 and soft.shape == (3,) + tuple(int(v) for v in props['size_after_cropping'])
            stored = pickle.load(open(os.path.join(out, c + ".pkl"), "rb"))
            assert list(stored['crop_bbox']) == list(props['crop_bbox']) and 'regions_class_order' not in stored
            assert labels[c].shape == tuple(int(v) for v in props['original_size_of_raw_data'])
        folders.append(out)
    assert any((np.load(os.path.join(folders[0], c + ".npz"))['softmax'] != np.load(os.path.join(folders[1], c + ".npz"))['softmax']).any()
               for c in cases)
    # without -z nothing but the labels is written
    plain = {}
    predict_from_folder(os.path.join(str(tmp_path), "model_0"), stage, str(tmp_path / "plain"), [0], False, 1, 1, None, 0, 1, False,
                        checkpoint_name="shiftConvPP_model_final_checkpoint", writer=lambda seg, path, props: plain.__setitem__(path, seg))
    assert sorted(os.listdir(str(tmp_path / "plain"))) == ["plans.pkl"] and len(plain) == len(cases)

    vpv = 1.0
    mins = {(1, 2): 40 * vpv, 1: 3.5 * vpv, 2: 1e9}
    pp_file = str(tmp_path / "postprocessing.json")
    json.dump({"for_which_classes": [[1, 2], 1, 2], "min_valid_object_sizes": str(mins)}, open(pp_file, "w"))
    written = {}
    for threads in (1, 3):
        out = str(tmp_path / ("merged_%d" % threads))
        merge(folders, out, threads, postprocessing_file=pp_file, store_npz=True,
              writer=lambda seg, path, props: np.save(path[:-7] + ".npy", seg))
        assert os.path.isfile(os.path.join(out, "postprocessing.json"))
        written[threads] = out
    out = written[1]
    changed = 0
    for c in cases:
        srcs = [np.load(os.path.join(f, c + ".npz"))['softmax'] for f in folders]
        props = pickle.load(open(os.path.join(folders[0], c + ".pkl"), "rb"))
        want_raw, want_mean = eo.merge_softmax(srcs, props, return_mean=True)
        raw = np.load(os.path.join(out, "not_postprocessed", c + ".npy"))
        assert raw.dtype == np.uint8 and np.array_equal(raw, want_raw), c
        final = np.load(os.path.join(out, c + ".npy"))
        want_final = co.remove_all_but_the_largest_connected_component(raw.copy(), load_postprocessing(pp_file)[0], vpv, mins)[0]
        assert np.array_equal(final, want_final), c
        changed += int((final != raw).any())
        assert np.array_equal(_bits(np.load(os.path.join(out, "not_postprocessed", c + ".npz"))['softmax']), _bits(want_mean))
        assert len(pickle.load(open(os.path.join(out, "not_postprocessed", c + ".pkl"), "rb"))) == 2
        for sub in ("", "not_postprocessed"):
            a, b = (os.path.join(written[t], sub, c + ".npy") for t in (1, 3))
            assert open(a, "rb").read() == open(b, "rb").read(), (c, sub)
    assert changed >= 1
