"""Device preprocessing (csrc/preprocess.hip, e2enet_medical_amd/preprocessing) against its fp64 numpy / scipy restatement
(tests/preprocess_oracle.py): crop to the non-zero region, cubic and segmentation resize, the four normalisation schemes, the whole
chain of GenericPreprocessor.preprocess_test_case, and its wiring into the trainer and into folder prediction."""
import os
import pickle

import numpy as np
import pytest
import torch

from tests import preprocess_oracle as po

pytestmark = pytest.mark.gpu

RESIZE_BAR = 3e-5            # cubic resize at unit range: fp32 coefficient storage between the prefilter passes (test_gpu_augment.py)
SEG_FLIP_CAP = 2e-4          # share of label decisions that may sit on a rounding boundary at non-dyadic ratios (test_gpu_augment.py)
NORM_BAR = 2e-6              # pointwise fp32 normalisation against fp64 (test_gpu_augment.py)


# ------------------------------------------------------------------------------------------------------------------ crop
def _crop_case():
    """[2, 19, 37, 45]: a block with a closed cavity, a tunnel to the outside, a cavity that reaches the outside only across a voxel
    diagonal, a slab on the face z = 0 with a hole lying on that face, signal in modality 1 only, and a NaN in the far corner"""
    x = np.zeros((2, 19, 37, 45), dtype=np.float32)
    x[0, 3:16, 5:31, 6:41] = 1.5
    x[0, 6:9, 10:14, 10:14] = 0          # closed cavity: filled
    x[0, 10, 20, 20:41] = 0              # tunnel that leaves the block at its x end: stays open
    x[0, 12, 25, 39] = 0                 # touches the dent below only across a diagonal: a hole under the 6-neighbour rule, filled
    x[0, 12, 26, 40] = 0                 # a dent in the block's surface: outside
    x[0, 0:2, 32:35, 2:5] = 2.0          # slab on the face z = 0 ...
    x[0, 0, 33, 3] = 0                   # ... with a hole that lies on the face: not filled
    x[1, 4:7, 31:35, 10:15] = -3.0       # signal in modality 1 only
    x[1, 18, 36, 44] = np.nan            # non-zero: widens the box to the far corner
    return x


def test_crop_case_against_the_oracle():
    from e2enet_medical_amd.preprocessing import create_nonzero_mask, crop_to_nonzero, get_bbox_from_mask
    x = _crop_case()
    want_mask = po.create_nonzero_mask(x)
    raw = (x[0] != 0) | (x[1] != 0)
    assert want_mask[7, 11, 11] and want_mask[12, 25, 39] and not want_mask[10, 20, 30] and not want_mask[12, 26, 40] and not want_mask[0, 33, 3]
    assert int((want_mask & ~raw).sum()) == 3 * 4 * 4 + 1
    mask = create_nonzero_mask(x)
    assert mask.dtype == bool and np.array_equal(mask, want_mask)
    assert get_bbox_from_mask(mask, 0) == po.get_bbox_from_mask(want_mask, 0) == [[0, 19], [5, 37], [2, 45]]
    d, s, box = crop_to_nonzero(x)
    wd, ws, wbox = po.crop_to_nonzero(x)
    assert box == wbox and d.dtype == np.float32 and np.array_equal(d, wd, equal_nan=True) and np.isnan(d).sum() == 1
    assert s.shape == ws.shape and np.array_equal(s, ws) and set(np.unique(s)) == {-1, 0}
    # with a seg: -1 only where the seg is 0 and the mask is off; labels stay, a label < -1 is reported and then zeroed by the cropper
    seg = np.zeros((1,) + x.shape[1:], dtype=np.float32)
    seg[0, 4:8, 6:20, 8:30] = 2
    seg[0, 17, 6, 3] = 5                 # a label off the mask keeps its value
    seg[0, 5, 6, 7] = -2
    d2, s2, box2 = crop_to_nonzero(x, seg.copy())
    wd2, ws2, _ = po.crop_to_nonzero(x, seg.copy())
    assert box2 == wbox and np.array_equal(s2, ws2) and s2.dtype == np.float32
    from e2enet_medical_amd.preprocessing import ImageCropper
    props, wprops = {"original_spacing": (1, 1, 1)}, {"original_spacing": (1, 1, 1)}
    d3, s3, props = ImageCropper.crop(x, props, seg.copy())
    _, ws3, wprops = po.crop(x, wprops, seg.copy())
    assert np.array_equal(s3, ws3) and (s3 >= -1).all() and (ws2 == -2).any()
    assert np.array_equal(props["classes"], wprops["classes"]) and list(props["classes"]) == [-2, -1, 0, 2, 5]
    assert props["crop_bbox"] == wprops["crop_bbox"] and tuple(props["size_after_cropping"]) == tuple(wprops["size_after_cropping"])


@pytest.mark.parametrize("shape,seed", [((1, 5, 11, 130), 3), ((2, 1, 23, 67), 4), ((1, 7, 9, 64), 5), ((1, 3, 4, 5), 6)])
def test_crop_random_masks_rows_across_waves_and_single_planes(shape, seed):
    """rows longer than a wave and no multiple of 64, a single plane (every voxel on a face: nothing is filled), a tiny volume"""
    from e2enet_medical_amd.preprocessing import create_nonzero_mask, crop_to_nonzero
    rng = np.random.default_rng(seed)
    x = (rng.random(shape) > 0.45).astype(np.float32) * rng.normal(size=shape).astype(np.float32)
    x[:, :, :1] = 0
    x[:, :, :, :2] = 0                   # a margin: the box is not the volume
    want = po.create_nonzero_mask(x)
    assert np.array_equal(create_nonzero_mask(x), want)
    if min(shape[1:]) >= 5:
        assert (want & ~(x != 0).any(0)).any()                  # some holes were filled
    d, s, box = crop_to_nonzero(x)
    wd, ws, wbox = po.crop_to_nonzero(x)
    assert box == wbox and np.array_equal(d, wd) and np.array_equal(s, ws)
    t = torch.from_numpy(x).cuda()                              # device tensors in, device tensors out
    dt, st, bt = crop_to_nonzero(t)
    assert dt.is_cuda and bt == wbox and np.array_equal(dt.cpu().numpy(), wd) and np.array_equal(st.cpu().numpy(), ws.astype(np.float32))


def test_crop_full_and_empty_cases():
    from e2enet_medical_amd.preprocessing import crop_to_nonzero, get_bbox_from_mask
    x = np.ones((1, 5, 6, 7), dtype=np.float32)
    d, s, box = crop_to_nonzero(x)
    assert box == [[0, 5], [0, 6], [0, 7]] and np.array_equal(d, x) and (s == 0).all()
    with pytest.raises(ValueError):
        crop_to_nonzero(np.zeros((2, 4, 5, 6), dtype=np.float32))
    with pytest.raises(ValueError):
        get_bbox_from_mask(np.zeros((4, 5, 6), dtype=bool))
    m = np.zeros((4, 5, 6), dtype=np.int64)
    m[1:3, 2, 3:6] = 7
    assert get_bbox_from_mask(m) == po.get_bbox_from_mask(m) == [[1, 3], [2, 3], [3, 6]]


# ------------------------------------------------------------------------------------------------------------------ cubic resize
CUBIC_CASES = [  # (shape [C, ...], new shape, separate axis or None)
    ((2, 9, 14, 11), (13, 9, 17), None),          # up and down at non-dyadic ratios
    ((1, 16, 16, 16), (8, 8, 8), None),           # exact halves
    ((1, 16, 16, 16), (32, 32, 32), None),        # exact doubles
    ((1, 3, 6, 5), (7, 6, 9), None),              # an axis of length 3 to 7, one unchanged axis
    ((1, 6, 20, 24), (12, 25, 30), 0),            # spacings (5, 1, 1) -> (2.5, 0.8, 0.8)
    ((1, 20, 24, 6), (25, 30, 12), 2),            # the same case with the low-resolution axis last
    ((1, 6, 20, 24), (6, 25, 30), 0),             # the separate axis keeps its length
]


@pytest.mark.parametrize("lo,hi", [(0.0, 1.0), (-1000.0, 3000.0)], ids=["unit", "ct"])      # ct: -1000 ... 3000
@pytest.mark.parametrize("shape,new,axis", CUBIC_CASES)
def test_cubic_resize(shape, new, axis, lo, hi):
    from e2enet_medical_amd.preprocessing import resample_data_or_seg
    x = po.step_case(shape, 11, lo, hi)
    if axis == 2:                                                # the transposed twin of the axis-0 case: the same numbers
        x = np.ascontiguousarray(po.step_case((shape[0], shape[3], shape[1], shape[2]), 11, lo, hi).transpose(0, 2, 3, 1))
    ax = None if axis is None else np.array([axis])
    want, _ = po.resample_data_or_seg(x, new, False, ax, 3, axis is not None)
    loose, _ = po.resample_data_or_seg(x, new, False, ax, 3, axis is not None, clip=False)
    assert loose.max() > x.max() or loose.min() < x.min()       # the step makes the cubic overshoot: the clip is exercised
    got = resample_data_or_seg(x, new, False, ax, 3, axis is not None)
    assert got.dtype == np.float32 and got.shape == (shape[0],) + tuple(new)
    assert got.max() <= x.max() and got.min() >= x.min()
    bar = RESIZE_BAR * max(1.0, float(np.abs(x).max()))
    err = float(np.abs(got.astype(np.float64) - want).max())
    print("cubic %s -> %s axis %s range [%g, %g]: max err %.3e, bar %.3e" % (shape, new, axis, x.min(), x.max(), err, bar))
    assert err <= bar
    if axis == 0 and new[0] != shape[1]:
        # the low-resolution axis last, through a transposed device view (transpose_forward = [2, 0, 1]): the same bits
        t = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 3, 1))).cuda().permute(0, 3, 1, 2)
        assert not t.is_contiguous()
        got_t = resample_data_or_seg(t, new, False, ax, 3, True)
        assert got_t.is_cuda and got_t.is_contiguous() and np.array_equal(got_t.cpu().numpy(), got)
    if axis == 2:
        twin = resample_data_or_seg(np.ascontiguousarray(x.transpose(0, 3, 1, 2)), (new[2], new[0], new[1]), False, np.array([0]), 3, True)
        assert np.array_equal(twin.transpose(0, 2, 3, 1), got)


def test_linear_data_resize_is_the_linear_preprocessor():
    from e2enet_medical_amd.preprocessing import resample_data_or_seg
    x = po.step_case((2, 9, 14, 11), 12)
    want, _ = po.resample_data_or_seg(x, (13, 9, 17), False, None, 1, False)
    got = resample_data_or_seg(x, (13, 9, 17), False, None, 1, False)
    assert float(np.abs(got - want).max()) <= 1e-6


# ------------------------------------------------------------------------------------------------------------------ seg resize
def _label_volume(shape, labels, seed):
    rng = np.random.default_rng(seed)
    coarse = rng.choice(np.array(labels, dtype=np.float32), size=tuple(-(-s // 3) for s in shape))
    return np.ascontiguousarray(np.kron(coarse, np.ones((3, 3, 3), dtype=np.float32))[tuple(slice(0, s) for s in shape)])[None]


@pytest.mark.parametrize("labels", [(-1, 0), (-1, 0, 1, 2, 5)])
def test_seg_resize_dyadic_is_exact_and_ties_go_to_the_later_label(labels):
    from e2enet_medical_amd.preprocessing import resample_data_or_seg
    seg = _label_volume((8, 12, 16), labels, 21)
    seg[0, :, :4, :8] = np.array([0, 0, -1, 0, labels[-1], 0, 0, -1], dtype=np.float32)
    if len(labels) > 2:
        seg[0, :, 4:8, :8] = np.array([1, 2, 2, 5, 5, 1, -1, 1], dtype=np.float32)
    new = (16, 24, 8)                                            # two axes doubled, the last halved: weights 0.5 / 0.5 there
    want, margin = po.resample_data_or_seg(seg, new, True, None, 1, False)
    assert (margin == 0).sum() > 50                              # voxels where two labels both reach exactly 0.5
    got = resample_data_or_seg(seg, new, True, None, 1, False)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert np.array_equal(got[0, 4:12, 2:6, :4], np.broadcast_to(np.array([0, 0, labels[-1], 0], dtype=np.float32), (8, 4, 4)))
    if len(labels) > 2:
        assert np.array_equal(got[0, 4:12, 10:14, :4], np.broadcast_to(np.array([2, 5, 5, 1], dtype=np.float32), (8, 4, 4)))


@pytest.mark.parametrize("labels", [(-1, 0), (-1, 0, 1, 2, 5)])
@pytest.mark.parametrize("shape,new,axis", [((9, 14, 11), (13, 9, 17), None), ((6, 20, 24), (12, 25, 30), 0), ((20, 24, 6), (25, 30, 6), 2)])
def test_seg_resize_non_dyadic(shape, new, axis, labels):
    from e2enet_medical_amd.preprocessing import resample_data_or_seg
    seg = _label_volume(shape, labels, 22)
    seg[0, 1, 1, 1] = -2                                         # a label < -1: resized like a label, then written as 0
    seg[0, 4:7, 4:7, 3:6] = -2
    ax = None if axis is None else np.array([axis])
    want, margin = po.resample_data_or_seg(seg, new, True, ax, 1, axis is not None)
    again, _ = po.resample_data_or_seg(seg, new, True, ax, 1, axis is not None)
    assert np.array_equal(want, again)                           # the oracle against itself is at 0
    assert (want == -2).any()
    want[want < -1] = 0
    got = resample_data_or_seg(seg, new, True, ax, 1, axis is not None)
    diff = got != want
    print("seg %s -> %s axis %s labels %s: %d of %d voxels differ" % (shape, new, axis, labels, int(diff.sum()), diff.size))
    assert diff.mean() <= SEG_FLIP_CAP
    assert (margin[diff] <= 1e-6).all()                          # only decisions on a rounding boundary may differ
    assert (got >= -1).all()


# ------------------------------------------------------------------------------------------------------------------ normalisation
IP = {c: {'mean': 80.5, 'sd': 37.25, 'percentile_00_5': -60.0, 'percentile_99_5': 210.0} for c in range(8)}
IP[5] = dict(IP[0], percentile_00_5=5000.0, percentile_99_5=6000.0)          # an empty CT2 window


def _norm_case(use_mask):
    shape = (11, 13, 17)
    rng = np.random.default_rng(31)
    data = np.stack([rng.normal(60, 90, shape), rng.normal(40, 120, shape), rng.normal(3, 2, shape), rng.normal(-5, 4, shape),
                     np.full(shape, 0.1), rng.normal(60, 90, shape)]).astype(np.float32)
    schemes = {0: "CT", 1: "CT2", 2: "noNorm", 3: "nonCT", 4: "nonCT", 5: "CT2"}       # 4: std = 0; 5: nothing inside the window
    seg = rng.choice(np.array([-1, 0, 1], dtype=np.float32), size=(1,) + shape)
    return data, seg, schemes, {c: use_mask for c in schemes}


@pytest.mark.parametrize("use_mask", [False, True])
def test_normalisation_schemes(use_mask):
    from e2enet_medical_amd.preprocessing import GenericPreprocessor
    data, seg, schemes, masks = _norm_case(use_mask)
    want = po.normalize(data, seg, schemes, masks, IP)
    pre = GenericPreprocessor(schemes, masks, [0, 1, 2], IP)
    runs = []
    for _ in range(2):
        props = {"original_spacing": np.array([1.0, 1.0, 1.0])}
        d, s, props = pre.resample_and_normalize(data.copy(), np.array([1.0, 1.0, 1.0]), props, seg.copy())
        runs.append(d)
        assert d.dtype == np.float32 and np.array_equal(s, seg) and tuple(props["size_after_resampling"]) == data.shape[1:]
    assert runs[0].tobytes() == runs[1].tobytes()                # the same bits on every run
    got = runs[0].astype(np.float64)
    inside = seg[0] >= 0
    assert np.isnan(want[5][inside if use_mask else slice(None)]).all()            # numpy: mean of an empty selection is NaN
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got[2], data[2].astype(np.float64))                       # noNorm: untouched, mask or not
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok]))
    print("normalisation use_mask=%s: max scaled err %.3e" % (use_mask, float(err.max())))
    assert err.max() <= NORM_BAR
    assert np.abs(want[4]).max() <= 1e-6 and np.abs(got[4]).max() <= 1e-6              # std = 0: a division by 1e-8, no NaN
    if use_mask:
        for c in (0, 1, 3, 4, 5):
            assert (got[c][~inside] == 0).all()


def test_normalisation_needs_a_seg_for_the_mask():
    from e2enet_medical_amd.preprocessing import GenericPreprocessor
    pre = GenericPreprocessor({0: "nonCT"}, {0: True}, [0, 1, 2])
    with pytest.raises(ValueError):
        pre.resample_and_normalize(np.ones((1, 4, 4, 4), dtype=np.float32), [1, 1, 1], {"original_spacing": [1, 1, 1]}, None)


# ------------------------------------------------------------------------------------------------------------------ whole chain
SCHEMES2 = {0: "nonCT", 1: "nonCT"}
MASKS2 = {0: False, 1: True}
TARGET = np.array([2.5, 0.5, 0.5])


def _raw_case(seed, shape=(12, 24, 26), box=((1, 11), (3, 23), (2, 24)), spacing=(5.0, 1.0, 1.0)):
    """two modalities, zero outside ``box``, a hole and a NaN inside it"""
    rng = np.random.default_rng(seed)
    x = np.zeros((2,) + shape, dtype=np.float32)
    sl = tuple(slice(a, b) for a, b in box)
    inner = tuple(b - a for a, b in box)
    x[(0,) + sl] = po.step_volume(inner, seed, 1.0, 2.0) + 0.25
    x[(1,) + sl] = rng.normal(100.0, 20.0, inner).astype(np.float32)
    x[:, box[0][0] + 2, box[1][0] + 4:box[1][0] + 7, box[2][0] + 4:box[2][0] + 8] = 0        # zero in both: a filled hole
    x[1, box[0][0] + 3, box[1][0] + 5, box[2][0] + 5] = np.nan
    x[:, box[0][0]:box[0][0] + 3, box[1][0]:box[1][0] + 5, box[2][0]:box[2][0] + 6] = 0      # a corner of the box outside the mask
    props = {"original_spacing": np.array(spacing), "original_size_of_raw_data": np.array(shape),
             "itk_spacing": tuple(spacing[::-1]), "itk_origin": (0.0, 0.0, 0.0),
             "itk_direction": (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)}
    return x, props


def _check_chain(got, x, props_in, transpose_forward=(0, 1, 2)):
    d, s, props = got
    wd, ws, wprops, resized = po.preprocess_test_case(x, props_in, TARGET, SCHEMES2, MASKS2, list(transpose_forward))
    assert d.dtype == np.float32 and d.shape == wd.shape and s.shape == ws.shape
    assert props["crop_bbox"] == wprops["crop_bbox"] and np.array_equal(props["classes"], wprops["classes"])
    assert tuple(props["size_after_cropping"]) == tuple(wprops["size_after_cropping"])
    assert tuple(props["size_after_resampling"]) == tuple(wprops["size_after_resampling"])
    assert np.array_equal(props["spacing_after_resampling"], TARGET)
    assert np.array_equal(s, ws) and s.dtype.kind == "i"        # every ratio is a power of two: no decision on a rounding boundary
    assert not np.isnan(d).any()
    for c in range(2):
        sel = resized[c][ws[0] >= 0] if MASKS2[c] else resized[c]
        tol = RESIZE_BAR * max(1.0, float(np.abs(resized[c]).max())) / float(sel.astype(np.float64).std()) \
            + NORM_BAR * np.maximum(1.0, np.abs(wd[c]))
        err = np.abs(d[c].astype(np.float64) - wd[c])
        print("chain modality %d: max err %.3e, smallest tolerance %.3e" % (c, float(err.max()), float(np.min(tol))))
        assert (err <= tol).all()
    assert (d[1][ws[0] < 0] == 0).all()
    return wprops


def test_whole_chain_in_memory():
    from e2enet_medical_amd.preprocessing import GenericPreprocessor
    x, props = _raw_case(41)
    pre = GenericPreprocessor(SCHEMES2, MASKS2, [0, 1, 2])
    wprops = _check_chain(pre.preprocess_test_case((x.copy(), dict(props)), TARGET), x, props)
    assert wprops["crop_bbox"] == [[1, 11], [3, 23], [2, 24]] and tuple(wprops["size_after_resampling"]) == (20, 40, 44)
    # the low-resolution axis last on disk, first for the network: transpose_forward = [2, 0, 1]
    xt = np.ascontiguousarray(x.transpose(0, 2, 3, 1))
    pt = dict(props, original_spacing=np.array([1.0, 1.0, 5.0]), original_size_of_raw_data=np.array(xt.shape[1:]))
    pre_t = GenericPreprocessor(SCHEMES2, MASKS2, [2, 0, 1])
    _check_chain(pre_t.preprocess_test_case((xt.copy(), dict(pt)), TARGET), xt, pt, (2, 0, 1))
    # a reader instead of the in-memory case
    got = pre.preprocess_test_case(["a_0000", "a_0001"], TARGET, reader=lambda files: (x.copy(), dict(props)))
    _check_chain(got, x, props)


# ------------------------------------------------------------------------------------------------------------------ trainer, folder
def _plans():
    from tests.test_gpu_trainer import PLANS
    stage = dict(PLANS['plans_per_stage'][0], current_spacing=TARGET)
    return dict(PLANS, plans_per_stage={0: stage}, num_modalities=2, normalization_schemes=SCHEMES2, use_mask_for_norm=MASKS2)


def _trainer(out=None):
    from e2enet_medical_amd.training.network_training.nnUNetTrainer_simple import nnUNetTrainer_simple
    tr = nnUNetTrainer_simple(_plans(), 0, output_folder=out, batch_dice=False, Tconv='shiftConvPP', max_num_epochs=1,
                              num_batches_per_epoch=2)
    tr.base_num_features_override = 8
    torch.manual_seed(0)
    tr.synthetic_data = True
    tr.initialize(True)
    return tr


def test_trainer_preprocess_patient():
    x, props = _raw_case(42)
    tr = _trainer()
    _check_chain(tr.preprocess_patient((x.copy(), dict(props))), x, props)
    tr.plans['preprocessor_name'] = "GenericPreprocessor_linearResampling"
    d, s, p = tr.preprocess_patient((x.copy(), dict(props)))
    assert d.shape == (2, 20, 40, 44) and tuple(p["size_after_cropping"]) == (10, 20, 22) and (s == -1).any()
    tr.plans['preprocessor_name'] = "PreprocessorFor2D"
    with pytest.raises(NotImplementedError):
        tr.preprocess_patient((x.copy(), dict(props)))


def test_predict_from_folder_on_raw_cases(tmp_path):
    """<case>_0000 / _0001.nii.gz files a test reader understands -> preprocess_patient -> predict_cases -> export to the original
    geometry; equal to the preprocessed-layout path fed with the device preprocessor's own output; zero outside the crop box."""
    from e2enet_medical_amd.inference.predict import predict_from_folder
    model, raw, pre = str(tmp_path / "model"), str(tmp_path / "raw"), str(tmp_path / "pre")
    os.makedirs(raw)
    os.makedirs(pre)
    tr = _trainer(model)
    tr.save_checkpoint(os.path.join(tr.output_folder, "shiftConvPP_model_final_checkpoint.model"))
    with open(os.path.join(model, "plans.pkl"), "wb") as f:
        pickle.dump(tr.plans, f)
    cases = {"resampled": _raw_case(43),                                              # (5, 1, 1) -> (2.5, 0.5, 0.5), crop box inside
             "native": _raw_case(44, shape=(18, 36, 40), box=((0, 18), (2, 36), (0, 37)), spacing=(2.5, 0.5, 0.5))}
    for name, (x, props) in cases.items():
        for m in range(2):
            with open(os.path.join(raw, "%s_%04d.nii.gz" % (name, m)), "wb") as f:
                np.savez(f, data=x[m], spacing=props["original_spacing"])

    def reader(files):
        loaded = [np.load(f) for f in files]
        x = np.stack([l["data"] for l in loaded])
        return x, dict(cases[os.path.basename(files[0])[:-12]][1], list_of_data_files=list(files))

    def predict(folder, out, **more):
        got = {}
        done = predict_from_folder(model, folder, str(tmp_path / out), [0], False, 1, 1, None, 0, 1, False,
                                   checkpoint_name="shiftConvPP_model_final_checkpoint",
                                   writer=lambda seg, path, props: got.__setitem__(os.path.basename(path)[:-7], (seg.copy(), props)), **more)
        assert sorted(os.path.basename(d)[:-7] for d in done) == sorted(cases)
        return got
    got = predict(raw, "out_raw", reader=reader)
    for name, (x, props) in cases.items():
        d, s, p = tr.preprocess_patient((x.copy(), dict(props)))
        np.save(os.path.join(pre, name + ".npy"), d)
        with open(os.path.join(pre, name + ".pkl"), "wb") as f:
            pickle.dump(p, f)
    want = predict(pre, "out_pre")
    for name, (x, props) in cases.items():
        seg, p = got[name]
        assert seg.dtype == np.uint8 and seg.shape == tuple(props["original_size_of_raw_data"]) == x.shape[1:]
        assert np.array_equal(seg, want[name][0]), name
        box = p["crop_bbox"]
        outside = np.ones(seg.shape, dtype=bool)
        outside[tuple(slice(b[0], b[1]) for b in box)] = False
        assert outside.any() and (seg[outside] == 0).all()
    assert got["resampled"][1]["crop_bbox"] == [[1, 11], [3, 23], [2, 24]]
    assert tuple(got["resampled"][1]["size_after_resampling"]) == (20, 40, 44) and tuple(got["native"][1]["size_after_resampling"]) == (18, 34, 37)
