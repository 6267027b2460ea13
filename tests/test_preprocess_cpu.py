"""Preprocessing without a GPU: the identities the oracle (tests/preprocess_oracle.py) and the device kernels are built on, and the
host logic of e2enet_medical_amd/preprocessing (the separate-z decision, the new shape's rounding, the reader fallback)."""
import os

import numpy as np
import pytest
from scipy import ndimage as ndi

from tests import preprocess_oracle as po


# ------------------------------------------------------------------------------------------------------ oracle identities
@pytest.mark.parametrize("shape,new", [((9, 14, 11), (13, 9, 17)), ((16, 16, 16), (8, 8, 8)), ((16, 16, 16), (32, 32, 32)),
                                       ((3, 6, 5), (7, 6, 9)), ((20, 24), (25, 30))])
def test_order3_zoom_is_edge_padding_prefilter_and_gather(shape, new):
    x = po.step_volume(shape, 1, 0.0, 100.0).astype(np.float64)
    ref = po.zoom(x, new, 3)
    assert np.abs(ref - po.zoom3_by_padding(x, new)).max() <= 1e-10 * 100.0
    assert ref.max() > x.max() or ref.min() < x.min()                   # the cubic overshoots at the step: the clip matters
    clipped = po.resize(x, new, 3)
    assert clipped.max() <= x.max() and clipped.min() >= x.min()


def test_fill_holes_is_background_labelling():
    rng = np.random.default_rng(2)
    for shape in ((12, 13, 14), (1, 9, 11), (7, 1, 5)):
        a = rng.random(shape) > 0.55
        if min(shape) > 8:
            a[3:9, 3:9, 3:9] = True
            a[5:7, 5:7, 5:7] = False
        assert np.array_equal(ndi.binary_fill_holes(a), po.fill_holes_by_labelling(a))


def test_order0_along_is_map_coordinates():
    for old, new in ((7, 14), (6, 12), (6, 5), (5, 13)):
        y = np.arange(old, dtype=float)[None, None, :].repeat(2, 0).repeat(3, 1)
        cm = np.array(np.meshgrid(np.arange(2), np.arange(3), (np.arange(new) + .5) * (old / new) - .5, indexing='ij'))
        assert np.array_equal(ndi.map_coordinates(y, cm, order=0, mode='nearest'), po.order0_along(y, 2, new))


def test_resize_segmentation_ties_go_to_the_later_label():
    """halving an axis puts every output voxel midway between two input voxels (weights 0.5 / 0.5): two different labels both reach
    exactly 0.5 and the one written later, the larger, stays"""
    seg = np.zeros((4, 4, 8), dtype=np.float32)
    seg[:, :] = np.array([0, 0, 1, 2, 2, 5, -1, 0], dtype=np.float32)
    out, margin = po.resize_segmentation(seg, (8, 8, 4))
    assert (margin == 0).any()
    assert np.array_equal(out, np.broadcast_to(np.array([0, 2, 5, 0], dtype=np.float32), (8, 8, 4)))


def test_crop_oracle_labels_outside_voxels():
    data = np.zeros((2, 6, 7, 8), dtype=np.float32)
    data[1, 2:5, 1:6, 2:7] = 3.0
    data[1, 3, 3, 4] = 0.0                                       # a closed cavity
    d, s, box = po.crop_to_nonzero(data)
    assert box == [[2, 5], [1, 6], [2, 7]] and d.shape == (2, 3, 5, 5) and s.shape == (1, 3, 5, 5)
    assert (s == 0).all()                                        # the cavity is filled: nothing inside the box is outside the mask
    with pytest.raises(ValueError):
        po.crop_to_nonzero(np.zeros((1, 3, 3, 3), dtype=np.float32))


# ------------------------------------------------------------------------------------------------------ host logic
def test_separate_z_decision_table():
    from e2enet_medical_amd.preprocessing.preprocessing import separate_z_plan, get_do_separate_z, get_lowres_axis
    cases = [((5, 1, 1), (2.5, 0.8, 0.8), None, True, [0]),            # anisotropic original
             ((1, 1, 1), (4, 1, 1), None, True, [0]),                  # anisotropic target only
             ((1, 1, 5), (1, 1, 1), None, True, [2]),                  # low-resolution axis last
             ((1, 1.5, 2), (1, 1, 1), None, False, None),              # below the threshold of 3
             ((3, 1, 1), (1, 1, 1), None, False, None),                # exactly 3 is not "> 3"
             ((0.24, 1.25, 1.25), (1, 1, 1), None, False, [1, 2]),     # two axes share the largest spacing
             ((1, 1, 1), (1, 1, 1), True, False, [0, 1, 2]),           # forced, but every axis has the spacing
             ((1, 2, 1), (1, 1, 1), True, True, [1]),                  # forced
             ((5, 1, 1), (2.5, 0.8, 0.8), False, False, None)]         # forbidden
    for orig, tgt, force, want_do, want_axis in cases:
        do, axis = separate_z_plan(np.array(orig), np.array(tgt), force)
        assert bool(do) == want_do, (orig, tgt, force)
        assert (axis is None and want_axis is None) or list(axis) == want_axis, (orig, tgt, force, axis)
        odo, oaxis = po.separate_z_plan(np.array(orig), np.array(tgt), force)
        assert bool(odo) == want_do and ((oaxis is None) == (axis is None))
    assert get_do_separate_z((0.24, 1.25, 1.25)) and list(get_lowres_axis((0.24, 1.25, 1.25))) == [1, 2]
    # the helpers live in one place
    from e2enet_medical_amd.inference import predict
    from e2enet_medical_amd.preprocessing import preprocessing
    assert predict.get_do_separate_z is preprocessing.get_do_separate_z and predict.get_lowres_axis is preprocessing.get_lowres_axis
    assert predict.resample_plan({'original_spacing': (0.24, 1.25, 1.25), 'spacing_after_resampling': (1, 1, 1)}) == (False, None)


def test_new_shape_rounding():
    from e2enet_medical_amd.preprocessing.preprocessing import resampled_shape
    assert list(resampled_shape((6, 20, 24), (5, 1, 1), (2.5, 0.8, 0.8))) == [12, 25, 30]
    assert list(resampled_shape((5, 7, 9), (1, 1, 1), (2, 2, 2))) == [2, 4, 4]          # np.round: halves go to the even number
    assert list(resampled_shape((3, 3, 3), (1, 1, 1), (2, 2, 2))) == [2, 2, 2]
    assert list(resampled_shape((10, 10, 10), (1, 1, 1), (1, 1, 1))) == [10, 10, 10]
    assert list(po.resampled_shape((5, 7, 9), (1, 1, 1), (2, 2, 2))) == [2, 4, 4]


def test_orders_outside_the_defaults_are_refused_before_any_device_work():
    from e2enet_medical_amd.preprocessing import resample_data_or_seg
    x = np.zeros((1, 4, 4, 4), dtype=np.float32)
    assert resample_data_or_seg(x, (4, 4, 4), False) is x                             # "no resampling necessary"
    for kwargs in (dict(is_seg=False, order=0), dict(is_seg=False, order=5), dict(is_seg=True, order=0), dict(is_seg=True, order=3),
                   dict(is_seg=False, order=3, order_z=1)):
        with pytest.raises(NotImplementedError, match="order"):
            resample_data_or_seg(x, (5, 4, 4), **kwargs)


def _no_simpleitk():
    try:
        import SimpleITK  # noqa: F401
        return False
    except ImportError:
        return True


def test_reader_fallback_and_its_messages(tmp_path):
    """A list of paths with no reader and no importable SimpleITK is refused with a NotImplementedError that contains the word
    "preprocessing", names the missing reader and no longer calls preprocessing out of scope; a given reader is used."""
    from e2enet_medical_amd.preprocessing import GenericPreprocessor, ImageCropper, default_reader
    from e2enet_medical_amd.preprocessing.cropping import require_reader
    from e2enet_medical_amd.inference.predict import predict_from_folder
    mine = lambda files: (None, {})
    assert require_reader(mine, "x") is mine
    if not _no_simpleitk():
        assert default_reader() is not None
        return
    assert default_reader() is None
    pre = GenericPreprocessor({0: 'nonCT'}, {0: False}, [0, 1, 2])
    calls = [lambda: pre.preprocess_test_case(["c_0000.nii.gz"], [1, 1, 1]),
             lambda: ImageCropper.crop_from_list_of_files(["c_0000.nii.gz"]),
             lambda: require_reader(None, "somebody")]
    import pickle
    model, raw = tmp_path / "model", tmp_path / "raw"
    os.makedirs(model)
    os.makedirs(raw)
    with open(model / "plans.pkl", "wb") as f:
        pickle.dump({'num_modalities': 1}, f)
    open(raw / "c_0000.nii.gz", "wb").close()
    calls.append(lambda: predict_from_folder(str(model), str(raw), str(tmp_path / "out"), None, False, 1, 1, None, 0, 1, True))
    for call in calls:
        with pytest.raises(NotImplementedError, match="preprocessing") as e:
            call()
        msg = str(e.value)
        assert "reader" in msg and "SimpleITK" in msg and "out of scope" not in msg
