"""Host side of the connected-component post-processing (e2enet_medical_amd/postprocessing/connected_components.py): the scipy
restatement of the removal (tests/cc_oracle.py) against what the reference's own function returned (tests/golden/postprocessing.npz,
tools/make_golden_postprocessing.py), and the decision logic of determine_postprocessing with that restatement injected, on cases
whose answers are worked out by hand in the docstrings.  Nothing here needs a device."""
import json
import os

import numpy as np
import pytest

from tests import cc_oracle as co
from e2enet_medical_amd.postprocessing import connected_components as cc

GOLDEN = co.golden_cases()
PP_KEYS = ['dc_per_class_pp_all', 'dc_per_class_pp_per_class', 'dc_per_class_raw', 'for_which_classes', 'min_valid_object_sizes',
           'num_samples', 'validation_final', 'validation_raw']


@pytest.mark.parametrize("i", range(len(GOLDEN)))
def test_restatement_equals_the_reference_golden(i):
    c = GOLDEN[i]
    vol = c["vol"].copy()
    img, removed, kept = co.remove_all_but_the_largest_connected_component(vol, c["fwc"], c["vpv"], c["mins"])
    assert img is vol and np.array_equal(img, c["out"])
    assert removed == c["removed"] and kept == c["kept"]
    assert list(removed.keys()) == list(c["removed"].keys())


def test_golden_file_covers_what_it_is_there_for():
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "postprocessing.npz")) < 100 * 1024
    assert any(c["fwc"] is None for c in GOLDEN) and any(c["mins"] is not None for c in GOLDEN)
    assert any(any(isinstance(k, tuple) for k in c["kept"]) and any(isinstance(k, int) for k in c["kept"]) for c in GOLDEN)
    assert any(None in c["kept"].values() for c in GOLDEN) and any(None in c["removed"].values() for c in GOLDEN)
    assert all((c["vol"] != c["out"]).any() for c in GOLDEN)


def _volume(boxes, shape=(2, 6, 12)):
    v = np.zeros(shape, np.uint8)
    for label, (z, y, x) in boxes:
        v[z, y, x] = label
    return v


# building blocks: A = 8 voxels, B = 6 voxels touching A along W, FAR = 6 voxels nowhere near A, STRAY = 2 voxels, alone
A = (slice(0, 2), slice(0, 2), slice(0, 2))
B_TOUCHING = (slice(0, 1), slice(0, 2), slice(2, 5))
FAR = (slice(0, 1), slice(4, 6), slice(8, 11))
STRAY = (slice(1, 2), slice(5, 6), slice(0, 2))


def _case(pred, gt, name, spacing=None):
    return (pred, gt, "/raw/%s.nii.gz" % name, "/gt/%s.nii.gz" % name, spacing)


def _search(tmp_path, cases, classes, **kw):
    written = {}
    res, final = cc.determine_postprocessing(cases, classes, str(tmp_path), "validation_raw", final_subf_name="validation_raw_postprocessed",
                                             writer=lambda vol, path, i: written.__setitem__(path, (i, vol.copy())),
                                             remove=co.remove_all_but_the_largest_connected_component, **kw)
    return res, final, written


def test_stray_blob_makes_the_joint_region_the_choice(tmp_path):
    """Ground truth: class 1 = A (8 voxels), class 2 = B touching A (6 voxels).  Prediction = ground truth + a stray 2-voxel blob of
    class 1.  Raw Dice: class 1 = 2*8 / (10 + 8) = 8/9, class 2 = 1.  As one foreground region the prediction has two objects,
    A+B (14) and the stray (2): the stray goes, class 1 rises to 1, class 2 stays 1 -> one class better, none worse: [1, 2] is
    chosen.  Per class on those volumes every class is one object already: nothing changes, nothing more is chosen."""
    gt = _volume([(1, A), (2, B_TOUCHING)])
    pred = _volume([(1, A), (2, B_TOUCHING), (1, STRAY)])
    raw = pred.copy()
    res, final, written = _search(tmp_path, [_case(pred, gt, "c0")], [1, 2])
    assert res['dc_per_class_raw'] == {"1": 8 / 9, "2": 1.0}
    assert res['dc_per_class_pp_all'] == {"1": 1.0, "2": 1.0} and res['dc_per_class_pp_per_class'] == {"1": 1.0, "2": 1.0}
    assert res['for_which_classes'] == [[1, 2]] and res['min_valid_object_sizes'] == "None" and res['num_samples'] == 1
    assert np.array_equal(final[0], gt) and np.array_equal(pred, raw), "the raw prediction must stay as it was"
    path = os.path.join(str(tmp_path), "validation_raw_postprocessed", "c0.nii.gz")
    assert list(written) == [path] and written[path][0] == 0 and np.array_equal(written[path][1], gt)
    js = json.load(open(os.path.join(str(tmp_path), "postprocessing.json")))
    assert sorted(js.keys()) == PP_KEYS
    assert js['validation_raw'] == "validation_raw" and js['validation_final'] == "validation_raw_postprocessed"
    summary = json.load(open(os.path.join(str(tmp_path), "validation_raw_postprocessed", "summary.json")))
    assert summary["results"]["mean"]["1"]["Dice"] == 1.0 and summary["results"]["all"][0]["test"] == path
    assert cc.load_postprocessing(os.path.join(str(tmp_path), "postprocessing.json")) == ([[1, 2]], None)


def test_a_class_that_gets_worse_rejects_the_joint_region_and_one_class_is_chosen(tmp_path):
    """Ground truth: class 1 = A (8), class 2 = FAR (6, no contact with A).  Prediction = ground truth + the stray class-1 blob (2).
    As one region the objects are A (8), FAR (6), stray (2): only A stays, class 1 rises 8/9 -> 1 but class 2 falls 1 -> 0: rejected.
    Per class on the RAW volumes: class 1 has A and the stray, the stray goes, 8/9 -> 1: chosen; class 2 is one object: unchanged,
    not chosen.  The final volumes are the raw ones without the stray."""
    gt = _volume([(1, A), (2, FAR)])
    pred = _volume([(1, A), (2, FAR), (1, STRAY)])
    res, final, _ = _search(tmp_path, [_case(pred, gt, "c0")], [1, 2])
    assert res['dc_per_class_raw'] == {"1": 8 / 9, "2": 1.0} and res['dc_per_class_pp_all'] == {"1": 1.0, "2": 0.0}
    assert res['dc_per_class_pp_per_class'] == {"1": 1.0, "2": 1.0}
    assert res['for_which_classes'] == [1] and np.array_equal(final[0], gt)
    # a threshold the gain of 1/9 does not clear: nothing is chosen and the final volumes are the raw ones
    res, final, _ = _search(tmp_path, [_case(pred, gt, "c0")], [1, 2], dice_threshold=0.2)
    assert res['for_which_classes'] == [] and np.array_equal(final[0], pred)


def test_a_single_class_skips_the_per_class_pass(tmp_path):
    """One foreground class: A and the stray; the region pass removes the stray (8/9 -> 1) and is chosen; the per-class pass would
    repeat it and is skipped, so dc_per_class_pp_per_class stays empty."""
    gt = _volume([(1, A)])
    pred = _volume([(1, A), (1, STRAY)])
    res, final, _ = _search(tmp_path, [_case(pred, gt, "c0")], [1])
    assert res['for_which_classes'] == [[1]] and res['dc_per_class_pp_per_class'] == {} and np.array_equal(final[0], gt)
    assert res['dc_per_class_raw'] == {"1": 8 / 9} and res['dc_per_class_pp_all'] == {"1": 1.0}


def test_advanced_postprocessing_keeps_the_smallest_kept_size_over_the_cases(tmp_path):
    """Two cases.  Case 0 (spacing 2 x 0.5 x 1.5: 1.5 per voxel): A + B touching + stray; region objects 14 and 2 voxels: kept 21.0.
    Case 1 (spacing 1 x 1 x 1): class 1 = A alone plus the stray, no class 2; region objects 8 and 2: kept 8.0.  The minimum over
    the cases is 8.0, so the second run removes only objects below 8.0: the strays (3.0 and 2.0) go, [1, 2] is chosen with
    {(1, 2): 8.0}.  Per class on those volumes nothing changes, so no per-class size is recorded."""
    gt0, pred0 = _volume([(1, A), (2, B_TOUCHING)]), _volume([(1, A), (2, B_TOUCHING), (1, STRAY)])
    gt1, pred1 = _volume([(1, A)]), _volume([(1, A), (1, STRAY)])
    cases = [_case(pred0, gt0, "c0", (2.0, 0.5, 1.5)), _case(pred1, gt1, "c1", (1.0, 1.0, 1.0))]
    res, final, written = _search(tmp_path, cases, [1, 2], advanced_postprocessing=True)
    assert res['for_which_classes'] == [[1, 2]] and res['min_valid_object_sizes'] == str({(1, 2): 8.0}) and res['num_samples'] == 2
    assert np.array_equal(final[0], gt0) and np.array_equal(final[1], gt1) and len(written) == 2
    fwc, mins = cc.load_postprocessing(os.path.join(str(tmp_path), "postprocessing.json"))
    assert fwc == [[1, 2]] and mins == {(1, 2): 8.0}
    # the stored decision applied with the restatement: a 5-voxel stray at 1.5 per voxel is 7.5 < 8.0 and goes, at 2.0 per voxel it
    # is 10.0 and stays
    big_stray = _volume([(1, A), (2, B_TOUCHING), (1, (slice(1, 2), slice(5, 6), slice(0, 5)))])
    out, removed, kept = co.remove_all_but_the_largest_connected_component(big_stray.copy(), fwc, 1.5, mins)
    assert np.array_equal(out, gt0) and removed == {(1, 2): 7.5} and kept == {(1, 2): 21.0}
    out, removed, kept = co.remove_all_but_the_largest_connected_component(big_stray.copy(), fwc, 2.0, mins)
    assert np.array_equal(out, big_stray) and removed == {(1, 2): None} and kept == {(1, 2): 28.0}


def test_load_postprocessing_round_trip(tmp_path):
    f = str(tmp_path / "pp.json")
    mins = {(1, 2, 3): 388.75, 1: 8.75}
    json.dump({'for_which_classes': [[1, 2, 3], 1], 'min_valid_object_sizes': str(mins)}, open(f, "w"))
    fwc, got = cc.load_postprocessing(f)
    assert fwc == [[1, 2, 3], 1] and got == mins and all(type(v) is float for v in got.values())
    json.dump({'for_which_classes': [2], 'min_valid_object_sizes': "None"}, open(f, "w"))
    assert cc.load_postprocessing(f) == ([2], None)
    json.dump({'for_which_classes': []}, open(f, "w"))
    assert cc.load_postprocessing(f) == ([], None)


def test_volume_per_voxel_multiplies_in_the_reference_order():
    s = (2.5, 0.8, 0.7)                                   # array-axis order (z, y, x); SimpleITK's GetSpacing is (x, y, z)
    assert cc.volume_per_voxel_of(s) == float(np.prod((0.7, 0.8, 2.5), dtype=np.float64)) and cc.volume_per_voxel_of(None) == 1.0


def test_entries_that_need_no_device_and_background():
    """an empty list and classes the volume does not hold return before anything is launched; class 0 asserts"""
    vol = _volume([(1, A)])
    img, removed, kept = cc.remove_all_but_the_largest_connected_component(vol, [], 1.0)
    assert img is vol and removed == {} and kept == {}
    img, removed, kept = cc.remove_all_but_the_largest_connected_component(vol, [3, (4, 5)], 1.0, {3: 1.0})
    assert img is vol and removed == {3: None, (4, 5): None} and kept == {3: None, (4, 5): None}
    with pytest.raises(AssertionError, match="background"):
        cc.remove_all_but_the_largest_connected_component(vol, [1, 0], 1.0)
    with pytest.raises(AssertionError, match="background"):
        cc.remove_all_but_the_largest_connected_component(vol, [(0, 1)], 1.0)
