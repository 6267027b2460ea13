"""The component table on the device (csrc/components.hip: e2e_ct_label, e2e_ct_emit; postprocessing/component_table.py) against its
scipy restatement (tests/component_table_oracle.py), and the folder search built on it against the in-memory search.

Everything is exact: integer atomics only, so tables are compared field by field with array_equal, volumes with array_equal and
files byte for byte."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import component_table_oracle as cto

pytestmark = pytest.mark.gpu

CLASSES = [1, 2, 3]
FIELDS = ("first", "label", "size", "tp", "fg", "fg_first", "fg_size")


def _check(pred, gt, classes=CLASSES, on_device=False):
    """device table == restatement, and both agree with the label census; returns the device table"""
    from e2enet_medical_amd.postprocessing.component_table import component_table
    from e2enet_medical_amd.evaluation.evaluator import label_census
    want = cto.component_table(pred, gt, classes)
    got = component_table(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), classes) if on_device else component_table(pred, gt, classes)
    for name in FIELDS:
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == np.int64 and np.array_equal(a, b), (name, a[:8], b[:8], len(a), len(b))
    assert got.classes == want.classes and got.voxels == want.voxels and got.gt_count == want.gt_count
    assert np.all(np.diff(got.first) > 0) and np.all(np.diff(got.fg_first) > 0), "the records are sorted by their first voxel"
    joint, slot_of, _ = label_census(pred, gt, classes)
    for c in classes:
        k = slot_of[c]
        assert int(got.size[got.label == c].sum()) == int(joint[:, k].sum()) and int(got.tp[got.label == c].sum()) == int(joint[k, k])
        assert got.gt_count[c] == int(joint[k, :].sum())
    assert int(got.fg_size.sum()) == int(got.size.sum())
    return got


SHAPES = [(5, 7, 67), (3, 33, 130), (1, 96, 96), (17, 40, 64), (1, 1, 300)]
FILLS = [0.25, 0.35, 0.59]                             # around the site-percolation thresholds of the cubic and the square lattice


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_random_volumes_equal_the_restatement(shape, fill):
    objects = 0
    for seed in range(4):
        pred, gt = cto.random_case(shape, fill, 1000 * seed + sum(shape))
        objects += len(_check(pred, gt, on_device=bool(seed % 2)).first)
    assert objects > 20, objects


def _hand(voxels, shape=(3, 5, 7)):
    v = np.zeros(shape, np.uint8)
    for p, label in voxels:
        v[p] = label
    return v


def test_two_touching_objects_of_different_classes_in_one_foreground_object():
    pred = _hand([((0, 0, 0), 1), ((0, 0, 1), 1), ((0, 0, 2), 2), ((0, 1, 2), 2), ((1, 1, 2), 1), ((2, 4, 6), 2)])
    gt = _hand([((0, 0, 0), 1), ((0, 0, 1), 2), ((0, 0, 2), 2), ((2, 4, 6), 2)])
    t = _check(pred, gt)
    assert t.label.tolist() == [1, 2, 1, 2] and t.size.tolist() == [2, 2, 1, 1] and t.tp.tolist() == [1, 1, 0, 1]
    assert t.fg.tolist() == [0, 0, 0, 1] and t.fg_size.tolist() == [5, 1]


def test_diagonal_contact_and_row_ends_stay_separate():
    # in-plane and cross-plane diagonals; (0,2,6)|(0,3,0) and (1,4,6)|(2,0,0) are flat neighbours but no 6-neighbours
    pred = _hand([((0, 0, 0), 2), ((0, 1, 1), 2), ((1, 2, 2), 2), ((0, 2, 6), 1), ((0, 3, 0), 1), ((1, 4, 6), 3), ((2, 0, 0), 3)])
    t = _check(pred, pred.copy())
    assert len(t.first) == 7 and t.size.tolist() == [1] * 7 and t.tp.tolist() == [1] * 7 and len(t.fg_first) == 7
    # equal values that meet only through another class are two class objects in one foreground object
    pred = _hand([((1, 1, 1), 1), ((1, 1, 2), 2), ((1, 1, 3), 1)])
    t = _check(pred, np.zeros_like(pred))
    assert t.label.tolist() == [1, 2, 1] and t.fg.tolist() == [0, 0, 0] and t.fg_size.tolist() == [3] and t.tp.tolist() == [0, 0, 0]


def test_absent_class_all_background_and_a_class_value_above_127():
    pred = _hand([((0, 0, 0), 1), ((0, 0, 1), 1)])
    gt = _hand([((0, 0, 0), 1), ((2, 2, 2), 3), ((2, 2, 3), 3)])                       # class 3: in the ground truth only
    t = _check(pred, gt)
    assert t.label.tolist() == [1] and t.gt_count == {1: 1, 2: 0, 3: 2}
    zero = np.zeros((2, 3, 70), np.uint8)
    t = _check(zero, gt=_hand([((0, 0, 0), 2)], zero.shape))
    assert len(t.first) == 0 and len(t.fg_first) == 0 and t.gt_count == {1: 0, 2: 1, 3: 0} and t.voxels == zero.size
    pred = np.zeros((2, 4, 130), np.uint8)
    pred[0, 1, 60:70] = 200
    pred[0, 2, 64:66] = 131
    pred[1, 1, 62] = 200
    pred[1, 3, :] = 7                                                                   # not in the set: background to the table
    gt = pred.copy()
    gt[0, 1, 60] = 131
    t = _check(pred, gt, [131, 200])
    assert t.label.tolist() == [200, 131] and t.size.tolist() == [11, 2] and t.tp.tolist() == [10, 2] and t.fg_size.tolist() == [13]
    # a row-long run that crosses several waves, and one value per voxel
    pred = np.zeros((1, 2, 300), np.uint8)
    pred[0, 0, :] = 2
    pred[0, 1, :] = np.arange(300) % 3 + 1
    t = _check(pred, pred.copy())
    assert t.size.tolist()[0] == 300 + 100 and len(t.first) == 1 + 200 and t.fg_size.tolist() == [600]


def _raw_calls(pred, gt, members, guard=64):
    """ct_label and ct_emit of the C entry on a workspace of exactly the queried size followed by ``guard`` bytes of 0xA5, the record
    buffers of exactly the counts read, each followed by the same guard"""
    from e2enet_medical_amd._lib import lib
    L = lib()
    D, H, W = pred.shape
    n = L.ct_ws_bytes(D, H, W)
    assert n == 20 * pred.size + 128
    st = torch.cuda.current_stream().cuda_stream
    x, g = torch.from_numpy(pred.copy()).cuda(), torch.from_numpy(gt.copy()).cuda()
    ws = torch.full((n + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    res = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    words = [0] * 8
    for v in members:
        words[v >> 5] |= 1 << (v & 31)
    L.ct_label(x.data_ptr(), g.data_ptr(), D, H, W, ctypes.cast((ctypes.c_uint * 8)(*words), ctypes.c_void_p), ws.data_ptr(), res.data_ptr(), st)
    n_class, n_fg, gave_up, zero = res.cpu().tolist()
    class_rec = torch.full((n_class * 20 + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    fg_rec = torch.full((n_fg * 8 + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    L.ct_emit(x.data_ptr(), D, H, W, ws.data_ptr(), class_rec.data_ptr(), n_class, n_class, fg_rec.data_ptr(), n_fg, n_fg, st)
    torch.cuda.synchronize()
    assert np.array_equal(x.cpu().numpy(), pred) and np.array_equal(g.cpu().numpy(), gt), "the volumes are read only"
    return (n_class, n_fg, gave_up, zero), ws.cpu().numpy(), class_rec.cpu().numpy(), fg_rec.cpu().numpy(), n


@functools.lru_cache(maxsize=None)
def _percolating():
    pred, gt = cto.random_case((9, 31, 70), 0.33, 5)
    pred.setflags(write=False)
    gt.setflags(write=False)
    return pred, gt


def test_result_words_buffer_bounds_and_identical_bits_on_every_run():
    pred, gt = _percolating()
    want = cto.component_table(pred, gt, CLASSES)
    runs = [_raw_calls(pred, gt, CLASSES) for _ in range(2)]
    sorted_records = []
    for (n_class, n_fg, gave_up, zero), ws, class_rec, fg_rec, n in runs:
        assert (n_class, n_fg, gave_up, zero) == (len(want.first), len(want.fg_first), 0, 0)
        assert (ws[n:] == 0xA5).all() and (class_rec[n_class * 20:] == 0xA5).all() and (fg_rec[n_fg * 8:] == 0xA5).all(), \
            "a call wrote past the size it asked for"
        cr = class_rec[:n_class * 20].view(np.uint32).reshape(-1, 5)
        fr = fg_rec[:n_fg * 8].view(np.uint32).reshape(-1, 2)
        cr, fr = cr[np.argsort(cr[:, 0])], fr[np.argsort(fr[:, 0])]
        assert np.array_equal(cr[:, 0], want.first) and np.array_equal(cr[:, 1], want.label) and np.array_equal(cr[:, 2], want.size)
        assert np.array_equal(cr[:, 3], want.tp) and np.array_equal(cr[:, 4], want.fg_first[want.fg])
        assert np.array_equal(fr[:, 0], want.fg_first) and np.array_equal(fr[:, 1], want.fg_size)
        sorted_records.append((cr, fr))
    assert np.array_equal(sorted_records[0][0], sorted_records[1][0]) and np.array_equal(sorted_records[0][1], sorted_records[1][1])
    assert np.array_equal(runs[0][1][:20 * pred.size], runs[1][1][:20 * pred.size]), "the five arrays differ between two runs"


def test_refused_arguments_launch_nothing():
    from e2enet_medical_amd._lib import lib, E2EError
    L = lib()
    st = torch.cuda.current_stream().cuda_stream
    x = torch.full((64,), 1, dtype=torch.uint8, device="cuda")
    g = torch.full((64,), 1, dtype=torch.uint8, device="cuda")
    ws = torch.full((20 * 64 + 128,), 0xA5, dtype=torch.uint8, device="cuda")
    res = torch.full((4,), -7, dtype=torch.int64, device="cuda")
    rec = torch.full((64,), 0xA5, dtype=torch.uint8, device="cuda")
    one = [2, 0, 0, 0, 0, 0, 0, 0]

    def label(dims, words, pred=x.data_ptr(), gt=g.data_ptr(), work=ws.data_ptr(), out=res.data_ptr()):
        L.ct_label(pred, gt, *dims, ctypes.cast((ctypes.c_uint * 8)(*words), ctypes.c_void_p), work, out, st)

    for kw, code in ((dict(dims=(0, 4, 4), words=one), "(-1)"), (dict(dims=(4, -1, 4), words=one), "(-1)"), (dict(dims=(4, 4, 0), words=one), "(-1)"),
                     (dict(dims=(2048, 1024, 1024), words=one), "(-3)"), (dict(dims=(1, 1, 2 ** 31 - 1), words=one), "(-3)"),
                     (dict(dims=(4, 4, 4), words=[3, 0, 0, 0, 0, 0, 0, 0]), "(-1)"), (dict(dims=(4, 4, 4), words=[0] * 8), "(-1)"),
                     (dict(dims=(4, 4, 4), words=one, pred=None), "(-1)"), (dict(dims=(4, 4, 4), words=one, gt=None), "(-1)"),
                     (dict(dims=(4, 4, 4), words=one, work=None), "(-1)"), (dict(dims=(4, 4, 4), words=one, out=None), "(-1)")):
        with pytest.raises(E2EError) as e:
            label(**kw)
        assert code in str(e.value), (kw, str(e.value))

    def emit(dims=(4, 4, 4), pred=x.data_ptr(), work=ws.data_ptr(), cbuf=rec.data_ptr(), ccap=3, ccount=3, fbuf=rec.data_ptr(), fcap=3, fcount=3):
        L.ct_emit(pred, *dims, work, cbuf, ccap, ccount, fbuf, fcap, fcount, st)

    for kw, code in ((dict(dims=(0, 4, 4)), "(-1)"), (dict(dims=(2048, 1024, 1024)), "(-3)"), (dict(pred=None), "(-1)"), (dict(work=None), "(-1)"),
                     (dict(ccap=2), "(-1)"), (dict(fcap=2), "(-1)"), (dict(ccount=-1), "(-1)"), (dict(ccount=65, ccap=65), "(-1)"),
                     (dict(fcount=4, fcap=4), "(-1)"), (dict(cbuf=None), "(-1)"), (dict(fbuf=None), "(-1)")):
        with pytest.raises(E2EError) as e:
            emit(**kw)
        assert code in str(e.value), (kw, str(e.value))
    assert L.ct_ws_bytes(0, 4, 4) == 0 and L.ct_ws_bytes(2048, 1024, 1024) == 0 and L.ct_ws_bytes(1, 1, 2 ** 31 - 2) == 20 * (2 ** 31 - 2) + 128
    torch.cuda.synchronize()
    assert int(x.min()) == int(x.max()) == 1 and int(ws.min()) == int(ws.max()) == 0xA5 and int(res.min()) == int(res.max()) == -7
    assert int(rec.min()) == int(rec.max()) == 0xA5
    label((4, 4, 4), one)                                     # the same buffers, accepted: one object of 64 voxels, all of them hits
    torch.cuda.synchronize()
    assert res.tolist() == [1, 1, 0, 0]
    emit(ccap=1, ccount=1, fcap=1, fcount=1, fbuf=rec[32:].data_ptr())
    torch.cuda.synchronize()
    assert rec[:20].cpu().numpy().view(np.uint32).tolist() == [0, 1, 64, 64, 0] and rec[32:40].cpu().numpy().view(np.uint32).tolist() == [0, 64]
    assert int(rec[20:32].min()) == int(rec[40:].min()) == 0xA5


def test_host_and_wrapper_refusals():
    from e2enet_medical_amd.postprocessing.component_table import component_table
    v = np.zeros((2, 3, 4), np.uint8)
    with pytest.raises(AssertionError, match="background"):
        component_table(v, v, [0, 1])
    with pytest.raises(ValueError, match="Shape mismatch"):
        component_table(v, np.zeros((2, 3, 5), np.uint8), [1])
    with pytest.raises(ValueError, match="uint8"):
        component_table(v, v, [1, 256])


# ---- the folder search, end to end on the device ---------------------------------------------------------------------------------
def _blobby_case(seed, shape=(8, 24, 28)):
    """ground truth: class 1 and class 2 touching, class 3 apart; prediction: the same plus stray voxels of every class"""
    rng = np.random.RandomState(seed)
    gt = np.zeros(shape, np.uint8)
    gt[1:6, 2:12, 2:10] = 1
    gt[1:6, 2:12, 10:16] = 2
    gt[2:7, 15:22, 20:27] = 3
    pred = gt.copy()
    stray = (rng.rand(*shape) < 0.04) & (gt == 0)
    pred[stray] = rng.randint(1, 4, int(stray.sum()))
    return pred, gt


def _in_memory(folder, cases, **kw):
    from e2enet_medical_amd.postprocessing.connected_components import determine_postprocessing
    os.makedirs(folder)
    res, final = determine_postprocessing([(p, g, n, n, s) for p, g, n, s in cases], CLASSES, folder, "validation_raw",
                                          final_subf_name="validation_final", **kw)
    return json.loads(json.dumps(res)), final, json.load(open(os.path.join(folder, "validation_final", "summary.json")))["results"]["mean"]


@pytest.mark.parametrize("advanced", [False, True])
def test_folder_search_over_npy_files_equals_the_in_memory_search(tmp_path, advanced):
    from e2enet_medical_amd.postprocessing.connected_components import determine_postprocessing
    from e2enet_medical_amd.evaluator import evaluate_folder
    base = str(tmp_path / "folder")
    raw, gts = os.path.join(base, "validation_raw"), os.path.join(base, "gt")
    os.makedirs(raw)
    os.makedirs(gts)
    cases = [_blobby_case(k) + ("case%d.npy" % k, None) for k in range(4)]
    for pred, gt, name, _ in cases:
        np.save(os.path.join(raw, name), pred)
        np.save(os.path.join(gts, name), gt)
    evaluate_folder(gts, raw, (0, 1, 2, 3), num_threads=2)
    got = determine_postprocessing(base, gts, final_subf_name="validation_final", processes=2, advanced_postprocessing=advanced)
    want, want_final, want_mean = _in_memory(str(tmp_path / "mem"), cases, advanced_postprocessing=advanced)
    assert json.load(open(os.path.join(base, "postprocessing.json"))) == want == json.loads(json.dumps(got))
    assert want['for_which_classes'] == [1, 2, 3], "the strays must make every class's own removal the choice"
    for (pred, _, name, _), w in zip(cases, want_final):
        final = np.load(os.path.join(base, "validation_final", name))
        assert final.dtype == np.uint8 and np.array_equal(final, w) and (final != pred).any()
    mean = json.load(open(os.path.join(base, "validation_final", "summary.json")))["results"]["mean"]
    assert json.dumps(mean, sort_keys=True) == json.dumps(want_mean, sort_keys=True)
    assert sorted(os.listdir(base)) == ["gt", "postprocessing.json", "validation_final", "validation_raw"]


def test_consolidate_folds_over_native_nifti_files_and_apply_to_folder(tmp_path):
    """two folds of .nii.gz files with their own spacings, read and written natively: the consolidated decision equals the in-memory
    search on the same arrays, and the stored decision applied to cv_niftis_raw reproduces cv_niftis_postprocessed byte for byte"""
    from e2enet_medical_amd import nifti
    from e2enet_medical_amd.evaluator import evaluate_folder
    from e2enet_medical_amd.postprocessing import connected_components as cc
    from e2enet_medical_amd.postprocessing.consolidate_postprocessing import main
    base = str(tmp_path / "model")
    gts = os.path.join(base, "gt_niftis")
    os.makedirs(gts)
    cases = []
    for k in range(4):
        pred, gt = _blobby_case(10 + k)
        props = {"itk_spacing": (0.75, 0.5, 1.0 + 0.5 * k), "itk_origin": (1.0, -2.0, 3.0), "itk_direction": (1., 0., 0., 0., 1., 0., 0., 0., 1.)}
        raw = os.path.join(base, "fold_%d" % (k % 2), "validation_raw")
        os.makedirs(raw, exist_ok=True)
        name = "case%d.nii.gz" % k
        nifti.write(pred, os.path.join(raw, name), props)
        nifti.write(gt, os.path.join(gts, name), props)
        cases.append((pred, gt, name, tuple(nifti.read_raw(os.path.join(raw, name)).itk_spacing)[::-1]))
    for fold in (0, 1):
        evaluate_folder(gts, os.path.join(base, "fold_%d" % fold, "validation_raw"), (0, 1, 2, 3), num_threads=2, reader=nifti.evaluator_reader)
    got = main(["-f", base, "--advanced", "--folds", "0", "1", "--native_nifti", "-tf", "2"])
    order = sorted(range(4), key=lambda k: cases[k][2])
    want, want_final, want_mean = _in_memory(str(tmp_path / "mem"), [cases[k] for k in order], advanced_postprocessing=True)
    stored = json.load(open(os.path.join(base, "postprocessing.json")))
    assert stored == dict(want, validation_raw="cv_niftis_raw", validation_final="cv_niftis_postprocessed") == json.loads(json.dumps(got))
    assert stored['for_which_classes'] == [1, 2, 3] and stored['min_valid_object_sizes'] != "None"
    final_folder = os.path.join(base, "cv_niftis_postprocessed")
    for k, w in zip(order, want_final):
        raw = nifti.read_raw(os.path.join(final_folder, cases[k][2]))
        assert np.array_equal(nifti.decode_u8(raw).cpu().numpy(), w) and (w != cases[k][0]).any()
        assert tuple(raw.itk_spacing)[::-1] == cases[k][3], "the input file's geometry"
    mean = json.load(open(os.path.join(final_folder, "summary.json")))["results"]["mean"]
    assert json.dumps(mean, sort_keys=True) == json.dumps(want_mean, sort_keys=True)
    fwc, mins = cc.load_postprocessing(os.path.join(base, "postprocessing.json"))
    applied = str(tmp_path / "applied")
    cc.apply_postprocessing_to_folder(os.path.join(base, "cv_niftis_raw"), applied, fwc, mins, 2, reader=cc.native_reader, writer=nifti.writer)
    assert sorted(os.listdir(applied)) == sorted(c[2] for c in cases)
    for c in cases:
        assert open(os.path.join(applied, c[2]), "rb").read() == open(os.path.join(final_folder, c[2]), "rb").read()
