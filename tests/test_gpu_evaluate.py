"""Folder evaluation on the device: the label census (csrc/evaluate.hip), the border of a label set (csrc/surface.hip), and
``evaluate_pair_device`` / ``evaluate_folder`` / the command line built on them.

Yardsticks.  The census is integers: the joint table must equal numpy's joint ``bincount`` and the boxes scipy's ``find_objects``
(``label_boxes``) exactly.  ``evaluate_pair_device`` on integer labels runs the kernels ``evaluate_pair`` runs, on the same boxes, so
every number is compared bit for bit.  Regions have no earlier device path: they are compared with tests/surface_oracle.py on the
``np.isin`` masks at the bars of tests/test_gpu_surface.py (its docstring derives them): 1e-6 relative on distances, 1e-9 on NSD at
thresholds no oracle distance comes within 1e-4 of."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import surface_oracle as so
from tests.test_gpu_surface import label_maps, CASES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _device_copy(x, misalign):
    """a contiguous device copy of the flat volume whose data pointer is ``misalign`` bytes past a 16-byte boundary"""
    buf = torch.empty(x.size + 32, dtype=torch.uint8, device="cuda")
    start = (-buf.data_ptr()) % 16 + misalign
    view = buf[start:start + x.size]
    view.copy_(torch.from_numpy(np.array(x, order="C").reshape(-1)))
    assert view.data_ptr() % 16 == misalign % 16
    return view


def census(t, r, lut, slots, misalign=(0, 0)):
    import ctypes
    from e2enet_medical_amd._lib import lib
    D, H, W = t.shape
    dt, dr = _device_copy(t, misalign[0]), _device_copy(r, misalign[1])
    joint = torch.full((slots * slots,), -5, dtype=torch.int64, device="cuda")          # (the call initialises its outputs itself)
    boxes = torch.full((slots * 6,), -5, dtype=torch.int32, device="cuda")
    lib().eval_census(dt.data_ptr(), dr.data_ptr(), (ctypes.c_ubyte * 256)(*[int(v) for v in lut]), slots, D, H, W, joint.data_ptr(),
                      boxes.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return joint.cpu().numpy().reshape(slots, slots), boxes.cpu().numpy().reshape(slots, 6)


def check_census(t, r, lut, slots, misalign=(0, 0)):
    from e2enet_medical_amd.evaluation.surface_distance import label_boxes
    lut = np.asarray(lut)
    joint, boxes = census(t, r, lut, slots, misalign)
    st, sr = lut[t].astype(np.uint8), lut[r].astype(np.uint8)
    want = np.bincount(sr.reshape(-1).astype(np.int64) * slots + st.reshape(-1), minlength=slots * slots).reshape(slots, slots)
    assert np.array_equal(joint, want), np.argwhere(joint != want)[:5]
    want_boxes = label_boxes(st, sr)
    for s in range(slots):
        if s in want_boxes:
            got = tuple(slice(int(boxes[s, a]), int(boxes[s, 3 + a])) for a in range(3))
            assert got == want_boxes[s], (s, got, want_boxes[s])
        else:
            assert all(boxes[s, a] >= boxes[s, 3 + a] for a in range(3)), (s, boxes[s])
    return joint, boxes


def _identity_lut(k):
    """values 0..k-2 -> their own slot, every other value -> slot k-1"""
    return [min(v, k - 1) for v in range(256)]


def _blocks(shape, seed, values):
    """a piecewise-constant volume: boxes of random size and value painted over each other, plus 0.1 % speckle"""
    rng = np.random.RandomState(seed)
    m = np.zeros(shape, np.uint8)
    for _ in range(24):
        lo = [rng.randint(0, n) for n in shape]
        hi = [min(n, l + 1 + rng.randint(0, max(1, n // 2))) for l, n in zip(lo, shape)]
        m[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = values[rng.randint(len(values))]
    speck = rng.rand(*shape) < 0.001
    m[speck] = np.asarray(values, np.uint8)[rng.randint(len(values), size=int(speck.sum()))]
    return m


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 17), (3, 5, 7), (4, 9, 33), (19, 37, 70)], ids=str)
def test_census_small_shapes_random_and_piecewise(shape):
    rng = np.random.RandomState(sum(shape))
    for slots in (1, 5, 64):
        lut = _identity_lut(slots)
        hi = 256 if slots < 64 else 80                          # values past the lut's own slots land in the last one
        t, r = rng.randint(0, hi, shape).astype(np.uint8), rng.randint(0, hi, shape).astype(np.uint8)       # lanes diverge
        check_census(t, r, lut, slots)
    vals = [0, 1, 2, 7, 255]
    lut = [{0: 0, 1: 1, 2: 2, 255: 3}.get(v, 4) for v in range(256)]                    # 255 has a slot, 7 is "other"
    t, r = _blocks(shape, 1, vals), _blocks(shape, 2, vals)
    check_census(t, r, lut, 5)
    check_census(t, r, lut, 6)                                  # slot 5: nobody carries it


@pytest.mark.parametrize("misalign", [(1, 1), (13, 13), (15, 15), (3, 8), (0, 5)], ids=str)
def test_census_misaligned_start(misalign):
    """both volumes start off a 16-byte boundary (head and tail spans), and on different phases (byte loads throughout)"""
    for shape in ((4, 9, 33), (1, 1, 17), (1, 1, 5), (19, 37, 70)):
        t, r = label_maps((19, 37, 70)) if shape == (19, 37, 70) else (_blocks(shape, 3, [0, 1, 2, 3]), _blocks(shape, 4, [0, 1, 2, 3]))
        check_census(t, r, _identity_lut(5), 5, misalign)


@pytest.mark.parametrize("i", [0, 1, 2, 3], ids=[str(CASES[i][0]) for i in range(4)])
def test_census_label_maps(i):
    """the piecewise-constant maps the surface tests use; label 3 is in the test only.  Two calls give identical tables."""
    t, r = label_maps(CASES[i][0])
    joint, boxes = check_census(t, r, _identity_lut(5), 5)
    assert joint[:, 3].sum() > 0 and joint[3, :].sum() == 0 and joint[4].sum() == 0 and joint[:, 4].sum() == 0
    again = census(t, r, _identity_lut(5), 5)
    assert np.array_equal(again[0], joint) and np.array_equal(again[1], boxes)
    one = np.full(CASES[i][0], 2, np.uint8)                     # a one-value volume
    j, b = check_census(one, one, _identity_lut(5), 5)
    assert j[2, 2] == one.size and j.sum() == one.size and tuple(b[2]) == (0, 0, 0) + CASES[i][0]


@pytest.mark.parametrize("above", [False, True], ids=["below", "above"])
def test_census_around_one_grid_of_chunks(above):
    """just below chunk x workgroups voxels every workgroup makes one trip and the last chunk is partial; just above, the grid
    stride takes a second trip that ends in a partial chunk"""
    from e2enet_medical_amd._lib import lib
    L = lib()
    assert L.eval_census_max_slots() == 64
    full = L.eval_census_chunk() * L.eval_census_workgroups()
    H, W = 257, 251
    D = full // (H * W) + (1 if above else 0)
    n = D * H * W
    assert (n > full) == above and abs(n - full) < H * W and n % L.eval_census_chunk() != 0
    vals = [0, 1, 2, 3, 9]
    t, r = _blocks((D, H, W), 5, vals), _blocks((D, H, W), 6, vals)
    t[-1, -1, -3:] = 3                                           # something to count at the very end of the last chunk
    check_census(t, r, _identity_lut(5), 5)


def test_census_refuses_bad_arguments():
    from e2enet_medical_amd._lib import E2EError
    t = np.zeros((2, 3, 4), np.uint8)
    for lut, slots in ((_identity_lut(5), 0), (_identity_lut(5), 65), (_identity_lut(5), 4)):
        with pytest.raises(E2EError):
            census(t, t, lut, slots)


MEMBER_SETS = [(2,), (1, 2, 3), (0,), (255,), ()]


@pytest.mark.parametrize("shape", [(5, 33, 65), (1, 40, 72), (19, 37, 70)], ids=str)
def test_border_of_a_label_set(shape):
    from e2enet_medical_amd._lib import lib
    from e2enet_medical_amd.evaluation.surface_distance import member_words
    L = lib()
    t, r = label_maps(shape)
    vol = np.array(t)
    vol[np.asarray(r) == 2] = 255
    assert all((vol == v).any() for v in (0, 1, 2, 3, 255))
    D, H, W = shape
    dv = torch.from_numpy(vol).cuda()
    st = torch.cuda.current_stream().cuda_stream
    for members in MEMBER_SETS:
        out = torch.full(shape, 7, dtype=torch.uint8, device="cuda")
        cnt = torch.full((1,), -3, dtype=torch.int64, device="cuda")
        L.surface_border_set(dv.data_ptr(), member_words(members), out.data_ptr(), cnt.data_ptr(), D, H, W, st)
        want = so.border(np.isin(vol, members))
        assert np.array_equal(out.cpu().numpy(), want.astype(np.uint8)), members
        assert int(cnt) == int(want.sum()), members
        if len(members) == 1:
            one = torch.full(shape, 9, dtype=torch.uint8, device="cuda")
            cnt1 = torch.full((1,), -3, dtype=torch.int64, device="cuda")
            L.surface_border(dv.data_ptr(), members[0], one.data_ptr(), cnt1.data_ptr(), D, H, W, st)
            assert torch.equal(one, out) and int(cnt1) == int(cnt)


def _same(a, b):
    return (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b)) or a == b


def _same_tree(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a.keys()) == list(b.keys()) and all(_same_tree(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same_tree(x, y) for x, y in zip(a, b))
    return _same(a, b)


@pytest.mark.parametrize("i", [0, 1, 2], ids=[str(CASES[i][0]) for i in range(3)])
def test_evaluate_pair_device_equals_evaluate_pair_on_integer_labels(i):
    from e2enet_medical_amd.evaluation.evaluator import evaluate_pair, evaluate_pair_device
    shape, spacing, thr = CASES[i]
    t, r = label_maps(shape)
    labels = [0, 1, 2, 3]
    want = evaluate_pair(t, r, labels, advanced=True, voxel_spacing=spacing, nsd_tolerance=thr)
    got = evaluate_pair_device(t, r, labels, advanced=True, voxel_spacing=spacing, nsd_tolerance=thr)
    assert len(got["1"]) == 17 and math.isnan(got["3"]["Hausdorff Distance 95"]) and math.isfinite(got["2"]["Hausdorff Distance 95"])
    assert _same_tree(got, want), (got, want)
    for kw in (dict(), dict(nan_for_nonexisting=False), dict(advanced=True, nan_for_nonexisting=False, voxel_spacing=spacing)):
        assert _same_tree(evaluate_pair_device(t, r, labels, **kw), evaluate_pair(t, r, labels, **kw)), kw
    # the other label forms give the same numbers; None reads the values present from the device pass
    assert _same_tree(evaluate_pair_device(torch.from_numpy(np.array(t)).cuda(), torch.from_numpy(np.array(r)).cuda(), np.array(labels)),
                      evaluate_pair(t, r, labels))
    assert _same_tree(evaluate_pair_device(t, r, None), evaluate_pair(t, r, labels))
    t2 = np.array(t)
    t2[0, 0, :3] = 200                                           # a value past the 63 slots of the first pass
    assert _same_tree(evaluate_pair_device(t2, r, None, advanced=True, voxel_spacing=spacing),
                      evaluate_pair(t2, r, [0, 1, 2, 3, 200], advanced=True, voxel_spacing=spacing))
    named = evaluate_pair_device(t, r, {1: "one", 2: 2}, advanced=True, voxel_spacing=spacing, nsd_tolerance=thr)
    assert list(named.keys()) == ["one", "2"] and _same_tree(named["one"], want["1"]) and _same_tree(named["2"], want["2"])


REGIONS = {(1, 2, 3): "a", (2, 3): "b", (1, 2): "c", (3,): "d"}


@pytest.mark.parametrize("i", [0, 1, 2, 3], ids=[str(CASES[i][0]) for i in range(4)])
def test_evaluate_pair_device_on_regions(i):
    from e2enet_medical_amd.evaluation.evaluator import evaluate_pair_device, metrics_from_counts, DEFAULT_METRICS
    from e2enet_medical_amd.evaluation.surface_distance import ADVANCED_METRICS, NSD_KEY
    shape, spacing, thr = CASES[i]
    t, r = label_maps(shape)
    got = evaluate_pair_device(t, r, REGIONS, advanced=True, voxel_spacing=spacing, nsd_tolerance=thr)
    assert list(got.keys()) == ["a", "b", "c", "d"]
    for members, name in REGIONS.items():
        a, b = np.isin(t, members), np.isin(r, members)
        ref = so.metrics(a, b, spacing, thr)
        counts = (int((a & b).sum()), int((a & ~b).sum()), int((~a & ~b).sum()), int((~a & b).sum()))
        host = metrics_from_counts(*counts)
        assert sorted(got[name].keys()) == sorted(DEFAULT_METRICS + list(ADVANCED_METRICS) + [NSD_KEY])
        for k in DEFAULT_METRICS:                               # counts and Dice: exact
            assert _same(got[name][k], host[k]), (name, k, got[name][k], host[k])
        if name == "d":                                         # (3,) is empty in the reference map: the NaN rule
            assert ref["d1"] is None and all(math.isnan(got[name][k]) for k in ADVANCED_METRICS + (NSD_KEY,))
            continue
        for d in (ref["d1"], ref["d2"]):                        # no oracle distance near the threshold: NSD is comparable
            assert np.abs(d - thr).min() > 1e-4 * thr, (name, float(np.abs(d - thr).min()))
        for k in ADVANCED_METRICS:
            print(name, k, got[name][k], ref[k])
            assert abs(got[name][k] - ref[k]) <= 1e-6 * abs(ref[k]) or got[name][k] == ref[k], (name, k, got[name][k], ref[k])
        assert abs(got[name][NSD_KEY] - ref[NSD_KEY]) <= 1e-9, (name, got[name][NSD_KEY], ref[NSD_KEY])
    off = evaluate_pair_device(t, r, REGIONS, nan_for_nonexisting=False, advanced=True, voxel_spacing=spacing)
    assert all(off["d"][k] == 0 for k in ADVANCED_METRICS) and _same(off["a"]["Dice"], got["a"]["Dice"])


LABELS = (0, 1, 2, 3)
SUMMARY_KEYS = ["author", "description", "id", "name", "results", "task", "timestamp"]       # the reference's (evaluator.py:390-398)


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    """three .npy pairs: one prediction named with _0000, one pair without label 1"""
    root = tmp_path_factory.mktemp("evalfolder")
    gt, pred = root / "gt", root / "pred"
    gt.mkdir()
    pred.mkdir()
    cases = []
    for stem, pred_name, shape, drop in (("a", "a.npy", (5, 33, 65), None), ("b", "b_0000.npy", (19, 37, 70), None), ("c", "c.npy", (1, 40, 72), 1)):
        t, r = (np.array(m) for m in label_maps(shape))
        if drop is not None:
            t[t == drop] = 0
            r[r == drop] = 0
        np.save(pred / pred_name, t)
        np.save(gt / (stem + ".npy"), r)
        cases.append((t, r, str(pred / pred_name), str(gt / (stem + ".npy"))))
    return str(gt), str(pred), cases


def _as_json(scores):
    """what json.load gives back for a file written with sorted keys"""
    return json.loads(json.dumps(scores, sort_keys=True))


def _stable_lines(path):
    return [l for l in open(path).read().splitlines() if '"timestamp":' not in l and '"id":' not in l]


def test_evaluate_folder_writes_the_reference_summary(folders, tmp_path):
    from e2enet_medical_amd.evaluator import evaluate_folder, aggregate_scores, pair_files
    from e2enet_medical_amd.evaluation import evaluator as host
    gt, pred, cases = folders
    scores = evaluate_folder(gt, pred, LABELS)
    js = json.load(open(os.path.join(pred, "summary.json")))
    assert sorted(js.keys()) == SUMMARY_KEYS and js["author"] == "Fabian" and len(js["id"]) == 12
    want = host.aggregate_scores(cases, LABELS)
    assert _same_tree(scores, want)
    assert _same_tree(js["results"], _as_json(want))
    assert [os.path.basename(c["reference"]) for c in js["results"]["all"]] == ["a.npy", "b.npy", "c.npy"]
    assert math.isnan(js["results"]["all"][2]["1"]["Dice"]) and math.isfinite(js["results"]["mean"]["1"]["Dice"])
    files = []
    for n in (1, 4):
        files.append(str(tmp_path / ("summary%d.json" % n)))
        aggregate_scores(pair_files(gt, pred), labels=LABELS, json_output_file=files[-1], num_threads=n, advanced=True, nsd_tolerance=1.5)
    assert _stable_lines(files[0]) == _stable_lines(files[1]) and len(_stable_lines(files[0])) > 100
    adv = json.load(open(files[0]))["results"]
    want = host.aggregate_scores(cases, LABELS, advanced=True, nsd_tolerance=1.5)
    assert _same_tree(adv, _as_json(want))


def test_command_line_writes_the_same_results(folders, tmp_path):
    from e2enet_medical_amd.evaluation import evaluator as host
    gt, pred, cases = folders
    out = os.path.join(pred, "summary.json")
    if os.path.exists(out):
        os.remove(out)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    done = subprocess.run([sys.executable, "-m", "e2enet_medical_amd.evaluator", "-ref", gt, "-pred", pred, "-l"] + [str(l) for l in LABELS] +
                          ["-tf", "2"], cwd=ROOT, env=env, timeout=300, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    js = json.load(open(out))
    assert sorted(js.keys()) == SUMMARY_KEYS
    assert _same_tree(js["results"], _as_json(host.aggregate_scores(cases, LABELS)))
