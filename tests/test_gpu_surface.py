"""Surface-distance scoring on the device (csrc/surface.hip, evaluation/surface_distance.py) against the scipy restatement of
medpy's algorithm in tests/surface_oracle.py.  Parity is pinned to that restatement, not to a run of the reference (medpy is not
installable here); tests/test_surface_cpu.py checks the restatement against answers worked out by hand.

Bars.  Border masks, surface-voxel counts and the squared-distance map at unit spacing (integers below 2^24) are exact.  At
anisotropic spacing each of the three passes adds one fp32 rounding of a term and one of a sum: <= 4 * 2^-24 ~ 2.4e-7 relative on d^2,
the bar is 1e-6; the distance metrics inherit it (sums and means are fp64).  NSD counts distances <= threshold, so it is compared at
1e-9 at thresholds of which the test first proves, on the restatement's own distances, that none lies within 1e-4 * threshold."""
import functools
import json
import math
import os
import pickle

import numpy as np
import pytest
import torch

from tests import surface_oracle as so

pytestmark = pytest.mark.gpu

LABELS = [0, 1, 2, 3]
# (shape, spacing, NSD threshold).  Axis lengths above 252 / 496 make the strided passes stage 32 / 16 lines per workgroup instead
# of 64; every W here is wider than one tile or not a multiple of it; (1,40,72) has a length-1 axis.
CASES = [((5, 33, 65), (1., 1., 1.), 1.5),
         ((19, 37, 70), (2.5, 0.8, 0.7), 1.9),
         ((40, 48, 130), (3., 1., 1.25), 2.2),
         ((1, 40, 72), (1., 1., 1.), 1.5),
         ((300, 9, 5), (0.7, 2.5, 0.8), 1.9),
         ((5, 300, 9), (2.5, 0.8, 0.7), 1.9),
         ((5, 9, 300), (3., 1.25, 1.), 2.2),
         ((520, 6, 7), (1., 1., 1.), 1.5),
         ((6, 520, 7), (1.25, 1., 3.), 2.2)]
IDS = ["x".join(str(v) for v in c[0]) for c in CASES]


def _ellipsoid(shape, centre, radii):
    g = np.meshgrid(*[(np.arange(n) + 0.5) / n for n in shape], indexing="ij")
    return sum(((a - c) / r) ** 2 for a, c, r in zip(g, centre, radii)) <= 1.0


@functools.lru_cache(maxsize=None)
def label_maps(shape):
    """(test, reference) uint8 label maps: label 1 a large ellipsoid touching the volume face W = 0, offset and rescaled between the
    two; label 2 two distant blobs in the test and one in the reference, plus 0.2 % speckle on both sides (long distances, many
    tiny components); label 3 in the test only"""
    rng = np.random.RandomState(sum(shape))
    out = []
    for side in range(2):
        m = np.zeros(shape, np.uint8)
        m[_ellipsoid(shape, (0.5, 0.45 + 0.06 * side, 0.12), (0.42 - 0.07 * side, 0.3 + 0.05 * side, 0.34))] = 1
        m[_ellipsoid(shape, (0.3, 0.2 + 0.04 * side, 0.8), (0.25, 0.14, 0.12))] = 2
        if side == 0:
            m[_ellipsoid(shape, (0.8, 0.85, 0.9), (0.32, 0.12, 0.12))] = 2
            m[_ellipsoid(shape, (0.75, 0.2, 0.6), (0.3, 0.12, 0.12))] = 3
        m[rng.rand(*shape) < 0.002] = 2
        m.setflags(write=False)
        out.append(m)
    t, r = out
    assert all((t == l).any() and (r == l).any() for l in (0, 1, 2)) and (t == 3).any() and not (r == 3).any()
    return t, r


@functools.lru_cache(maxsize=None)
def oracle_case(i):
    shape, spacing, thr = CASES[i]
    t, r = label_maps(shape)
    return so.label_metrics(t, r, LABELS, spacing, thr)


def _scorer(i, spacing=None):
    from e2enet_medical_amd.evaluation.surface_distance import SurfaceScorer
    shape, sp, _ = CASES[i]
    t, r = label_maps(shape)
    return SurfaceScorer(t, r, sp if spacing is None else spacing), t, r


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_border_mask_equals_the_restatement(i):
    sc, t, r = _scorer(i)
    for which, vol in ((0, t), (1, r)):
        for l in LABELS + [9]:
            b, n = sc.border(which, l)
            want = so.border(vol == l)
            assert np.array_equal(b.cpu().numpy().astype(bool), want), (which, l)
            assert int(n) == int(want.sum())


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_squared_distance_map_at_unit_spacing_is_exact(i):
    sc, t, r = _scorer(i, (1., 1., 1.))
    for l in (1, 2, 9):                                        # 9: no such label, the border is empty -> +inf everywhere
        b, _ = sc.border(0, l)
        got = sc.edt_sq(0).cpu().numpy()
        want = np.rint(so.edt(b.cpu().numpy()) ** 2)
        assert want[np.isfinite(want)].max(initial=0) < 2 ** 24
        assert np.array_equal(got, want.astype(np.float32)), (l, float(np.abs(got - want).max()))
        assert l != 9 or np.isinf(got).all()


@pytest.mark.parametrize("shape", [(7, 11, 70), (1, 1, 1), (300, 2, 3)], ids=str)
def test_squared_distance_from_one_corner_voxel(shape):
    from e2enet_medical_amd.evaluation.surface_distance import SurfaceScorer
    v = np.zeros(shape, np.uint8)
    v[-1, 0, -1] = 1
    sc = SurfaceScorer(v, v, (1., 1., 1.))
    b, n = sc.border(0, 1)
    assert int(n) == 1
    z, y, x = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    want = ((z - (shape[0] - 1)) ** 2 + y ** 2 + (x - (shape[2] - 1)) ** 2).astype(np.float32)
    assert np.array_equal(sc.edt_sq(0).cpu().numpy(), want)


@pytest.mark.parametrize("i", [k for k, c in enumerate(CASES) if c[1] != (1., 1., 1.)], ids=[IDS[k] for k, c in enumerate(CASES) if c[1] != (1., 1., 1.)])
def test_squared_distance_map_at_anisotropic_spacing(i):
    sc, t, r = _scorer(i)
    worst = 0.0
    for which, l in ((0, 1), (1, 2), (0, 2)):
        b, _ = sc.border(which, l)
        got = sc.edt_sq(which).cpu().numpy().astype(np.float64)
        want = so.edt(b.cpu().numpy(), CASES[i][1]) ** 2
        assert np.array_equal(got == 0, want == 0)
        err = np.abs(got - want) / np.maximum(want, 1e-300)
        worst = max(worst, float(err[want > 0].max()))
    print("max relative error of d^2: %.3g" % worst)
    assert worst <= 1e-6, worst


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_distance_metrics_counts_and_nsd(i):
    from e2enet_medical_amd.evaluation.surface_distance import surface_distance_metrics, NSD_KEY
    shape, spacing, thr = CASES[i]
    ref = oracle_case(i)
    for l in (0, 1, 2):                  # the condition on the inputs that makes NSD comparable: no distance near the threshold
        for d in (ref[l]["d1"], ref[l]["d2"]):
            assert np.abs(d - thr).min() > 1e-4 * thr, (l, float(np.abs(d - thr).min()))
    sc, t, r = _scorer(i)
    got = surface_distance_metrics(t, r, LABELS, spacing, nsd_tolerance=thr)
    for l in (0, 1, 2):
        assert sc.stats(l, thr)["n"] == ref[l]["n"], l
        for k in so.DISTANCE_KEYS:
            print(l, k, got[l][k], ref[l][k])
            assert _rel(got[l][k], ref[l][k]) <= 1e-6 or got[l][k] == ref[l][k], (l, k, got[l][k], ref[l][k])
        assert abs(got[l][NSD_KEY] - ref[l][NSD_KEY]) <= 1e-9, (l, got[l][NSD_KEY], ref[l][NSD_KEY])
    assert all(math.isnan(v) for v in got[3].values()) and list(got[3].keys()) == list(so.DISTANCE_KEYS) + [NSD_KEY]
    from e2enet_medical_amd.evaluation.surface_distance import SurfaceScorer
    whole = SurfaceScorer(t, r, spacing, crop=False)         # label 1 lies in a proper sub-box: the route above scored the box alone
    assert sc.boxes[1] != tuple(slice(0, n) for n in shape) and whole.stats(1, thr)["n"] == ref[1]["n"]
    m = whole.metrics(1, thr)
    assert all(_rel(m[k], ref[1][k]) <= 1e-6 or m[k] == ref[1][k] for k in so.DISTANCE_KEYS) and abs(m[NSD_KEY] - ref[1][NSD_KEY]) <= 1e-9


def test_one_sided_label_is_nan_or_zero_everywhere():
    from e2enet_medical_amd.evaluation.surface_distance import surface_distance_metrics
    from e2enet_medical_amd.evaluation.evaluator import evaluate_pair, aggregate_scores
    shape, spacing, thr = CASES[1]
    t, r = label_maps(shape)
    adv = ("Hausdorff Distance 95", "Avg. Surface Distance", "Avg. Symmetric Surface Distance")
    m = surface_distance_metrics(t, r, LABELS, spacing)
    assert all(math.isnan(m[3][k]) for k in so.DISTANCE_KEYS) and all(math.isfinite(m[1][k]) for k in so.DISTANCE_KEYS)
    m0 = surface_distance_metrics(t, r, LABELS, spacing, nan_for_nonexisting=False)
    assert all(m0[3][k] == 0 for k in so.DISTANCE_KEYS) and m0[1] == m[1]
    pair = evaluate_pair(t, r, LABELS, advanced=True, voxel_spacing=spacing)
    assert all(math.isnan(pair["3"][k]) for k in adv) and all(pair["2"][k] == m[2][k] for k in adv)
    assert all(evaluate_pair(t, r, LABELS, nan_for_nonexisting=False, advanced=True, voxel_spacing=spacing)["3"][k] == 0 for k in adv)
    scores = aggregate_scores([(t, r, "a", "b", spacing), (t, r, "c", "d")], LABELS, advanced=True, voxel_spacing=spacing, nsd_tolerance=thr)
    assert all(math.isnan(scores["mean"]["3"][k]) for k in adv + ("Normalized Surface Dice",))
    assert all(scores["mean"]["1"][k] == m[1][k] for k in adv)
    assert list(scores["all"][0]["1"].keys()) == sorted(scores["all"][0]["1"].keys()) and len(scores["all"][0]["1"]) == 17


@pytest.mark.parametrize("i", [1, 4], ids=[IDS[1], IDS[4]])
def test_label_map_route_equals_materialised_masks_bit_for_bit(i):
    from e2enet_medical_amd.evaluation import surface_distance as sd
    shape, spacing, thr = CASES[i]
    t, r = label_maps(shape)
    got = sd.surface_distance_metrics(torch.from_numpy(np.array(t)).cuda(), torch.from_numpy(np.array(r)).cuda(), LABELS, spacing, nsd_tolerance=thr)
    host = sd.surface_distance_metrics(t, r, LABELS, spacing, nsd_tolerance=thr)
    for l in (0, 1, 2):
        a, b = t == l, r == l
        want = {"Hausdorff Distance": sd.hausdorff_distance(a, b, voxel_spacing=spacing),
                "Hausdorff Distance 95": sd.hausdorff_distance_95(a, b, voxel_spacing=spacing),
                "Avg. Surface Distance": sd.avg_surface_distance(a, b, voxel_spacing=spacing),
                "Avg. Symmetric Surface Distance": sd.avg_surface_distance_symmetric(a, b, voxel_spacing=spacing),
                sd.NSD_KEY: sd.normalized_surface_dice(a, b, thr, spacing)}
        for k, v in want.items():
            assert np.float64(got[l][k]).tobytes() == np.float64(v).tobytes() == np.float64(host[l][k]).tobytes(), (l, k, got[l][k], v)
    assert sd.normalized_surface_dice(t == 1, t == 1, 0.5) == 2 / (2 + 1e-8)


def test_refused_arguments_launch_nothing():
    from e2enet_medical_amd._lib import lib, E2EError
    L = lib()
    n = L.surface_max_line() + 1
    mask = torch.zeros(n, dtype=torch.uint8, device="cuda")
    dt2 = torch.full((n,), -1.0, device="cuda")
    cnt = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    for dims, sp, what in (((0, 4, 4), (1., 1., 1.), "(-1)"), ((4, 4, 4), (1., 0., 1.), "(-1)"), ((4, 4, 4), (1., 1., -2.), "(-1)"),
                           ((4, 4, 4), (float("nan"), 1., 1.), "(-1)"), ((n, 1, 1), (1., 1., 1.), "(-3)"), ((1, n, 1), (1., 1., 1.), "(-3)"),
                           ((1, 1, n), (1., 1., 1.), "(-3)")):
        with pytest.raises(E2EError) as e:
            L.distance_transform_edt_sq(mask.data_ptr(), dt2.data_ptr(), *dims, *sp, st)
        assert what in str(e.value), str(e.value)
    with pytest.raises(E2EError):
        L.surface_border(mask.data_ptr(), 1, mask.data_ptr(), cnt.data_ptr(), 4, 0, 4, st)
    with pytest.raises(E2EError):
        L.surface_border(mask.data_ptr(), 256, mask.data_ptr(), cnt.data_ptr(), 4, 4, 4, st)
    out = torch.full((10,), -1.0, dtype=torch.float64, device="cuda")
    ws = torch.zeros(L.surface_distances_ws_bytes(), dtype=torch.uint8, device="cuda")
    for nvox, lo, hi in ((0, 0, 0), (8, -1, 0), (8, 3, 2), (8, 0, 16)):
        with pytest.raises(E2EError):
            L.surface_distances_stats(mask.data_ptr(), dt2.data_ptr(), mask.data_ptr(), dt2.data_ptr(), nvox, 1.0, lo, hi, out.data_ptr(),
                                      ws.data_ptr(), st)
    torch.cuda.synchronize()
    assert float(dt2.min()) == float(dt2.max()) == -1.0 and int(cnt) == -7 and float(out.max()) == -1.0 and int(ws.max()) == 0


def test_two_rank_select_on_hand_made_values():
    """e2e_surface_distances_stats on 600 voxels, both borders all ones, so the select sees all 1200 squared distances: ties of 300,
    400 and 54 values, 256 + 64 values that differ in the lowest byte of their bit pattern alone (with one carry into the third
    byte) and one value per top byte 0x01 .. 0x7e.  The order statistics are np.sqrt(np.sort(.).astype(float64))[rank], exactly.
    Counts, maxima and the counts within the threshold are exact too; a sum of m non-negative fp64 terms is within (m - 1) 2^-53
    of the true sum in any order, so the device's and numpy's differ by at most 2 * 599 * 2^-53 relative."""
    from e2enet_medical_amd._lib import lib
    L = lib()
    n, thr = 600, 1.75
    words = np.concatenate([np.zeros(300, np.uint32), np.full(400, 0x3FC00000, np.uint32),
                            0x40490F00 + np.arange(256, dtype=np.uint32), 0x40491000 + np.arange(64, dtype=np.uint32),
                            (np.arange(1, 0x7F, dtype=np.uint32) << 24) | 0x123456, np.full(54, 0x7149F2CA, np.uint32)]).astype(np.uint32)
    assert words.size == 2 * n
    d2 = np.random.RandomState(7).permutation(words).view(np.float32).reshape(2, n)     # [0]: dt2_b (direction 0), [1]: dt2_a
    want = np.sqrt(np.sort(d2.reshape(-1)).astype(np.float64))
    bits = np.sort(d2.reshape(-1)).view(np.uint32)
    at = lambda w: int(np.flatnonzero(bits == w)[0])
    low, carry, tie = at(0x40490F0A), at(0x40490FFF), at(0x3FC00000) + 100
    assert 0 < (bits[low] ^ bits[low + 1]) < 256 and bits[carry + 1] == 0x40491000 and bits[tie] == bits[tie + 1] == 0x3FC00000
    dev = torch.from_numpy(d2).cuda()
    ones = torch.ones(n, dtype=torch.uint8, device="cuda")
    out = torch.empty(10, dtype=torch.float64, device="cuda")
    ws = torch.empty(L.surface_distances_ws_bytes(), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    d = np.sqrt(d2.astype(np.float64))
    assert np.abs(d - thr).min() > 1e-3
    for lo, hi in ((low, low), (800, 800), (low, low + 1), (carry, carry + 1), (0, 2 * n - 1), (tie, tie + 1), (299, 300)):
        L.surface_distances_stats(ones.data_ptr(), dev[0].data_ptr(), ones.data_ptr(), dev[1].data_ptr(), n, thr, lo, hi, out.data_ptr(),
                                  ws.data_ptr(), st)
        o = out.cpu().numpy()
        print(lo, hi, o.tolist())
        assert o[8] == want[lo] and o[9] == want[hi], (lo, hi, o[8], want[lo], o[9], want[hi])
        for dir in range(2):
            assert o[4 * dir] == n and o[4 * dir + 2] == d[dir].max() and o[4 * dir + 3] == (d[dir] <= thr).sum(), (dir, o.tolist())
            assert _rel(o[4 * dir + 1], d[dir].sum()) <= 2 * (n - 1) * 2.0 ** -53, (dir, o[4 * dir + 1], d[dir].sum())


def test_validate_scores_the_advanced_metrics(tmp_path):
    """validate(advanced_metrics=True) writes the three default_advanced_metrics (and NSD with a tolerance) into every label's dict
    of summary.json, scored under properties['itk_spacing'][::-1]; the values are the restatement's on the exported volumes.  Without
    the keyword the file has the thirteen keys it had before."""
    from tests.helpers import write_synthetic_task
    from tests.test_gpu_trainer import PLANS
    from e2enet_medical_amd.evaluation.evaluator import DEFAULT_METRICS
    from e2enet_medical_amd.training.network_training.nnUNetTrainer_simple import nnUNetTrainer_simple
    ddir, plans = write_synthetic_task(str(tmp_path / "pre"), plans=dict(PLANS, transpose_forward=[0, 1, 2], transpose_backward=[0, 1, 2]))
    folder = os.path.join(ddir, plans['data_identifier'] + "_stage0")
    for f in sorted(os.listdir(folder)):
        if f.endswith(".pkl"):
            props = pickle.load(open(os.path.join(folder, f), "rb"))
            props["itk_spacing"] = (0.7, 0.8, 2.5)                       # (x, y, z): the volumes are scored at (2.5, 0.8, 0.7)
            pickle.dump(props, open(os.path.join(folder, f), "wb"))
    tr = nnUNetTrainer_simple(plans, 0, output_folder=str(tmp_path / "out"), dataset_directory=ddir, batch_dice=False,
                              Tconv='shiftConvPP', max_num_epochs=1, num_batches_per_epoch=2)
    tr.base_num_features_override = 8
    torch.manual_seed(0)
    np.random.seed(0)
    tr.initialize(True)
    written = {}
    kw = dict(do_mirroring=False, save_softmax=False, writer=lambda seg, path, props: written.__setitem__(path, seg.copy()))
    tr.validate(validation_folder_name="plain", **kw)
    js = json.load(open(os.path.join(tr.output_folder, "plain", "summary.json")))
    for rec in js["results"]["all"]:
        assert set(rec.keys()) == {"0", "1", "2", "test", "reference"}
        assert all(sorted(rec[l].keys()) == sorted(DEFAULT_METRICS) for l in "012")
    thr = 1.9
    scores = tr.validate(validation_folder_name="advanced", advanced_metrics=True, nsd_tolerance=thr, **kw)
    out = os.path.join(tr.output_folder, "advanced")
    js = json.load(open(os.path.join(out, "summary.json")))
    adv = ["Hausdorff Distance 95", "Avg. Surface Distance", "Avg. Symmetric Surface Distance"]
    finite = 0
    for k, rec in zip(tr.dataset_val.keys(), js["results"]["all"]):
        assert rec["voxel_spacing"] == [2.5, 0.8, 0.7]
        seg = written[os.path.join(out, k + ".nii.gz")]
        gt = np.load(os.path.join(ddir, "gt_segmentations", k + ".npy"))
        ref = so.label_metrics(seg, gt, [0, 1, 2], (2.5, 0.8, 0.7), thr)
        for l in (0, 1, 2):
            assert sorted(rec[str(l)].keys()) == sorted(DEFAULT_METRICS + adv + ["Normalized Surface Dice"])
            for name in adv:
                got, want = rec[str(l)][name], ref[l][name]
                print(k, l, name, got, want)
                assert (math.isnan(got) and math.isnan(want)) or _rel(got, want) <= 1e-6 or got == want, (k, l, name, got, want)
                finite += math.isfinite(got)
            if ref[l]["d1"] is not None and min(np.abs(d - thr).min() for d in (ref[l]["d1"], ref[l]["d2"])) > 1e-4 * thr:
                assert abs(rec[str(l)]["Normalized Surface Dice"] - ref[l]["Normalized Surface Dice"]) <= 1e-9
    assert finite > 0, "the prediction of this fixture left no label that both volumes hold"
    assert set(scores["mean"]["1"].keys()) == set(DEFAULT_METRICS + adv + ["Normalized Surface Dice"])
