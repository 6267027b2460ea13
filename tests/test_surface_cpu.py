"""Surface-distance metrics without a device: the scipy restatement of medpy's algorithm (tests/surface_oracle.py), which is the
yardstick of tests/test_gpu_surface.py, gives the answers one can work out by hand; and the parts of the package that are decided
from voxel counts alone (key sets, the empty / full rule, refused arguments) behave as the reference's evaluator does.

Parity is pinned to medpy's documented algorithm as restated, not to a run of the reference: medpy is not installable here."""
import math

import numpy as np
import pytest

from tests import surface_oracle as so

ADVANCED = ["Avg. Surface Distance", "Avg. Symmetric Surface Distance", "Hausdorff Distance 95"]


@pytest.mark.parametrize("delta,spacing", [((3, 0, 0), (1., 1., 1.)), ((2, 3, 4), (2.5, 0.8, 0.7)), ((0, 5, 1), (3., 1., 1.25))])
def test_two_single_voxels_are_their_euclidean_distance_apart(delta, spacing):
    a, b = np.zeros((8, 9, 10), bool), np.zeros((8, 9, 10), bool)
    a[1, 2, 3] = True
    b[1 + delta[0], 2 + delta[1], 3 + delta[2]] = True
    want = math.sqrt(sum((d * s) ** 2 for d, s in zip(delta, spacing)))
    m = so.metrics(a, b, spacing)
    for k in so.DISTANCE_KEYS:
        assert abs(m[k] - want) < 1e-12, (k, m[k], want)
    assert m["n"] == (1, 1)


def test_shifted_cube_by_hand():
    """A = the 6^3 cube [2,8)^3, B = A shifted by 2 along axis 0, unit spacing.  A's border is its shell, 216 - 64 = 152 voxels.
    From A's shell to B's shell: the face x = 2 (36 voxels) lies 2 from B's face x = 4; the ring of the layer x = 3 (20 voxels, y or z
    on the cube's edge) lies 1 from B's ring at x = 4; the rings of x = 4, 5, 6 (60 voxels) and the ring of the face x = 7 (20) are
    voxels of B's shell: 0; the 4 x 4 inside of the face x = 7 lies inside B, whose shell is 2 away along x (x = 9) and 1 or 2 away
    along y and z: its 2 x 2 centre gets 2, the other 12 voxels 1.  Sum = 36 * 2 + 20 * 1 + 4 * 2 + 12 * 1 = 112 over 152 voxels, and
    B -> A is the mirror image: ASD = ASSD = 112 / 152, HD = 2, and with 80 of the 304 distances equal to 2, HD95 = 2."""
    a, b = np.zeros((14, 10, 10), bool), np.zeros((14, 10, 10), bool)
    a[2:8, 2:8, 2:8] = True
    b[4:10, 2:8, 2:8] = True
    for axis in range(3):
        m = so.metrics(np.moveaxis(a, 0, axis), np.moveaxis(b, 0, axis))
        assert m["n"] == (152, 152)
        assert m["Hausdorff Distance"] == 2.0 and m["Hausdorff Distance 95"] == 2.0
        assert abs(m["Avg. Surface Distance"] - 112 / 152) < 1e-12
        assert abs(m["Avg. Symmetric Surface Distance"] - 112 / 152) < 1e-12
        assert sorted(set(m["d1"].tolist())) == [0.0, 1.0, 2.0] and int((m["d1"] == 2).sum()) == 40


def test_identical_masks():
    rng = np.random.RandomState(0)
    a = rng.rand(7, 8, 9) > 0.6
    m = so.metrics(a, a, (2.5, 0.8, 0.7), threshold=0.0)
    assert all(m[k] == 0.0 for k in so.DISTANCE_KEYS)
    assert m["Normalized Surface Dice"] == 2 / (2 + 1e-8)


def test_a_mask_on_the_volume_face_has_its_border_there():
    a = np.zeros((6, 7, 8), bool)
    a[0:4, 2:6, 3:8] = True                      # touches the faces axis0 = 0 and axis2 = 7
    b = so.border(a)
    assert b[0, 2:6, 3:8].all() and b[0:4, 2:6, 7].all()
    assert not b[1:3, 3:5, 4:7].any() and int(b.sum()) == int(a.sum()) - 2 * 2 * 3
    full = np.ones((3, 4, 5), bool)              # a full volume: everything on a face is border, the inside is not
    assert int(so.border(full).sum()) == 60 - 1 * 2 * 3
    assert np.isinf(so.edt(np.zeros((3, 4, 5), bool))).all()


def _maps(seed, shape=(6, 7, 8), k=4):
    rng = np.random.RandomState(seed)
    return rng.randint(0, k, shape).astype(np.uint8), rng.randint(0, k, shape).astype(np.uint8)


def test_default_arguments_give_the_thirteen_keys_of_today():
    from e2enet_medical_amd.evaluation.evaluator import aggregate_scores, evaluate_pair, DEFAULT_METRICS
    t, r = _maps(1)
    scores = aggregate_scores([(t, r, "a", "b"), (r, t, None, None)], labels=[0, 1, 2, 3])
    for rec in scores["all"]:
        assert "voxel_spacing" not in rec
        for l in "0123":
            assert list(rec[l].keys()) == sorted(DEFAULT_METRICS)
    assert set(scores["all"][0].keys()) == {"0", "1", "2", "3", "test", "reference"}
    assert list(scores["mean"]["2"].keys()) == sorted(DEFAULT_METRICS)
    assert evaluate_pair(t, r, [1]) == evaluate_pair(t, r, [1], advanced=False, voxel_spacing=(3, 2, 1), nsd_tolerance=1.0)


@pytest.mark.parametrize("nsd", [None, 1.5])
def test_advanced_keys_join_sorted_and_enter_the_mean(monkeypatch, nsd):
    """key parity with a real value behind every key: the device scorer is replaced by the restatement here (the device is
    compared against it in test_gpu_surface.py), everything around it is the package's own code"""
    from e2enet_medical_amd.evaluation import evaluator, surface_distance as sd
    from e2enet_medical_amd.evaluation.evaluator import DEFAULT_METRICS

    class HostScorer:
        def __init__(self, test, reference, spacing):
            self.t, self.r, self.s = np.asarray(test), np.asarray(reference), spacing

        def metrics(self, label, tol):
            return so.metrics(self.t == label, self.r == label, self.s, tol)
    monkeypatch.setattr(sd, "SurfaceScorer", HostScorer)
    t, r = _maps(2)
    u, v = _maps(3)
    names = sorted(DEFAULT_METRICS + ADVANCED + (["Normalized Surface Dice"] if nsd is not None else []))
    scores = evaluator.aggregate_scores([(t, r, "a", "b", (2.5, 0.8, 0.7)), (u, v, "c", "d")], labels=[0, 1, 2, 3], advanced=True,
                                        voxel_spacing=(1, 1, 2), nsd_tolerance=nsd)
    assert scores["all"][0]["voxel_spacing"] == [2.5, 0.8, 0.7] and scores["all"][1]["voxel_spacing"] == [1.0, 1.0, 2.0]
    for l in "0123":
        assert list(scores["all"][0][l].keys()) == names and list(scores["mean"][l].keys()) == names
    assert "voxel_spacing" not in scores["mean"]
    want = [so.metrics(t == 2, r == 2, (2.5, 0.8, 0.7)), so.metrics(u == 2, v == 2, (1, 1, 2))]
    for k in ADVANCED:
        assert scores["all"][0]["2"][k] == want[0][k]
        assert abs(scores["mean"]["2"][k] - (want[0][k] + want[1][k]) / 2) < 1e-12
    assert "Hausdorff Distance" not in scores["all"][0]["2"]          # (default_advanced_metrics lists HD95, not HD)


def test_empty_and_full_masks_are_decided_from_counts_without_a_device():
    from e2enet_medical_amd.evaluation.evaluator import aggregate_scores, evaluate_pair
    from e2enet_medical_amd.evaluation.surface_distance import surface_distance_metrics, hausdorff_distance_95
    t = np.zeros((4, 5, 6), np.uint8)            # test: all 0 (label 0 full, 1 and 2 empty); reference: 0 and 1 present, 2 empty
    r = np.zeros((4, 5, 6), np.uint8)
    r[1:3, 1:3, 1:3] = 1
    res = surface_distance_metrics(t, r, [0, 1, 2], (1., 1., 1.), nsd_tolerance=1.0)
    assert list(res[1].keys()) == list(so.DISTANCE_KEYS) + ["Normalized Surface Dice"]
    assert all(math.isnan(v) for l in (0, 1, 2) for v in res[l].values())
    res0 = surface_distance_metrics(t, r, [0, 1, 2], (1., 1., 1.), nan_for_nonexisting=False)
    assert all(v == 0 for l in (0, 1, 2) for v in res0[l].values())
    for l in (0, 1, 2):                          # the restatement applies the same rule
        assert all(math.isnan(so.metrics(t == l, r == l)[k]) for k in so.DISTANCE_KEYS)
    pair = evaluate_pair(t, r, [0, 1, 2], advanced=True)
    assert all(math.isnan(pair[l][k]) for l in "012" for k in ADVANCED)
    pair0 = evaluate_pair(t, r, [0, 1, 2], nan_for_nonexisting=False, advanced=True)
    assert all(pair0[l][k] == 0 for l in "012" for k in ADVANCED)
    scores = aggregate_scores([(t, r, "a", "b")], labels=[0, 1, 2], advanced=True, voxel_spacing=(3, 1, 1))
    assert all(math.isnan(scores["mean"][l][k]) for l in "012" for k in ADVANCED)
    assert math.isnan(hausdorff_distance_95(t == 1, r == 1)) and hausdorff_distance_95(t == 1, r == 1, nan_for_nonexisting=False) == 0


def test_refused_arguments():
    from e2enet_medical_amd.evaluation import surface_distance as sd
    a = np.ones((3, 3, 3), bool)
    for fn in (sd.hausdorff_distance, sd.hausdorff_distance_95, sd.avg_surface_distance, sd.avg_surface_distance_symmetric):
        with pytest.raises(NotImplementedError):
            fn(a, a, connectivity=2)
    with pytest.raises(NotImplementedError):
        sd.normalized_surface_dice(a, a, 1.0, connectivity=2)
    with pytest.raises(ValueError):
        sd.surface_distance_metrics(a, a, [1], (1., 0., 1.))
    with pytest.raises(ValueError):
        sd.surface_distance_metrics(a, a[:2], [1], (1., 1., 1.))
    with pytest.raises(ValueError):
        sd.surface_distance_metrics(a[0], a[0], [1], (1., 1., 1.))
    with pytest.raises(ValueError):
        sd.surface_distance_metrics(a, a, [256], (1., 1., 1.))
