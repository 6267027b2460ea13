"""The yardstick of the surface-distance metrics: medpy's documented algorithm (binary border by one erosion with the 6-neighbour
cross, exact Euclidean distance transform of the other border under the voxel spacing) restated with scipy / numpy in float64.

medpy is not installable where this suite runs, so parity is pinned to this restatement of its algorithm as called by the
reference (e2enet/evaluation/metrics.py:792-861, surface_dice.py:20-56; connectivity 1), not to a run of the reference.  All
arrays are 3-D, ``spacing`` is three positive numbers in array-axis order."""
import numpy as np
from scipy.ndimage import binary_erosion, distance_transform_edt, generate_binary_structure

DISTANCE_KEYS = ("Hausdorff Distance", "Hausdorff Distance 95", "Avg. Surface Distance", "Avg. Symmetric Surface Distance")


def border(m):
    """m & ~erode(m): 6-neighbour cross, one iteration, voxels outside the volume are 0"""
    m = np.asarray(m).astype(bool)
    return m ^ binary_erosion(m, generate_binary_structure(3, 1), iterations=1)


def edt(mask, spacing=(1., 1., 1.)):
    """distance of every voxel to the nearest set voxel of ``mask`` (float64); +inf everywhere for an empty mask (scipy itself
    returns a distance to a voxel outside the volume there)"""
    mask = np.asarray(mask).astype(bool)
    if not mask.any():
        return np.full(mask.shape, np.inf)
    return distance_transform_edt(~mask, sampling=tuple(float(s) for s in spacing))


def surface_distances(a, b, spacing=(1., 1., 1.)):
    """sd(a, b): the distance to the nearest border voxel of b, at every border voxel of a"""
    return edt(border(b), spacing)[border(a)]


def degenerate(test, reference):
    """metrics.py:797-803: the test or the reference mask is empty or fills the volume"""
    test, reference = np.asarray(test).astype(bool), np.asarray(reference).astype(bool)
    return (not test.any()) or test.all() or (not reference.any()) or reference.all()


def metrics(test, reference, spacing=(1., 1., 1.), threshold=None, nan_for_nonexisting=True):
    """the four distance metrics of one binary pair (+ "Normalized Surface Dice" when a threshold is given), the surface-voxel
    counts of both directions under "n", and the two distance multisets under "d1" / "d2" """
    out = {}
    if degenerate(test, reference):
        out.update((k, float("NaN") if nan_for_nonexisting else 0.) for k in DISTANCE_KEYS)
        d1 = d2 = None
    else:
        d1 = surface_distances(test, reference, spacing)
        d2 = surface_distances(reference, test, spacing)
        out["Hausdorff Distance"] = float(max(d1.max(), d2.max()))
        out["Hausdorff Distance 95"] = float(np.percentile(np.hstack((d1, d2)), 95))
        out["Avg. Surface Distance"] = float(d1.mean())
        out["Avg. Symmetric Surface Distance"] = float(np.mean((d1.mean(), d2.mean())))
        out["n"] = (int(d1.size), int(d2.size))
    if threshold is not None:          # (a label dict applies the empty / full rule to this entry too: medpy raises on an empty mask)
        out["Normalized Surface Dice"] = (float("NaN") if nan_for_nonexisting else 0.) if d1 is None else \
            normalized_surface_dice(test, reference, threshold, spacing)
    out["d1"], out["d2"] = d1, d2
    return out


def normalized_surface_dice(a, b, threshold, spacing=(1., 1., 1.)):
    """surface_dice.py:49-55: (p + q) / (2 + 1e-8), p / q = the share of each border within ``threshold`` of the other; NaN where
    a border is empty (the reference divides 0 by 0 there)"""
    ba, bb = border(a), border(b)
    if not ba.any() or not bb.any():
        return float("NaN")
    d1, d2 = edt(bb, spacing)[ba], edt(ba, spacing)[bb]
    p, q = np.sum(d1 <= threshold) / d1.size, np.sum(d2 <= threshold) / d2.size
    return float((p + q) / (2 + 1e-8))


def label_metrics(test, reference, labels, spacing, threshold=None, nan_for_nonexisting=True):
    """label -> metrics(test == label, reference == label)"""
    return {l: metrics(np.asarray(test) == l, np.asarray(reference) == l, spacing, threshold, nan_for_nonexisting) for l in labels}
