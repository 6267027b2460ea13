"""Region-based evaluation (reference e2enet/evaluation/region_based_evaluation.py:12-50): the label sets that are scored as
overlapping regions, and the Dice of one case per region.

The NIfTI-folder walker ``evaluate_regions`` (:53-110) reads volumes with SimpleITK and scores them with medpy; both are host
tooling outside this package.  ``evaluate_case`` here takes the two label arrays themselves.
"""
import numpy as np


def get_brats_regions():
    """the three BraTS regions: whole tumour contains tumour core contains enhancing tumour (labels 1 edema, 2 non-enhancing
    tumour, 3 enhancing tumour after the reference's label conversion)"""
    return {
        "whole tumor": (1, 2, 3),
        "tumor core": (2, 3),
        "enhancing tumor": (3,)
    }


def get_KiTS_regions():
    return {
        "kidney incl tumor": (1, 2),
        "tumor": (2,)
    }


def create_region_from_mask(mask, join_labels: tuple):
    mask_new = np.zeros_like(mask, dtype=np.uint8)
    for l in join_labels:
        mask_new[mask == l] = 1
    return mask_new


def evaluate_case(pred, gt, regions):
    """Dice per region of two label arrays of one shape (reference :41-50 on the arrays its two files hold).  ``regions``: a
    sequence of label tuples, or a region dict (its values, in order).  A region that is empty in both arrays scores ``nan``;
    the Dice itself is medpy's ``metric.dc``: 2 |A and B| / (|A| + |B|)."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    if pred.shape != gt.shape:
        raise ValueError("prediction %s and ground truth %s differ in shape" % (pred.shape, gt.shape))
    if isinstance(regions, dict):
        regions = list(regions.values())
    results = []
    for r in regions:
        mask_pred = create_region_from_mask(pred, r).astype(bool)
        mask_gt = create_region_from_mask(gt, r).astype(bool)
        n_pred, n_gt = int(mask_pred.sum()), int(mask_gt.sum())
        if n_pred == 0 and n_gt == 0:
            results.append(np.nan)
        else:
            results.append(2.0 * int((mask_pred & mask_gt).sum()) / float(n_pred + n_gt))
    return results
