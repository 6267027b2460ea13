"""Host restatement of the component table (e2enet_medical_amd/postprocessing/component_table.py, csrc/components.hip) with
scipy.ndimage.label and numpy.bincount: the parity yardstick of the device table and the table builder the CPU tests inject.

Per foreground class c: scipy.ndimage.label(pred == c) with its default structure (the 6-neighbour cross); per object its first
voxel in raster order, its voxels, its voxels with gt == c.  The foreground objects are those of label(isin(pred, classes)); a
class object lies in the foreground object that holds its first voxel.  gt_count[c] = (gt == c).sum()."""
import numpy as np
from scipy.ndimage import label

from e2enet_medical_amd.postprocessing.component_table import make_table


def _objects(mask):
    """(label map, first flat index per object, voxels per object)"""
    lmap, n = label(mask)
    flat = lmap.reshape(-1)
    first = np.full(n + 1, flat.size, np.int64)
    np.minimum.at(first, flat, np.arange(flat.size))
    return lmap, first[1:], np.bincount(flat, minlength=n + 1)[1:]


def component_table(pred, gt, classes):
    pred, gt = np.asarray(pred), np.asarray(gt)
    classes = [int(c) for c in classes]
    fg_map, fg_first, fg_size = _objects(np.isin(pred, classes))
    records = []
    for c in classes:
        lmap, first, size = _objects(pred == c)
        tp = np.bincount(lmap.reshape(-1), weights=(gt == c).reshape(-1), minlength=len(first) + 1)[1:].astype(np.int64)
        for f, s, t in zip(first, size, tp):
            records.append((f, c, s, t, fg_first[fg_map.reshape(-1)[f] - 1]))
    return make_table(classes, pred.size, np.array(records, np.int64).reshape(-1, 5), np.stack([fg_first, fg_size], 1),
                      {c: int((gt == c).sum()) for c in classes})


def random_case(shape, fill, seed, labels=3, agree=0.7):
    """a prediction of ``labels`` classes at the given fill and a ground truth that agrees with it on about ``agree`` of the voxels"""
    rng = np.random.RandomState(seed)
    pred = np.zeros(shape, np.uint8)
    m = rng.rand(*shape) < fill
    pred[m] = rng.randint(1, labels + 1, int(m.sum()))
    gt = pred.copy()
    flip = rng.rand(*shape) > agree
    gt[flip] = rng.randint(0, labels + 1, int(flip.sum()))
    return pred, gt
