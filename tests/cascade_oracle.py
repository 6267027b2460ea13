"""Host restatements for the cascade tests (tests/test_cascade_cpu.py, tests/test_gpu_cascade.py): what scikit-image evaluates in the
reference's pyramid_augmentations.py, through scipy.ndimage with the arguments scikit-image passes.

  binary_dilation(x, fp)  = scipy.ndimage.binary_dilation(x, structure=fp)                      (border 0)
  binary_erosion(x, fp)   = scipy.ndimage.binary_erosion(x, structure=fp, border_value=True)
  binary_closing          = erosion(dilation(x));   binary_opening = dilation(erosion(x))
  label(x)                = scipy.ndimage.label(x, structure=np.ones((3, 3, 3)))                 (full connectivity)
"""
import numpy as np
from scipy import ndimage

DILATION, EROSION, CLOSING, OPENING = 0, 1, 2, 3


def ball_literal(r):
    """skimage.morphology.ball, the expression itself"""
    n = 2 * r + 1
    Z, Y, X = np.mgrid[-r:r:n * 1j, -r:r:n * 1j, -r:r:n * 1j]
    s = X ** 2 + Y ** 2 + Z ** 2
    return s <= r * r


def dilation(x, fp):
    return ndimage.binary_dilation(x, structure=fp)


def erosion(x, fp):
    return ndimage.binary_erosion(x, structure=fp, border_value=True)


def morphology(x, fp, op):
    x = np.asarray(x) != 0
    fp = np.asarray(fp) != 0
    if op == DILATION:
        return dilation(x, fp)
    if op == EROSION:
        return erosion(x, fp)
    if op == CLOSING:
        return erosion(dilation(x, fp), fp)
    if op == OPENING:
        return dilation(erosion(x, fp), fp)
    raise ValueError(op)


def _shifted(x, off, fill):
    """y[p] = x[p + off], `fill` where p + off lies outside"""
    y = np.full(x.shape, fill, dtype=bool)
    src, dst = [], []
    for n, o in zip(x.shape, off):
        lo, hi = max(0, -o), min(n, n - o)
        if lo >= hi:
            return y
        dst.append(slice(lo, hi))
        src.append(slice(lo + o, hi + o))
    y[tuple(dst)] = x[tuple(src)]
    return y


def run_table_pass(x, table, reflect, complement):
    """What e2e_morph_pass computes from a run table, in numpy: OR over the table's voxels o of x[p - o] (reflect: x[p + o]), zero
    outside; complement: on the complement of x, the result complemented."""
    x = np.asarray(x) != 0
    src = ~x if complement else x
    out = np.zeros(x.shape, dtype=bool)
    for oz, oy, lo, hi in np.asarray(table).reshape(-1, 4):
        for ox in range(int(lo), int(hi) + 1):
            o = (int(oz), int(oy), ox)
            out |= _shifted(src, o if reflect else tuple(-v for v in o), False)
    return ~out if complement else out


PASSES = {DILATION: ((0, 0),), EROSION: ((1, 1),), CLOSING: ((0, 0), (1, 1)), OPENING: ((1, 1), (0, 0))}


def run_table_morphology(x, table, op):
    for reflect, complement in PASSES[op]:
        x = run_table_pass(x, table, reflect, complement)
    return x


def binary_operator(sample, channel, op, fp, others):
    """ApplyRandomBinaryOperatorTransform's body for one channel of a sample [C, D, H, W], in place"""
    workon = sample[channel] != 0
    res = morphology(workon, fp, op)
    sample[channel] = res.astype(sample.dtype)
    added = res & ~workon
    for oc in others:
        sample[oc][added] = 0
    return sample


def components(x):
    """(label map, sizes[1 .. n]) with full connectivity; ids in raster order of each component's first voxel"""
    lab, n = ndimage.label(np.asarray(x) != 0, structure=np.ones((3, 3, 3)))
    return lab, np.bincount(lab.reshape(-1), minlength=n + 1)[1:]


def remove_component(sample, channel, threshold, u, fill_channel=None):
    """The removal of one component of sample[channel], in place.  Returns (components, eligible, removed size)."""
    lab, sizes = components(sample[channel])
    ids = [i + 1 for i, s in enumerate(sizes) if float(s) < threshold]
    if not ids:
        return len(sizes), 0, 0
    pick = ids[min(int(np.floor(u * len(ids))), len(ids) - 1)]
    m = lab == pick
    sample[channel][m] = 0
    if fill_channel is not None:
        sample[fill_channel][m] = 1
    return len(sizes), len(ids), int(sizes[pick - 1])


def blobs(shape, seed, sigma=2.0, level=0.0):
    """smoothed noise thresholded: blobs that touch every face of the volume"""
    rng = np.random.RandomState(seed)
    f = ndimage.gaussian_filter(rng.standard_normal(shape), sigma, mode="wrap")
    x = (f > level * f.std()).astype(np.float32)
    for ax in range(3):                                             # one seeded voxel on each face, whatever the noise gave
        for side in (0, shape[ax] - 1):
            p = [int(rng.randint(n)) for n in shape]
            p[ax] = side
            x[tuple(p)] = 1
    return x
