"""Host restatement, in fp64 numpy / scipy, of the reference's preprocessing of one case (e2enet/preprocessing/cropping.py and
preprocessing.py, GenericPreprocessor): the yardstick of the device path (csrc/preprocess.hip).

scikit-image, batchgenerators and SimpleITK are not installed here, so the two third-party resizes are restated from their
definitions instead of being called:
  * ``skimage.transform.resize(x, shape, order, mode='edge', anti_aliasing=False, clip=True)`` evaluates, from scikit-image 0.19 on,
    ``scipy.ndimage.zoom(x, shape / x.shape, order=order, mode='nearest', grid_mode=True)`` and clips it to ``[x.min(), x.max()]``;
  * batchgenerators' ``resize_segmentation(seg, shape, order=1)`` starts from zeros and, for every label of ``np.unique(seg)`` in
    ascending order, writes the label where that resize of the label's binary mask is ``>= 0.5``.
Two identities the device code is built on are restated here and checked in tests/test_preprocess_cpu.py: the order-3 zoom equals
edge padding by 12, the mirror spline prefilter and a cubic gather at shifted coordinates; and ``binary_fill_holes`` equals adding
every background component that has no voxel on a face of the volume."""
import numpy as np
from scipy import ndimage as ndi

SPLINE_PAD = 12


# ---------------------------------------------------------------------------------------------------------------- cropping
def create_nonzero_mask(data):
    mask = np.zeros(data.shape[1:], dtype=bool)
    for c in range(data.shape[0]):
        mask |= data[c] != 0                                   # (NaN != 0 is True)
    return ndi.binary_fill_holes(mask)


def fill_holes_by_labelling(mask):
    """binary_fill_holes as the device computes it: label the background with the 6-neighbour structure; a component is a hole
    when none of its voxels lies on a face of the volume"""
    lab, n = ndi.label(~mask)
    outside = np.zeros(n + 1, dtype=bool)
    for a in range(mask.ndim):
        for face in (0, -1):
            outside[np.unique(np.take(lab, face, axis=a))] = True
    outside[0] = False
    return mask | ((lab > 0) & ~outside[lab])


def get_bbox_from_mask(mask, outside_value=0):
    idx = np.where(mask != outside_value)
    return [[int(np.min(i)), int(np.max(i)) + 1] for i in idx]


def crop_to_nonzero(data, seg=None, nonzero_label=-1):
    mask = create_nonzero_mask(data)
    bbox = get_bbox_from_mask(mask, 0)
    sl = tuple(slice(b[0], b[1]) for b in bbox)
    data = data[(slice(None),) + sl].copy()
    mask = mask[sl][None]
    if seg is not None:
        seg = seg[(slice(None),) + sl].copy()
        seg[(seg == 0) & (mask == 0)] = nonzero_label
    else:
        seg = np.where(mask, 0, nonzero_label).astype(int)
    return data, seg, bbox


def crop(data, properties, seg=None):
    """ImageCropper.crop"""
    data, seg, bbox = crop_to_nonzero(data, seg, -1)
    properties["crop_bbox"] = bbox
    properties["classes"] = np.unique(seg)
    seg[seg < -1] = 0
    properties["size_after_cropping"] = data[0].shape
    return data, seg, properties


# ---------------------------------------------------------------------------------------------------------------- resizing
def zoom(x, new_shape, order):
    x = np.asarray(x, dtype=np.float64)
    return ndi.zoom(x, [n / o for n, o in zip(new_shape, x.shape)], order=order, mode='nearest', grid_mode=True)


def zoom3_by_padding(x, new_shape):
    """the order-3 zoom spelled out: edge padding by 12, mirror prefilter, cubic gather at (o + 0.5) old / new - 0.5 + 12"""
    x = np.asarray(x, dtype=np.float64)
    coef = ndi.spline_filter(np.pad(x, SPLINE_PAD, mode='edge'), order=3, mode='mirror')
    grid = np.meshgrid(*[(np.arange(n) + 0.5) * o / n - 0.5 + SPLINE_PAD for n, o in zip(new_shape, x.shape)], indexing='ij')
    return ndi.map_coordinates(coef, np.array(grid), order=3, mode='mirror', prefilter=False)


def resize(x, new_shape, order=3, clip=True):
    """skimage.transform.resize(order, mode='edge', anti_aliasing=False, clip=clip)"""
    out = zoom(x, new_shape, order)
    return np.clip(out, np.min(x), np.max(x)) if clip else out


def resize_segmentation(seg, new_shape, order=1):
    """(resized seg, margin): margin = the smallest |interpolant - 0.5| over the labels, per voxel: how close the voxel's decision
    is to a rounding boundary"""
    out = np.zeros(new_shape, dtype=seg.dtype)
    margin = np.full(new_shape, np.inf)
    for c in np.unique(seg):
        m = resize((seg == c).astype(np.float64), new_shape, order)
        out[m >= 0.5] = c
        margin = np.minimum(margin, np.abs(m - 0.5))
    return out, margin


def order0_along(x, axis, new_len):
    """map_coordinates(order=0, mode='nearest') along one axis at (o + 0.5) old / new - 0.5 (the other coordinates are whole)"""
    old = x.shape[axis]
    c = np.clip((old / new_len) * (np.arange(new_len) + 0.5) - 0.5, 0, old - 1)
    return np.take(x, np.floor(c + 0.5).astype(int), axis=axis)


def resample_data_or_seg(data, new_shape, is_seg, axis=None, order=3, do_separate_z=False, clip=True):
    """(resampled [C, ...] in fp64 for data / the seg's dtype for a seg, margin or None); order_z = 0"""
    shape = np.array(data[0].shape)
    new_shape = np.array(new_shape)
    if not np.any(shape != new_shape):
        return data, None
    outs, margins = [], []
    for c in range(data.shape[0]):
        if do_separate_z:
            ax = int(axis[0])
            new_2d = tuple(int(v) for a, v in enumerate(new_shape) if a != ax)
            sl, mg = [], []
            for i in range(shape[ax]):
                plane = np.take(data[c], i, axis=ax)
                if is_seg:
                    r, m = resize_segmentation(plane, new_2d, order)
                    mg.append(m)
                else:
                    r = resize(plane, new_2d, order, clip).astype(np.float32).astype(np.float64)       # (.astype(dtype_data) per slice)
                sl.append(r)
            vol = np.stack(sl, ax)
            mvol = np.stack(mg, ax) if is_seg else None
            if shape[ax] != new_shape[ax]:
                vol = order0_along(vol, ax, int(new_shape[ax]))
                mvol = order0_along(mvol, ax, int(new_shape[ax])) if is_seg else None
        elif is_seg:
            vol, mvol = resize_segmentation(data[c], tuple(int(v) for v in new_shape), order)
        else:
            vol, mvol = resize(data[c], tuple(int(v) for v in new_shape), order, clip), None
        outs.append(vol)
        margins.append(mvol)
    return np.stack(outs), (np.stack(margins) if is_seg else None)


RESAMPLING_SEPARATE_Z_ANISO_THRESHOLD = 3


def separate_z_plan(original_spacing, target_spacing, force_separate_z=None):
    sep = lambda s: (np.max(s) / np.min(s)) > RESAMPLING_SEPARATE_Z_ANISO_THRESHOLD
    low = lambda s: np.where(max(s) / np.array(s) == 1)[0]
    if force_separate_z is not None:
        do, axis = force_separate_z, (low(original_spacing) if force_separate_z else None)
    elif sep(original_spacing):
        do, axis = True, low(original_spacing)
    elif sep(target_spacing):
        do, axis = True, low(target_spacing)
    else:
        do, axis = False, None
    if axis is not None and len(axis) != 1:
        do = False
    return do, axis


def resampled_shape(shape, original_spacing, target_spacing):
    return np.round(((np.array(original_spacing) / np.array(target_spacing)).astype(float) * np.array(shape))).astype(int)


# ---------------------------------------------------------------------------------------------------------------- normalising
def normalize(data, seg, schemes, use_nonzero_mask, intensityproperties=None):
    """the normalisation loop of resample_and_normalize in fp64; data [C, ...], seg [S, ...] or None"""
    data = np.array(data, dtype=np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        for c in range(len(data)):
            scheme = schemes[c]
            if scheme == "CT":
                ip = intensityproperties[c]
                data[c] = (np.clip(data[c], ip['percentile_00_5'], ip['percentile_99_5']) - ip['mean']) / ip['sd']
                if use_nonzero_mask[c]:
                    data[c][seg[-1] < 0] = 0
            elif scheme == "CT2":
                ip = intensityproperties[c]
                lb, ub = ip['percentile_00_5'], ip['percentile_99_5']
                mask = (data[c] > lb) & (data[c] < ub)
                data[c] = np.clip(data[c], lb, ub)
                sel = data[c][mask]
                mn, sd = (sel.mean(), sel.std()) if sel.size else (np.nan, np.nan)
                data[c] = (data[c] - mn) / sd
                if use_nonzero_mask[c]:
                    data[c][seg[-1] < 0] = 0
            elif scheme == "noNorm":
                pass
            elif use_nonzero_mask[c]:
                mask = seg[-1] >= 0
                data[c][mask] = (data[c][mask] - data[c][mask].mean()) / (data[c][mask].std() + 1e-8)
                data[c][mask == 0] = 0
            else:
                data[c] = (data[c] - data[c].mean()) / (data[c].std() + 1e-8)
    return data


def preprocess_test_case(data, properties, target_spacing, schemes, use_nonzero_mask, transpose_forward, intensityproperties=None,
                         order_data=3, force_separate_z=None):
    """GenericPreprocessor.preprocess_test_case on an in-memory case: (data fp64, seg, properties, resampled data before the
    normalisation)"""
    properties = dict(properties)
    data, seg, properties = crop(np.array(data, dtype=np.float32), properties, None)
    perm = (0, *[i + 1 for i in transpose_forward])
    data, seg = data.transpose(perm), seg.transpose(perm)
    spacing = np.array(properties["original_spacing"])[list(transpose_forward)]
    data = np.where(np.isnan(data), 0, data)
    new_shape = resampled_shape(data[0].shape, spacing, target_spacing)
    do, axis = separate_z_plan(spacing, target_spacing, force_separate_z)
    data, _ = resample_data_or_seg(data, new_shape, False, axis, order_data, do)
    data = np.asarray(data, dtype=np.float32)
    seg, _ = resample_data_or_seg(seg, new_shape, True, axis, 1, do)
    seg[seg < -1] = 0
    properties["size_after_resampling"] = data[0].shape
    properties["spacing_after_resampling"] = target_spacing
    return normalize(data, seg, schemes, use_nonzero_mask, intensityproperties), seg, properties, data


# ---------------------------------------------------------------------------------------------------------------- test volumes
def step_volume(shape, seed, lo=0.0, hi=1.0):
    """a box and a one-voxel spike of height hi - lo over the level lo, plus a little noise: step edges on every axis, so that a
    cubic resize leaves [min, max] at every ratio (the spike undershoots where an exact halving samples beside the box's faces)"""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=shape) * 0.002
    x[tuple(slice(s // 3, s // 3 + max(1, s // 2)) for s in shape)] += 1.0
    x[(1,) * len(shape)] += 1.0
    return (lo + (hi - lo) * x).astype(np.float32)


def step_case(shape, seed, lo=0.0, hi=1.0):
    """[C, ...]: one step_volume per modality"""
    return np.stack([step_volume(shape[1:], seed + c, lo, hi) for c in range(shape[0])])
