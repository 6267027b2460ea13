"""Surface-distance metrics on the device: the reference's ``default_advanced_metrics`` ("Hausdorff Distance 95", "Avg. Surface
Distance", "Avg. Symmetric Surface Distance"; e2enet/evaluation/evaluator.py:53-59, metrics.py:792-861), the plain Hausdorff
distance and ``normalized_surface_dice`` (surface_dice.py:20-56), computed by the kernels of csrc/surface.hip instead of one
``scipy.ndimage.distance_transform_edt`` over the whole volume per label and direction.

The contract is medpy's algorithm for connectivity 1, the only value the reference passes:
  border(m) = m & ~erode(m) (6-neighbour cross, outside the volume = 0);  sd(a, b) = distance to the nearest border voxel of b at
  every border voxel of a, under ``voxel_spacing`` (array-axis order);  with d1 = sd(test, reference), d2 = sd(reference, test):
  HD = max(max d1, max d2), HD95 = numpy.percentile(concat(d1, d2), 95), ASD = mean(d1), ASSD = (mean d1 + mean d2) / 2,
  NSD = (p + q) / (2 + 1e-8) with p, q the shares of d1, d2 within the tolerance.
An empty mask or one that fills the volume gives NaN (0 with ``nan_for_nonexisting=False``), decided from voxel counts before
anything is launched (metrics.py:797-803).  There is no host fallback: without the library or a device these functions raise.
"""
from collections import OrderedDict

import numpy as np

DISTANCE_METRICS = ("Hausdorff Distance", "Hausdorff Distance 95", "Avg. Surface Distance", "Avg. Symmetric Surface Distance")
ADVANCED_METRICS = ("Hausdorff Distance 95", "Avg. Surface Distance", "Avg. Symmetric Surface Distance")     # evaluator.py:53-59
NSD_KEY = "Normalized Surface Dice"


def _spacing(voxel_spacing):
    s = (1., 1., 1.) if voxel_spacing is None else tuple(float(v) for v in np.asarray(voxel_spacing).reshape(-1))
    if len(s) != 3 or not all(np.isfinite(v) and v > 0 for v in s):
        raise ValueError("voxel_spacing must be three positive numbers in array-axis order, got %r" % (voxel_spacing,))
    return s


def _label_volume(x, name):
    """a label volume as (host uint8 array or device uint8 tensor), 3-D and contiguous"""
    import torch
    if isinstance(x, torch.Tensor):
        if x.dtype == torch.bool:
            x = x.to(torch.uint8)
        if x.dtype != torch.uint8:
            raise TypeError("%s: a tensor label volume must be uint8 (got %s)" % (name, x.dtype))
    else:
        x = np.asarray(x)
        if x.dtype == np.bool_:
            x = x.astype(np.uint8)
        elif x.dtype != np.uint8:
            if x.size and (x.min() < 0 or x.max() > 255 or (x.dtype.kind == "f" and not np.all(x == np.floor(x)))):
                raise ValueError("%s: labels must be whole numbers in [0, 255]" % name)
            x = x.astype(np.uint8)
    if x.ndim != 3:
        raise ValueError("%s: need a 3-D volume, got shape %s" % (name, tuple(x.shape)))
    return x


def _voxel_counts(x):
    """number of voxels per uint8 value (host array or device tensor)"""
    import torch
    if isinstance(x, torch.Tensor):
        return torch.bincount(x.reshape(-1).to(torch.int32), minlength=256).cpu().numpy()
    return np.bincount(x.reshape(-1), minlength=256)


def label_boxes(test, reference):
    """label value -> the bounding box (three slices) of the voxels that carry it in either volume; one pass per volume.  Both
    borders of a label lie inside its box, a distance at a voxel of the box depends only on border voxels inside it, and every voxel
    next to the box carries another label, which the border rule treats like the outside of the volume: scoring the box alone gives
    the numbers of the whole volume."""
    from scipy.ndimage import find_objects
    boxes = {}
    for vol in (test, reference):
        for v, sl in enumerate(find_objects(np.asarray(vol).astype(np.int16) + 1, max_label=256)):
            if sl is not None:
                boxes[v] = sl if v not in boxes else tuple(slice(min(a.start, b.start), max(a.stop, b.stop)) for a, b in zip(boxes[v], sl))
    return boxes


def _members(label):
    """None for one integer label, else the sorted tuple of distinct values of a label set (a region)"""
    if isinstance(label, (tuple, list, set, frozenset, np.ndarray)):
        return tuple(sorted({int(v) for v in label}))
    return None


def member_words(values):
    """the 256-bit set of uint8 values as the eight words e2e_surface_border_set reads; values outside [0, 255] occur in no volume"""
    import ctypes
    words = (ctypes.c_uint * 8)()
    for v in values:
        if 0 <= int(v) <= 255:
            words[int(v) >> 5] |= 1 << (int(v) & 31)
    return words


def union_box(boxes, values):
    """the smallest box around the boxes of ``values`` (those that have one); None when none has"""
    have = [boxes[v] for v in values if v in boxes]
    if not have:
        return None
    return tuple(slice(min(b[a].start for b in have), max(b[a].stop for b in have)) for a in range(3))


class SurfaceScorer:
    """Both label volumes of one case on the device (uploaded once); every label of the case is scored from that copy, inside the
    label's bounding box when ``crop`` is set.  ``boxes``: value -> three slices, e.g. from ``evaluator.label_census``; given, it
    replaces the host ``find_objects`` pass of ``label_boxes``.  A label is one integer or a tuple of integers (a region: the
    mask "value is in the tuple"), scored inside the union of its members' boxes."""

    def __init__(self, test, reference, voxel_spacing=None, crop=True, boxes=None):
        import torch
        from .._lib import lib
        if not torch.cuda.is_available():
            raise RuntimeError("surface-distance metrics run on the GPU (csrc/surface.hip); there is no host fallback")
        self.L = lib()
        self.spacing = _spacing(voxel_spacing)
        test, reference = _label_volume(test, "test"), _label_volume(reference, "reference")
        if tuple(test.shape) != tuple(reference.shape):
            raise ValueError("Shape mismatch: {} and {}".format(tuple(test.shape), tuple(reference.shape)))
        dev = torch.device("cuda")
        host = lambda x: x.cpu().numpy() if isinstance(x, torch.Tensor) else x
        self.boxes = None if not crop else dict(boxes) if boxes is not None else label_boxes(host(test), host(reference))
        # (np.array: a contiguous copy torch may wrap whatever the caller's array allows)
        up = lambda x: (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.array(x, order="C"))).to(dev).contiguous()
        self.test, self.reference = up(test), up(reference)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.out = torch.empty(10, dtype=torch.float64, device=dev)
        self.count = torch.empty(2, dtype=torch.int64, device=dev)
        self.ws = torch.empty(self.L.surface_distances_ws_bytes(), dtype=torch.uint8, device=dev)
        self.select(None)

    def select(self, label):
        """the volumes the next calls work on: the label's bounding box of both volumes (a contiguous device copy), or the whole
        volumes for ``label=None`` or a scorer built with ``crop=False``"""
        import torch
        if label is None or self.boxes is None:
            box = None
        else:
            members = _members(label)
            box = self.boxes.get(int(label)) if members is None else union_box(self.boxes, members)
        self.vols = [self.test, self.reference] if box is None else [self.test[box].contiguous(), self.reference[box].contiguous()]
        self.shape = tuple(int(v) for v in self.vols[0].shape)
        dev = self.test.device
        self.borders = [torch.empty(self.shape, dtype=torch.uint8, device=dev) for _ in range(2)]
        self.dt2 = [torch.empty(self.shape, dtype=torch.float32, device=dev) for _ in range(2)]

    def border(self, which, label):
        """(border mask uint8 tensor of the selected volumes' shape; number of border voxels, a device scalar) of
        ``volume == label`` (a tuple: of "volume is one of its values"); ``which``: 0 = test, 1 = reference"""
        D, H, W = self.shape
        members = _members(label)
        if members is None:
            self.L.surface_border(self.vols[which].data_ptr(), int(label), self.borders[which].data_ptr(), self.count[which:].data_ptr(),
                                  D, H, W, self.stream)
        else:
            self.L.surface_border_set(self.vols[which].data_ptr(), member_words(members), self.borders[which].data_ptr(),
                                      self.count[which:].data_ptr(), D, H, W, self.stream)
        return self.borders[which], self.count[which]

    def edt_sq(self, which):
        """squared distance (fp32 tensor) to the nearest voxel of border mask ``which``"""
        D, H, W = self.shape
        self.L.distance_transform_edt_sq(self.borders[which].data_ptr(), self.dt2[which].data_ptr(), D, H, W, *self.spacing, self.stream)
        return self.dt2[which]

    def stats(self, label, threshold=None):
        """Raw record of one label whose masks are neither empty nor full: surface-voxel counts, sums, maxima, counts within
        ``threshold`` of both directions and the two order statistics around rank 0.95 (N - 1)."""
        self.select(label)
        self.border(0, label)
        self.border(1, label)
        self.edt_sq(0)
        self.edt_sq(1)
        n1, n2 = (int(v) for v in self.count.cpu())               # (the one read between launches: the ranks HD95 needs)
        if n1 == 0 or n2 == 0:
            raise RuntimeError("label %r has no voxel in one of the volumes: apply the empty-mask rule first" % (label,))
        rank = 0.95 * (n1 + n2 - 1)                               # numpy.percentile, linear interpolation
        lo = int(np.floor(rank))
        hi = min(lo + 1, n1 + n2 - 1)
        thr = float("inf") if threshold is None else float(threshold)
        self.L.surface_distances_stats(self.borders[0].data_ptr(), self.dt2[1].data_ptr(), self.borders[1].data_ptr(), self.dt2[0].data_ptr(),
                                       self.vols[0].numel(), thr, lo, hi, self.out.data_ptr(), self.ws.data_ptr(), self.stream)
        o = self.out.cpu().numpy()
        if int(o[0]) != n1 or int(o[4]) != n2:
            raise RuntimeError("surface reduction saw %d / %d border voxels, the border kernel counted %d / %d" % (o[0], o[4], n1, n2))
        return dict(n=(n1, n2), sum=(float(o[1]), float(o[5])), max=(float(o[2]), float(o[6])), within=(int(o[3]), int(o[7])),
                    q=(float(o[8]), float(o[9])), frac=float(rank - lo))

    def metrics(self, label, nsd_tolerance=None):
        r = self.stats(label, nsd_tolerance)
        (n1, n2), (s1, s2) = r["n"], r["sum"]
        out = {"Hausdorff Distance": max(r["max"]),
               "Hausdorff Distance 95": r["q"][0] + (r["q"][1] - r["q"][0]) * r["frac"],
               "Avg. Surface Distance": s1 / n1,
               "Avg. Symmetric Surface Distance": (s1 / n1 + s2 / n2) / 2.}
        if nsd_tolerance is not None:
            out[NSD_KEY] = (r["within"][0] / n1 + r["within"][1] / n2) / (2 + 1e-8)
        return out


def _degenerate(counts_test, counts_ref, size, label):
    t, r = int(counts_test[label]), int(counts_ref[label])
    return t == 0 or t == size or r == 0 or r == size


def surface_distance_metrics(test, reference, labels, voxel_spacing, nsd_tolerance=None, nan_for_nonexisting=True):
    """label -> {"Hausdorff Distance", "Hausdorff Distance 95", "Avg. Surface Distance", "Avg. Symmetric Surface Distance"} (and
    "Normalized Surface Dice" when ``nsd_tolerance`` is given) of the binary maps ``test == label`` / ``reference == label``.

    ``test`` / ``reference``: 3-D label volumes (numpy arrays with whole-number labels in [0, 255], or device uint8 tensors),
    uploaded once; every label is scored from that copy and no ``volume == label`` map is materialised.  ``voxel_spacing``: three
    positive numbers in array-axis order (None: 1 mm).  A label whose test or reference mask is empty or fills the volume gets
    NaN, or 0 with ``nan_for_nonexisting=False``, for every entry; that is decided from voxel counts, without the device."""
    spacing = _spacing(voxel_spacing)
    test, reference = _label_volume(test, "test"), _label_volume(reference, "reference")
    if tuple(test.shape) != tuple(reference.shape):
        raise ValueError("Shape mismatch: {} and {}".format(tuple(test.shape), tuple(reference.shape)))
    labels = [int(l) for l in labels]
    if any(l < 0 or l > 255 for l in labels):
        raise ValueError("labels must lie in [0, 255], got %r" % (labels,))
    keys = DISTANCE_METRICS + ((NSD_KEY,) if nsd_tolerance is not None else ())
    size = int(np.prod(tuple(test.shape)))
    ct, cr = _voxel_counts(test), _voxel_counts(reference)
    nan = float("NaN") if nan_for_nonexisting else 0.
    scorer, out = None, OrderedDict()
    for l in labels:
        if size == 0 or _degenerate(ct, cr, size, l):
            out[l] = OrderedDict((k, nan) for k in keys)
            continue
        if scorer is None:
            scorer = SurfaceScorer(test, reference, spacing)
        m = scorer.metrics(l, nsd_tolerance)
        out[l] = OrderedDict((k, m[k]) for k in keys)
    return out


def _binary_pair(test, reference, voxel_spacing, connectivity, nan_for_nonexisting=True, threshold=None):
    if connectivity != 1:
        raise NotImplementedError("connectivity %r: only the 6-neighbour cross (connectivity=1) is built, the one value the "
                                  "reference passes" % (connectivity,))
    test, reference = np.asarray(test), np.asarray(reference)
    return surface_distance_metrics(test != 0, reference != 0, [1], voxel_spacing, threshold, nan_for_nonexisting)[1]


def hausdorff_distance(test=None, reference=None, confusion_matrix=None, nan_for_nonexisting=True, voxel_spacing=None, connectivity=1,
                       **kwargs):
    """metrics.py:792-807 (``confusion_matrix`` is accepted for the signature's sake and not used)"""
    return _binary_pair(test, reference, voxel_spacing, connectivity, nan_for_nonexisting)["Hausdorff Distance"]


def hausdorff_distance_95(test=None, reference=None, confusion_matrix=None, nan_for_nonexisting=True, voxel_spacing=None,
                          connectivity=1, **kwargs):
    """metrics.py:810-825"""
    return _binary_pair(test, reference, voxel_spacing, connectivity, nan_for_nonexisting)["Hausdorff Distance 95"]


def avg_surface_distance(test=None, reference=None, confusion_matrix=None, nan_for_nonexisting=True, voxel_spacing=None,
                         connectivity=1, **kwargs):
    """metrics.py:828-843: test -> reference only"""
    return _binary_pair(test, reference, voxel_spacing, connectivity, nan_for_nonexisting)["Avg. Surface Distance"]


def avg_surface_distance_symmetric(test=None, reference=None, confusion_matrix=None, nan_for_nonexisting=True, voxel_spacing=None,
                                   connectivity=1, **kwargs):
    """metrics.py:846-861"""
    return _binary_pair(test, reference, voxel_spacing, connectivity, nan_for_nonexisting)["Avg. Symmetric Surface Distance"]


def normalized_surface_dice(a, b, threshold, spacing=None, connectivity=1):
    """surface_dice.py:20-56.  NaN where a mask is empty or fills the volume (medpy raises on an empty one)."""
    return _binary_pair(a, b, spacing, connectivity, True, float(threshold))[NSD_KEY]
