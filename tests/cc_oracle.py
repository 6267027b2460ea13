"""Host restatement of the reference's remove_all_but_the_largest_connected_component (e2enet/postprocessing/
connected_components.py:50-107) with scipy.ndimage.label: the parity yardstick of the device path (csrc/components.hip).
tests/test_postprocessing_cpu.py checks it against tests/golden/postprocessing.npz, which the reference's own function wrote.

Per entry of ``for_which_classes``, in order, on the volume the earlier entries left: mask = volume in entry's classes;
scipy.ndimage.label with its default structure (the 6-neighbour cross in 3-D); size of an object = voxels * volume_per_voxel (numpy
int64 * float); kept_size = the largest size; an object is set to 0 when its size != the largest size and (no minimum is given or
size < minimum[entry]); largest_removed = the largest size set to 0, None when none was; no object: None for both."""
import numpy as np
from scipy.ndimage import label


def remove_all_but_the_largest_connected_component(image, for_which_classes, volume_per_voxel, minimum_valid_object_size=None):
    """edits ``image`` in place and returns (image, largest_removed, kept_size)"""
    if for_which_classes is None:
        for_which_classes = [int(v) for v in np.unique(image) if v > 0]
    largest_removed, kept_size = {}, {}
    for c in for_which_classes:
        if isinstance(c, (list, tuple)):
            c = tuple(int(v) for v in c)
            members = c
        else:
            c = int(c)
            members = (c,)
        assert 0 not in members, "cannot remove background"
        mask = np.isin(image, members)
        lmap, n = label(mask)
        largest_removed[c] = kept_size[c] = None
        if n == 0:
            continue
        sizes = np.bincount(lmap.reshape(-1), minlength=n + 1)[1:].astype(np.int64) * volume_per_voxel
        biggest = sizes.max()
        kept_size[c] = float(biggest)
        drop = sizes != biggest
        if minimum_valid_object_size is not None:
            drop &= sizes < minimum_valid_object_size[c]
        if drop.any():
            largest_removed[c] = float(sizes[drop].max())
            image[np.concatenate([[False], drop])[lmap]] = 0
    return image, largest_removed, kept_size


def object_sizes(image, members):
    """voxel counts of the 6-connected objects of ``image in members``, ascending"""
    lmap, n = label(np.isin(image, members))
    return np.sort(np.bincount(lmap.reshape(-1), minlength=n + 1)[1:])


def golden_cases():
    """the cases of tests/golden/postprocessing.npz (tools/make_golden_postprocessing.py) as dicts: vol, fwc (as it was given to the
    reference), vpv, mins (dict or None), out, removed, kept (dicts as the reference returned them, None for 'no object')"""
    from tests.helpers import golden
    g = golden("postprocessing.npz")
    cases = []
    for i in range(int(g["num_cases"])):
        keys = []
        for row, joint in zip(g["members_%d" % i], g["joint_%d" % i]):
            t = tuple(int(v) for v in row if v >= 0)
            keys.append(t if joint else t[0])
        given = [list(k) if isinstance(k, tuple) else k for k in keys]
        opt = lambda a: {k: (None if np.isnan(v) else float(v)) for k, v in zip(keys, a)}
        cases.append(dict(vol=g["vol_%d" % i], fwc=None if int(g["none_%d" % i]) else given, vpv=float(g["vpv_%d" % i]),
                          mins={k: float(v) for k, v in zip(keys, g["min_%d" % i])} if int(g["hasmin_%d" % i]) else None,
                          out=g["out_%d" % i], removed=opt(g["removed_%d" % i]), kept=opt(g["kept_%d" % i])))
    return cases
