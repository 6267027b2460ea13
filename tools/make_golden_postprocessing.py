#!/usr/bin/env python
"""Generate tests/golden/postprocessing.npz by importing the REFERENCE's remove_all_but_the_largest_connected_component
(e2enet/postprocessing/connected_components.py:50-107) with the packages its module imports and this image lacks stubbed, as
tools/make_golden.py does.  Runs on the CPU of the build container only; the file holds data alone: a few small label volumes,
how ``for_which_classes`` was given, ``volume_per_voxel``, the minimum sizes, and what the reference returned.

    python tools/make_golden_postprocessing.py

Encoding, per case i: vol_i (uint8 input), out_i (uint8 output), vpv_i (float64), none_i (1: for_which_classes was None, the
entries below are then the keys the reference made), members_i (int16 [entries, 4], padded with -1), joint_i (1: the entry was given
as a list / tuple), min_i (float64 per entry, NaN-filled and unused when hasmin_i is 0), removed_i / kept_i (float64 per entry,
NaN = None)."""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden", "postprocessing.npz")


def install_stubs():
    fo = types.ModuleType('batchgenerators.utilities.file_and_folder_operations')
    fo.join, fo.isdir, fo.isfile = os.path.join, os.path.isdir, os.path.isfile
    fo.__all__ = ['join', 'isdir', 'isfile']
    ev = types.ModuleType('e2enet.evaluation.evaluator')
    ev.aggregate_scores = None
    sk = types.ModuleType('e2enet.utilities.sitk_stuff')
    sk.copy_geometry = None
    cfg = types.ModuleType('e2enet.configuration')
    cfg.default_num_threads = 1
    for n, m in [('batchgenerators', types.ModuleType('batchgenerators')),
                 ('batchgenerators.utilities', types.ModuleType('batchgenerators.utilities')),
                 ('batchgenerators.utilities.file_and_folder_operations', fo),
                 ('SimpleITK', types.ModuleType('SimpleITK')),
                 ('e2enet.evaluation.evaluator', ev), ('e2enet.utilities.sitk_stuff', sk), ('e2enet.configuration', cfg)]:
        sys.modules[n] = m


def cases():
    """(volume, for_which_classes, volume_per_voxel, minimum sizes or None)"""
    rng = np.random.RandomState(7)

    def blobs(shape, fill, labels=3):
        v = np.zeros(shape, np.uint8)
        m = rng.rand(*shape) < fill
        v[m] = rng.randint(1, labels + 1, int(m.sum()))
        return v
    a = blobs((6, 9, 11), 0.45)
    b = blobs((4, 13, 10), 0.6)
    twins = np.zeros((3, 5, 7), np.uint8)
    twins[0, 0, 0:3] = 1
    twins[2, 4, 4:7] = 1                      # two largest objects of equal size: both stay
    twins[1, 2, 3] = 1
    twins[0, 4, 0:2] = 2
    return [(a, None, 1.0, None),
            (a, [(1, 2, 3)], 0.75, None),
            (a, [[1, 2, 3], 2, 3], 2.5 * 0.8 * 0.7, None),
            (b, [1, 2, 3], 0.5, {1: 2.0, 2: 1.0, 3: 100.0}),
            (b, [(1, 2, 3), 1], 1.25, {(1, 2, 3): 3.0, 1: 2.6}),
            (twins, [1, 2, 4], 1.0, None),
            (twins, [(1, 2)], 0.3, {(1, 2): 0.5})]


def main():
    install_stubs()
    from e2enet.postprocessing.connected_components import remove_all_but_the_largest_connected_component as ref
    out = {}
    todo = cases()
    for i, (vol, fwc, vpv, mins) in enumerate(todo):
        img, removed, kept = ref(vol.copy(), fwc, vpv, mins)
        keys = list(kept.keys())
        members = np.full((len(keys), 4), -1, np.int16)
        joint = np.zeros(len(keys), np.uint8)
        for n, k in enumerate(keys):
            t = tuple(k) if isinstance(k, tuple) else (int(k),)
            members[n, :len(t)] = t
            joint[n] = isinstance(k, tuple)
        nan = float("nan")
        out["vol_%d" % i], out["out_%d" % i] = vol, img.astype(np.uint8)
        out["vpv_%d" % i] = np.float64(vpv)
        out["none_%d" % i] = np.uint8(fwc is None)
        out["members_%d" % i], out["joint_%d" % i] = members, joint
        out["hasmin_%d" % i] = np.uint8(mins is not None)
        out["min_%d" % i] = np.array([nan if mins is None else float(mins[k]) for k in keys], np.float64)
        out["removed_%d" % i] = np.array([nan if removed[k] is None else float(removed[k]) for k in keys], np.float64)
        out["kept_%d" % i] = np.array([nan if kept[k] is None else float(kept[k]) for k in keys], np.float64)
    out["num_cases"] = np.int64(len(todo))
    np.savez_compressed(OUT, **out)
    print("wrote %s: %d cases, %d bytes" % (OUT, len(todo), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
