"""The post-processing search without removed volumes: a table of the prediction's connected components per case (csrc/components.hip,
``e2e_ct_label`` / ``e2e_ct_emit``) and host arithmetic over the tables.

The search of ``determine_postprocessing`` (reference connected_components.py:124-399) asks, for three to five removal sweeps, what
the per-class ``tp, fp, fn`` of every case would be after "remove all but the largest component".  It never needs the removed
volumes for that:

  * removing an object of class ``c`` lowers that class's ``tp`` by the object's own ``tp`` (its voxels with ``gt == pred``) and its
    positives by the object's size; the ground truth does not change, so ``fn = gt_count[c] - tp``;
  * removing an object of the joint foreground region removes whole class objects, the ones that lie in it;
  * what is left of a class after either removal are whole objects of the raw prediction, with the sizes they had.

So one device visit per case gives every sweep.  The table:

  classes   the foreground classes, in the order given
  voxels    voxels of the volume
  first     int64 [n]  flat index of each class object's first voxel in raster order; the records are sorted by it
  label     int64 [n]  its class
  size      int64 [n]  its voxels
  tp        int64 [n]  its voxels with gt == pred
  fg        int64 [n]  index into the foreground records of the foreground object it lies in
  fg_first  int64 [m]  first voxel of each foreground object (sorted), fg_size its voxels
  gt_count  class -> voxels of the ground truth that carry it (from the label census, csrc/evaluate.hip)

A ``(label, case)`` with no voxel has no record.  There is no host fallback: without the library or a device ``component_table``
raises.  ``counts_after`` and ``search`` are host code and need neither.
"""
import os
from collections import OrderedDict, namedtuple
from copy import deepcopy

import numpy as np

ComponentTable = namedtuple("ComponentTable", "classes voxels first label size tp fg fg_first fg_size gt_count")


def make_table(classes, voxels, class_records, fg_records, gt_count):
    """records in any order (``[n, 5]``: first, label, size, tp, first voxel of the foreground object; ``[m, 2]``: first, size) ->
    the table, sorted by first voxel, ``fg`` an index into the foreground records"""
    cr = np.asarray(class_records, dtype=np.int64).reshape(-1, 5)
    fr = np.asarray(fg_records, dtype=np.int64).reshape(-1, 2)
    cr, fr = cr[np.argsort(cr[:, 0], kind="stable")], fr[np.argsort(fr[:, 0], kind="stable")]
    fg = np.searchsorted(fr[:, 0], cr[:, 4])
    if len(cr) and (len(fr) == 0 or fg.max() >= len(fr) or not np.array_equal(fr[fg, 0], cr[:, 4])):
        raise ValueError("component table: a class component names a foreground component that has no record")
    return ComponentTable(tuple(int(c) for c in classes), int(voxels), cr[:, 0], cr[:, 1], cr[:, 2], cr[:, 3], fg, fr[:, 0], fr[:, 1],
                          {int(c): int(gt_count[c]) for c in classes})


def component_table(pred, gt, classes):
    """The table of one case.  ``pred``, ``gt``: 3-D label volumes of one shape, host arrays with whole-number labels in [0, 255]
    (uploaded once) or contiguous device uint8 tensors (read where they are); ``classes``: the foreground classes (never 0)."""
    import ctypes
    import torch
    from .._lib import lib, E2EError
    from ..evaluation.evaluator import _device_pair, _census, _evaluated_values
    from .connected_components import _class_words
    classes = [int(c) for c in classes]
    assert 0 not in classes, "background has no components"
    x, g = _device_pair(pred, gt)
    if x.dim() != 3:
        raise ValueError("component_table: the volumes have shape %s, not three axes" % (tuple(x.shape),))
    D, H, W = (int(v) for v in x.shape)
    joint, slot_of, _ = _census(x, g, _evaluated_values([(None, c) for c in classes]))
    gt_count = {c: int(joint[slot_of[c], :].sum()) if c in slot_of else 0 for c in classes}
    if not classes or x.numel() == 0:
        return make_table(classes, x.numel(), np.zeros((0, 5)), np.zeros((0, 2)), gt_count)
    L = lib()
    nbytes = L.ct_ws_bytes(D, H, W)
    if nbytes <= 0:
        raise E2EError("ct_ws_bytes: a volume of %d x %d x %d is not supported (more than 2^31 - 2 voxels)" % (D, H, W))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    result = torch.zeros(4, dtype=torch.int64, device=x.device)
    stream = torch.cuda.current_stream().cuda_stream
    words = (ctypes.c_uint * 8)(*_class_words(classes))
    L.ct_label(x.data_ptr(), g.data_ptr(), D, H, W, ctypes.cast(words, ctypes.c_void_p), ws.data_ptr(), result.data_ptr(), stream)
    n_class, n_fg, gave_up, _ = (int(v) for v in result.cpu().numpy())               # (the one read between the two calls)
    if gave_up:
        raise E2EError("ct_label gave up: the union-find met a broken link or spent its step budget")
    class_rec = torch.empty((n_class, 5), dtype=torch.int32, device=x.device)
    fg_rec = torch.empty((n_fg, 2), dtype=torch.int32, device=x.device)
    L.ct_emit(x.data_ptr(), D, H, W, ws.data_ptr(), class_rec.data_ptr(), n_class, n_class, fg_rec.data_ptr(), n_fg, n_fg, stream)
    table = make_table(classes, x.numel(), class_rec.cpu().numpy().view(np.uint32), fg_rec.cpu().numpy().view(np.uint32), gt_count)
    # the census counted the same voxels: a table that disagrees with it is a failed call, not a result
    for c in classes:
        sel = table.label == c
        pos = int(joint[:, slot_of[c]].sum()) if c in slot_of else 0
        hit = int(joint[slot_of[c], slot_of[c]]) if c in slot_of else 0
        if int(table.size[sel].sum()) != pos or int(table.tp[sel].sum()) != hit:
            raise E2EError("component table of class %d: %d voxels and %d true positives, the census counted %d and %d"
                           % (c, int(table.size[sel].sum()), int(table.tp[sel].sum()), pos, hit))
    return table


def _drop(voxels, volume_per_voxel, minimum):
    """the removal rule of remove_all_but_the_largest_connected_component on the objects of one entry: (drop mask, largest removed
    size or None, kept size), sizes ``np.int64 * float`` in fp64; every object of the largest size stays"""
    sizes = np.asarray(voxels, dtype=np.int64) * volume_per_voxel
    biggest = sizes.max()
    drop = sizes != biggest
    if minimum is not None:
        drop &= sizes < minimum
    return drop, (float(sizes[drop].max()) if drop.any() else None), float(biggest)


def counts_after(table, volume_per_voxel, joint=False, joint_min=None, per_class=(), per_class_min=None):
    """The confusion counts a case would have after ``remove_all_but_the_largest_connected_component(pred, entries, volume_per_voxel,
    minima)`` with ``entries = [classes] * joint + list(per_class)``: the joint foreground region first (on the raw prediction), then
    each class of ``per_class`` in order on what is left.  ``joint_min``: the joint entry's minimum valid object size or None;
    ``per_class_min``: class -> minimum, or None; as in the removal, a minimum is looked up only for an entry that has an object.
    Returns ``(counts, largest_removed, kept_size)``: class -> ``(tp, fp, tn, fn)`` for every class of the table, and the two dicts
    of the removal (the joint entry keyed by the tuple of classes).  Bit-equal to removing and counting on the volumes."""
    alive = np.ones(len(table.size), dtype=bool)
    largest_removed, kept_size = {}, {}
    if joint:
        key = tuple(table.classes)
        largest_removed[key] = kept_size[key] = None
        if len(table.fg_size):
            drop, largest_removed[key], kept_size[key] = _drop(table.fg_size, volume_per_voxel, joint_min)
            alive &= ~drop[table.fg]
    for c in per_class:
        c = int(c)
        largest_removed[c] = kept_size[c] = None
        idx = np.nonzero(alive & (table.label == c))[0]
        if len(idx):
            drop, largest_removed[c], kept_size[c] = _drop(table.size[idx], volume_per_voxel,
                                                           None if per_class_min is None else per_class_min[c])
            alive[idx[drop]] = False
    counts = OrderedDict()
    for c in table.classes:
        sel = alive & (table.label == c)
        tp, pos = int(table.tp[sel].sum()), int(table.size[sel].sum())
        fp, fn = pos - tp, table.gt_count[c] - tp
        counts[c] = (tp, fp, table.voxels - tp - fp - fn, fn)
    return counts, largest_removed, kept_size


def search(tables, volumes_per_voxel, classes, dice_threshold=0, advanced_postprocessing=False, names=None, json_files=None):
    """The decision of ``determine_postprocessing`` (reference :167-362) from the cases' tables.  ``names``: per case
    ``(prediction name, ground-truth name)`` for the score records; ``json_files``: ``{"allClasses": path, "perClass": path}`` to
    write the two intermediate summary.json files (the reference's ``debug=True``).  Returns ``pp_results`` as the in-memory search
    builds it up to the final volumes: the three Dice dicts, ``for_which_classes``, ``min_valid_object_sizes`` (a dict or None, not
    yet a string) and ``num_samples``.  The scores go through ``metrics_from_counts`` and ``summarise_scores``, so every mean is the
    float the volume path produces."""
    from ..evaluation.evaluator import metrics_from_counts, summarise_scores
    from .connected_components import _fold_sizes
    classes = [int(c) for c in classes if int(c) != 0]
    key = tuple(classes)
    names = [(None, None)] * len(tables) if names is None else names
    json_files = json_files or {}

    def sweep(joint, joint_mins, per_class=(), per_class_min=None):
        # a minimum is asked for only where the removal would ask: for an entry that has an object in that case
        return [counts_after(t, v, joint, joint_mins[key] if (joint and joint_mins is not None and len(t.fg_size)) else None, per_class,
                             per_class_min) for t, v in zip(tables, volumes_per_voxel)]

    def mean_scores(results, json_output_file=None):
        records = []
        for (counts, _, _), (test_name, ref_name) in zip(results, names):
            res = OrderedDict((str(c), metrics_from_counts(*counts[c])) for c in classes)
            if test_name is not None:
                res["test"] = test_name
            if ref_name is not None:
                res["reference"] = ref_name
            records.append(res)
        return summarise_scores(records, json_output_file=json_output_file, json_author="Fabian")['mean']

    pp_results = OrderedDict()
    pp_results['dc_per_class_raw'] = {}
    pp_results['dc_per_class_pp_all'] = {}
    pp_results['dc_per_class_pp_per_class'] = {}
    pp_results['for_which_classes'] = []
    pp_results['min_valid_object_sizes'] = {}
    pp_results['num_samples'] = len(tables)
    validation_result_raw = mean_scores(sweep(False, None))

    # (1) all foreground classes as one region
    joint_mins = None
    if advanced_postprocessing:
        _, joint_mins = _fold_sizes([r[1:] for r in sweep(True, None)])
        print("foreground vs background, smallest valid object size was", joint_mins.get(key))
        print("removing only objects smaller than that...")
    validation_result_PP_test = mean_scores(sweep(True, joint_mins), json_files.get("allClasses"))
    for c in classes:
        pp_results['dc_per_class_raw'][str(c)] = validation_result_raw[str(c)]['Dice']
        pp_results['dc_per_class_pp_all'][str(c)] = validation_result_PP_test[str(c)]['Dice']
    do_fg_cc = False
    comp = [pp_results['dc_per_class_pp_all'][str(cl)] > (pp_results['dc_per_class_raw'][str(cl)] + dice_threshold) for cl in classes]
    print("Foreground vs background")
    print("before:", np.mean([pp_results['dc_per_class_raw'][str(cl)] for cl in classes]))
    print("after: ", np.mean([pp_results['dc_per_class_pp_all'][str(cl)] for cl in classes]))
    if any(comp):
        any_worse = any(pp_results['dc_per_class_pp_all'][str(cl)] < pp_results['dc_per_class_raw'][str(cl)] for cl in classes)
        if not any_worse:
            pp_results['for_which_classes'].append(classes)
            if joint_mins is not None:
                pp_results['min_valid_object_sizes'].update(deepcopy(joint_mins))
            do_fg_cc = True
            print("Removing all but the largest foreground region improved results!")
            print('for_which_classes', classes)
            print('min_valid_object_sizes', joint_mins)

    # (2) each class separately, on what step 1 chose
    if len(classes) > 1:
        min_size_kept = None
        if advanced_postprocessing:
            # (the joint entry's sizes were folded in step 1: only the classes' own entries count here)
            _, min_size_kept = _fold_sizes([({k: v for k, v in rem.items() if k != key}, {k: v for k, v in kept.items() if k != key})
                                            for _, rem, kept in sweep(do_fg_cc, joint_mins, classes)])
            print("classes treated separately, smallest valid object sizes are")
            print(min_size_kept)
            print("removing only objects smaller than that")
        old_res = deepcopy(validation_result_PP_test) if do_fg_cc else validation_result_raw
        validation_result_PP_test = mean_scores(sweep(do_fg_cc, joint_mins, classes, min_size_kept), json_files.get("perClass"))
        for c in classes:
            dc_raw = old_res[str(c)]['Dice']
            dc_pp = validation_result_PP_test[str(c)]['Dice']
            pp_results['dc_per_class_pp_per_class'][str(c)] = dc_pp
            print(c)
            print("before:", dc_raw)
            print("after: ", dc_pp)
            if dc_pp > (dc_raw + dice_threshold):
                pp_results['for_which_classes'].append(int(c))
                if min_size_kept is not None:
                    pp_results['min_valid_object_sizes'].update({c: min_size_kept[c]})
                print("Removing all but the largest region for class %d improved results!" % c)
                print('min_valid_object_sizes', min_size_kept)
    else:
        print("Only one class present, no need to do each class separately as this is covered in fg vs bg")

    if not advanced_postprocessing:
        pp_results['min_valid_object_sizes'] = None
    print("done")
    print("for which classes:")
    print(pp_results['for_which_classes'])
    print("min_object_sizes")
    print(pp_results['min_valid_object_sizes'])
    return pp_results
