"""The reference's only post-processing, "remove all but the largest connected component" (e2enet/postprocessing/
connected_components.py), with the labelling on the device (csrc/components.hip) instead of one ``scipy.ndimage.label`` over the
whole volume per class entry plus one ``(lmap == id).sum()`` per object.

  remove_all_but_the_largest_connected_component   :50-107, same name, arguments and return value
  load_postprocessing                              :110-121
  determine_postprocessing                         :124-399, the same search on the in-memory cases ``validate()`` holds (no
                                                   temp folders, no NIfTI round trips, no worker pool); called with a folder
                                                   name, the reference's folder form: one component table per case
                                                   (component_table.py) instead of one removed volume per case and sweep
  apply_postprocessing                             what ``load_remove_save`` (:32-47) does to one volume
  apply_postprocessing_to_folder                   :402-423

The label volume is uploaded once per call; a class entry's mask is formed on load from a 256-bit class set, so a joint region such
as (1, 2, 3) needs no mask volume.  Sizes are ``voxels * volume_per_voxel`` in fp64, which is numpy's ``int64 * float``.  There is
no host fallback: without the library or a device the removal raises.
"""
import ast
import json
import os
from collections import OrderedDict
from copy import deepcopy

import numpy as np


def _entry_key(c):
    """a ``for_which_classes`` entry as (dict key, tuple of member classes): a list / tuple is a joint region keyed by its tuple"""
    if isinstance(c, (list, tuple)):
        key = tuple(int(v) for v in c)
        return key, key
    return int(c), (int(c),)


def _class_words(members):
    words = [0] * 8
    for v in members:
        if not 0 <= v <= 255:
            raise ValueError("class %r is outside a uint8 label volume's range" % (v,))
        words[v >> 5] |= 1 << (v & 31)
    return words


def remove_all_but_the_largest_connected_component(image, for_which_classes, volume_per_voxel, minimum_valid_object_size=None):
    """Reference :50-107.  For every entry of ``for_which_classes``, in order and on the volume the earlier entries left: label the
    6-connected components of the entry's mask and set to 0 every component that is not of the largest size (and, when
    ``minimum_valid_object_size`` is given, whose size is below ``minimum_valid_object_size[entry]``).  All components of the largest
    size stay.

    ``image``: a 3-D label volume, either a numpy array with whole-number labels in [0, 255] (edited in place like the reference's,
    and returned) or a contiguous device uint8 tensor (edited in place and returned, never downloaded).  An entry is an int or a
    list / tuple of ints (a joint region; its dict key is the tuple); ``None`` means every label > 0 the volume holds, ascending.
    Returns ``(image, largest_removed, kept_size)``: per entry the largest removed and the kept size in ``volume_per_voxel`` units,
    or None when nothing was removed / the entry has no object."""
    import ctypes
    import torch
    from .._lib import lib, E2EError
    from ..evaluation.surface_distance import _label_volume, _voxel_counts
    vol = _label_volume(image, "image")
    counts = _voxel_counts(vol)
    if for_which_classes is None:
        for_which_classes = [int(v) for v in np.nonzero(counts)[0] if v > 0]
    entries = [_entry_key(c) for c in for_which_classes]
    assert all(0 not in members for _, members in entries), "cannot remove background"
    largest_removed = {key: None for key, _ in entries}
    kept_size = {key: None for key, _ in entries}
    # an entry none of whose classes the volume holds has no object: nothing to launch (and, like the reference, its minimum is
    # never looked up)
    entries = [(key, members) for key, members in entries if sum(int(counts[v]) for v in set(members) if 0 <= v <= 255) > 0]
    if not entries:
        return image, largest_removed, kept_size
    if not torch.cuda.is_available():
        raise RuntimeError("connected-component post-processing runs on the GPU (csrc/components.hip); there is no host fallback")
    vpv = float(volume_per_voxel)
    L = lib()
    dev = torch.device("cuda")
    if isinstance(vol, torch.Tensor):
        if not (vol.is_cuda and vol.is_contiguous()):
            raise ValueError("image: a tensor label volume must be a contiguous device tensor")
        work = vol
    else:
        work = torch.from_numpy(np.array(vol, order="C")).to(dev)
    D, H, W = (int(v) for v in work.shape)
    nbytes = L.cc_ws_bytes(D, H, W)
    if nbytes <= 0:
        raise E2EError("cc_ws_bytes: a volume of %d x %d x %d is not supported (more than 2^31 - 2 voxels)" % (D, H, W))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    result = torch.zeros((len(entries), 4), dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    for n, (key, members) in enumerate(entries):
        minimum = -1.0
        if minimum_valid_object_size is not None:
            minimum = max(float(minimum_valid_object_size[key]), 0.0)        # (no size is below a negative minimum either)
        words = (ctypes.c_uint * 8)(*_class_words(members))
        L.cc_remove_all_but_largest(work.data_ptr(), D, H, W, ctypes.cast(words, ctypes.c_void_p), vpv, minimum, ws.data_ptr(),
                                    result[n].data_ptr(), stream)
    res = result.cpu().numpy()                                               # (the one read: every entry's result words)
    if res[:, 3].any():
        raise E2EError("cc_remove_all_but_largest gave up on entry %r: the union-find met a broken link or spent its step budget"
                       % (entries[int(np.nonzero(res[:, 3])[0][0])][0],))
    for (key, _), (objects, largest, removed, _) in zip(entries, res):
        kept_size[key] = float(np.int64(largest) * vpv) if objects > 0 else None
        largest_removed[key] = float(np.int64(removed) * vpv) if removed > 0 else None
    if work is not vol:
        out = work.cpu().numpy()
        if isinstance(image, np.ndarray) and image.flags.writeable:
            image[...] = out.reshape(image.shape)
        else:
            image = out
    return image, largest_removed, kept_size


def load_postprocessing(json_file):
    """Reference :110-121: ``(for_which_classes, min_valid_object_sizes or None)`` of a postprocessing.json"""
    with open(json_file, 'r') as f:
        a = json.load(f)
    if 'min_valid_object_sizes' in a.keys():
        min_valid_object_sizes = ast.literal_eval(a['min_valid_object_sizes'])
    else:
        min_valid_object_sizes = None
    return a['for_which_classes'], min_valid_object_sizes


def volume_per_voxel_of(spacing):
    """product of a case's voxel spacing given in array-axis order (z, y, x), multiplied in the (x, y, z) order of the reference's
    ``np.prod(img.GetSpacing())`` (:38) so that the two agree to the bit; no spacing: 1"""
    if spacing is None:
        return 1.0
    return float(np.prod([float(v) for v in spacing][::-1], dtype=np.float64))


def apply_postprocessing(seg, for_which_classes, min_valid_object_sizes, volume_per_voxel):
    """The stored decision applied to one label volume (host array or device uint8 tensor); returns the volume."""
    return remove_all_but_the_largest_connected_component(seg, for_which_classes, volume_per_voxel, min_valid_object_sizes)[0]


def _fold_sizes(results):
    """(max removed, min kept) per entry over the cases' dicts (reference :191-207)"""
    max_size_removed, min_size_kept = {}, {}
    for mx_rem, min_kept in results:
        for k in mx_rem:
            if mx_rem[k] is not None:
                max_size_removed[k] = mx_rem[k] if max_size_removed.get(k) is None else max(max_size_removed[k], mx_rem[k])
        for k in min_kept:
            if min_kept[k] is not None:
                min_size_kept[k] = min_kept[k] if min_size_kept.get(k) is None else min(min_size_kept[k], min_kept[k])
    return max_size_removed, min_size_kept


def determine_postprocessing(*args, **kwargs):
    """Reference :124-399, in two forms told apart by the first argument.

    A folder name (``str``): the reference's own signature, ``determine_postprocessing(base, gt_labels_folder, raw_subfolder_name=
    "validation_raw", temp_folder="temp", final_subf_name="validation_final", processes=8, dice_threshold=0, debug=False,
    advanced_postprocessing=False, pp_filename="postprocessing.json", reader=None, writer=None)``: the search over the label files of
    ``<base>/<raw_subfolder_name>``, from one component table per case (``determine_postprocessing_folder``).

    A list of cases: ``determine_postprocessing(cases, classes, base, ...)``, the search on the volumes ``validate()`` holds in
    memory (``determine_postprocessing_in_memory``), unchanged."""
    first = args[0] if args else kwargs.get("cases", kwargs.get("base"))
    if isinstance(first, str):
        return determine_postprocessing_folder(*args, **kwargs)
    return determine_postprocessing_in_memory(*args, **kwargs)


def determine_postprocessing_in_memory(cases, classes, base, raw_subfolder_name="validation_raw", final_subf_name="validation_final",
                                       dice_threshold=0, advanced_postprocessing=False, pp_filename="postprocessing.json", writer=None,
                                       remove=None):
    """Reference :124-399 on in-memory cases: decide for which classes removing all but the largest component improves the mean
    Dice, apply that decision to every case, and record it.

    ``cases``: the ``(seg, gt, out_path, gt_path, spacing)`` tuples of the raw predictions (``spacing`` in array-axis order or
    None); ``classes``: the foreground classes.  The search: (1) all foreground classes as one region; kept only if some class's
    mean Dice improves by more than ``dice_threshold`` and none gets worse; (2) with more than one class, each class separately on
    the volumes step 1 chose, a class is kept when its mean Dice improves by more than ``dice_threshold``; with
    ``advanced_postprocessing`` each step first runs without a minimum and then again removing only objects smaller than the
    smallest object it kept in any case.  Writes ``<base>/<pp_filename>`` with the reference's keys and
    ``<base>/<final_subf_name>/summary.json``; every final volume goes to ``writer(seg, path, case_index)`` with ``path`` the
    case's file name under the final folder.  ``remove``: the removal function (default: the device one above).
    Returns ``(pp_results, final_volumes)``."""
    from ..evaluation.evaluator import aggregate_scores
    remove = remove_all_but_the_largest_connected_component if remove is None else remove
    classes = [int(c) for c in classes if int(c) != 0]
    cases = [tuple(c) + (None,) * (5 - len(c)) for c in cases]
    vpv = [volume_per_voxel_of(c[4]) for c in cases]
    final_folder = os.path.join(base, final_subf_name)
    os.makedirs(final_folder, exist_ok=True)

    def run(sources, for_which_classes, min_sizes):
        out, dicts = [], []
        for src, v in zip(sources, vpv):
            img, removed, kept = remove(np.array(src), for_which_classes, v, min_sizes)
            out.append(img)
            dicts.append((removed, kept))
        return out, dicts

    def mean_scores(volumes, json_output_file=None):
        return aggregate_scores([(vol, c[1], c[2], c[3]) for vol, c in zip(volumes, cases)], labels=classes,
                                json_output_file=json_output_file, json_author="Fabian")['mean']

    pp_results = OrderedDict()
    pp_results['dc_per_class_raw'] = {}
    pp_results['dc_per_class_pp_all'] = {}            # dice scores after treating all foreground classes as one
    pp_results['dc_per_class_pp_per_class'] = {}      # dice scores after removing all but the largest component per class, after pp_all
    pp_results['for_which_classes'] = []
    pp_results['min_valid_object_sizes'] = {}
    pp_results['num_samples'] = len(cases)
    raw = [c[0] for c in cases]
    validation_result_raw = mean_scores(raw)

    # (1) all foreground classes as one region
    min_size_kept = None
    if advanced_postprocessing:
        _, min_size_kept = _fold_sizes(run(raw, (classes,), None)[1])
        print("foreground vs background, smallest valid object size was", min_size_kept.get(tuple(classes)))
        print("removing only objects smaller than that...")
    pp_all, _ = run(raw, (classes,), min_size_kept)
    validation_result_PP_test = mean_scores(pp_all)
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
            if min_size_kept is not None:
                pp_results['min_valid_object_sizes'].update(deepcopy(min_size_kept))
            do_fg_cc = True
            print("Removing all but the largest foreground region improved results!")
            print('for_which_classes', classes)
            print('min_valid_object_sizes', min_size_kept)

    # (2) each class separately, on the volumes step 1 chose
    if len(classes) > 1:
        source = pp_all if do_fg_cc else raw
        min_size_kept = None
        if advanced_postprocessing:
            _, min_size_kept = _fold_sizes(run(source, classes, None)[1])
            print("classes treated separately, smallest valid object sizes are")
            print(min_size_kept)
            print("removing only objects smaller than that")
        per_class, _ = run(source, classes, min_size_kept)
        old_res = deepcopy(validation_result_PP_test) if do_fg_cc else validation_result_raw
        validation_result_PP_test = mean_scores(per_class)
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
    pp_results['validation_raw'] = raw_subfolder_name
    pp_results['validation_final'] = final_subf_name

    # the decision applied to the raw predictions
    final, _ = run(raw, pp_results['for_which_classes'], pp_results['min_valid_object_sizes'])
    paths = [os.path.join(final_folder, os.path.basename(c[2])) if c[2] is not None else None for c in cases]
    aggregate_scores([(vol, c[1], p, c[3]) for vol, c, p in zip(final, cases, paths)], labels=classes,
                     json_output_file=os.path.join(final_folder, "summary.json"), json_author="Fabian")
    if writer is not None:
        for i, (vol, p) in enumerate(zip(final, paths)):
            writer(vol, p, i)
    pp_results['min_valid_object_sizes'] = str(pp_results['min_valid_object_sizes'])
    with open(os.path.join(base, pp_filename), 'w') as f:
        json.dump(pp_results, f, sort_keys=True, indent=4)
    print("done")
    return pp_results, final


# ---- the folder forms: label files in, label files out -------------------------------------------------------------------------
def default_reader(path):
    """``reader(path) -> (volume, properties or None)`` of the folder functions.  ``.npy`` is read natively and has no geometry
    (``volume_per_voxel`` 1); everything else goes through SimpleITK, the geometry under the reference's ``itk_*`` keys."""
    if path.endswith(".npy"):
        return np.load(path), None
    try:
        import SimpleITK as sitk
    except ImportError:
        raise ImportError("reading %s needs SimpleITK (only .npy volumes are read without it): pass reader=native_reader and "
                          "writer=nifti.writer, or --native_nifti on the command line" % path)
    img = sitk.ReadImage(path)
    return sitk.GetArrayFromImage(img), {'itk_spacing': img.GetSpacing(), 'itk_origin': img.GetOrigin(), 'itk_direction': img.GetDirection()}


def native_reader(path, inflate="host"):
    """``default_reader`` with this package's own NIfTI-1 code: the host half (header and gzip; safe in a read-ahead thread) returns
    the ``nifti.NiftiRaw``, which the thread that owns the GPU decodes to a device uint8 tensor"""
    from .. import nifti
    if path.endswith(".npy"):
        return np.load(path), None
    raw = nifti.read_raw(path, inflate)                # ("device": the payload is inflated on the GPU when it is decoded)
    return raw, nifti.properties_of(raw)


def default_writer(seg, path, properties):
    """``writer(seg_uint8, path, properties)``: ``.npy`` natively, everything else through SimpleITK with the input file's geometry"""
    if path.endswith(".npy"):
        np.save(path, seg)
        return
    try:
        import SimpleITK as sitk
    except ImportError:
        raise ImportError("writing %s needs SimpleITK: pass writer=nifti.writer, or --native_nifti on the command line" % path)
    img = sitk.GetImageFromArray(np.asarray(seg).astype(np.uint8))
    if properties is not None:
        img.SetSpacing(properties['itk_spacing'])
        img.SetOrigin(properties['itk_origin'])
        img.SetDirection(properties['itk_direction'])
    sitk.WriteImage(img, path)


def label_files(folder):
    """the label files of a folder, sorted: ``.nii.gz``, or ``.npy`` when the folder holds no ``.nii.gz`` (``pair_files``' rule)"""
    files = sorted(f for f in os.listdir(folder) if os.path.isfile(os.path.join(folder, f)))
    suffix = ".nii.gz" if any(f.endswith(".nii.gz") for f in files) else ".npy"
    return [f for f in files if f.endswith(suffix)]


def _volume_per_voxel(properties):
    """reference :38, ``np.prod(img.GetSpacing())``; a file without geometry: 1"""
    if properties is None or properties.get('itk_spacing') is None:
        return 1.0
    return float(np.prod(properties['itk_spacing'], dtype=np.float64))


def _cases_of(pairs, reader, num_threads, on_device):
    """yields ``(prediction, ground truth or None, properties of the prediction)`` per pair of file names, read ``num_threads`` files
    ahead; ``on_device``: a pair comes as two device uint8 tensors of one shape, each uploaded once"""
    from ..evaluator import _read_ahead, _decoded
    from ..evaluation.evaluator import _device_pair
    for _, _, (pred, properties), gt in _read_ahead(pairs, reader, num_threads):
        pred, gt = _decoded(pred), (None if gt is None else _decoded(gt[0]))
        if on_device and gt is not None:
            pred, gt = _device_pair(pred, gt)
        yield pred, gt, properties


def _host_u8(seg):
    return seg.cpu().numpy() if hasattr(seg, "cpu") else np.asarray(seg)


def determine_postprocessing_folder(base, gt_labels_folder, raw_subfolder_name="validation_raw", temp_folder="temp",
                                    final_subf_name="validation_final", processes=8, dice_threshold=0, debug=False,
                                    advanced_postprocessing=False, pp_filename="postprocessing.json", reader=None, writer=None,
                                    table=None, remove=None):
    """Reference :124-399 on folders, with the reference's arguments: decide from the raw predictions in
    ``<base>/<raw_subfolder_name>`` and the ground truths of the same names in ``gt_labels_folder`` for which classes removing all
    but the largest component improves the mean Dice, apply the decision to every raw prediction, and record it.

    The classes and ``num_samples`` come from ``<base>/<raw_subfolder_name>/summary.json``.  Every file is read twice and no
    intermediate volume is written: the first pass (``processes`` host threads read ahead of the device) builds one component table
    per case (``component_table``), the search is arithmetic on the tables (``component_table.search``), the second pass applies
    the decision with the device removal and writes ``<base>/<final_subf_name>/<name>`` through ``writer(seg, path, properties)``
    with the input file's geometry, scored into ``<base>/<final_subf_name>/summary.json``.  ``<base>/<pp_filename>`` has the
    reference's keys.  ``debug``: the two intermediate summary.json files stay, in ``<base>/<temp_folder>_allClasses`` and
    ``<base>/<temp_folder>_perClass``.

    ``reader(path) -> (volume, properties or None)``: default ``default_reader``; ``native_reader`` with ``writer=nifti.writer`` reads
    and writes ``.nii.gz`` without SimpleITK.  ``table(pred, gt, classes)`` and ``remove``: the table builder and the removal
    (defaults: the device ones); with a ``table`` of the caller's the volumes stay where the reader put them and are scored on the
    host.  Returns ``pp_results``."""
    import shutil
    from .component_table import component_table, search
    from ..evaluation.evaluator import evaluate_pair, evaluate_pair_device, summarise_scores
    raw_folder, final_folder = os.path.join(base, raw_subfolder_name), os.path.join(base, final_subf_name)
    assert os.path.isfile(os.path.join(raw_folder, "summary.json")), "join(base, raw_subfolder_name) does not contain a summary.json"
    with open(os.path.join(raw_folder, "summary.json"), 'r') as f:
        summary = json.load(f)['results']
    classes = [int(i) for i in summary['mean'].keys() if int(i) != 0]
    on_device = table is None
    table = component_table if table is None else table
    remove = remove_all_but_the_largest_connected_component if remove is None else remove
    reader = default_reader if reader is None else reader
    writer = default_writer if writer is None else writer
    fnames = label_files(raw_folder)
    pairs = [(os.path.join(raw_folder, f), os.path.join(gt_labels_folder, f)) for f in fnames]
    missing = [g for _, g in pairs if not os.path.isfile(g)]
    if missing:
        raise FileNotFoundError("%d ground-truth file(s) missing: %s" % (len(missing), ", ".join(missing)))
    temp = {"allClasses": os.path.join(base, temp_folder + "_allClasses"), "perClass": os.path.join(base, temp_folder + "_perClass")}
    for folder in temp.values():
        if os.path.isdir(folder):
            shutil.rmtree(folder)
        if debug:
            os.makedirs(folder)
    os.makedirs(final_folder, exist_ok=True)

    tables, vpv = [], []
    for pred, gt, properties in _cases_of(pairs, reader, processes, on_device):
        tables.append(table(pred, gt, classes))
        vpv.append(_volume_per_voxel(properties))
    pp_results = search(tables, vpv, classes, dice_threshold, advanced_postprocessing,
                        names=pairs,                # (the raw file: the volume a record stands for is never written)
                        json_files={k: os.path.join(v, "summary.json") for k, v in temp.items()} if debug else None)
    pp_results['num_samples'] = len(summary['all'])
    pp_results['validation_raw'] = raw_subfolder_name
    pp_results['validation_final'] = final_subf_name

    # the decision applied to the raw predictions
    records = []
    cases = _cases_of(pairs, reader, processes, on_device)
    for f, (_, gt_name), v, (pred, gt, properties) in zip(fnames, pairs, vpv, cases):
        final = remove(pred, pp_results['for_which_classes'], v, pp_results['min_valid_object_sizes'])[0]
        res = (evaluate_pair_device if on_device else evaluate_pair)(final, gt, classes)
        res["test"], res["reference"] = os.path.join(final_folder, f), gt_name
        records.append(res)
        writer(_host_u8(final), os.path.join(final_folder, f), properties)
    summarise_scores(records, json_output_file=os.path.join(final_folder, "summary.json"), json_author="Fabian")
    pp_results['min_valid_object_sizes'] = str(pp_results['min_valid_object_sizes'])
    with open(os.path.join(base, pp_filename), 'w') as f:
        json.dump(pp_results, f, sort_keys=True, indent=4)
    print("done")
    return pp_results


def apply_postprocessing_to_folder(input_folder, output_folder, for_which_classes, min_valid_object_size=None, num_processes=8,
                                   reader=None, writer=None, remove=None):
    """Reference :402-423: the removal applied to every label file of ``input_folder``, written under the same name into
    ``output_folder`` with the input file's geometry.  ``num_processes`` host threads read ahead of the device; ``reader``,
    ``writer``, ``remove`` as in ``determine_postprocessing_folder``."""
    remove = remove_all_but_the_largest_connected_component if remove is None else remove
    reader = default_reader if reader is None else reader
    writer = default_writer if writer is None else writer
    os.makedirs(output_folder, exist_ok=True)
    fnames = label_files(input_folder)
    cases = _cases_of([(os.path.join(input_folder, f), None) for f in fnames], reader, num_processes, False)
    for f, (seg, _, properties) in zip(fnames, cases):
        seg = remove(seg, for_which_classes, _volume_per_voxel(properties), min_valid_object_size)[0]
        writer(_host_u8(seg), os.path.join(output_folder, f), properties)
