"""Label-map evaluation behind ``nnUNetTrainer_simple.validate``: the reference's ``aggregate_scores`` record
(e2enet/evaluation/evaluator.py:321-400) with its default confusion-matrix metrics (:37-51; formulas and empty-mask rules of
e2enet/evaluation/metrics.py:106-121, :601-790).

Host tooling, not the hot path: the inputs are the exported uint8 label volumes.  One joint histogram of (reference, test)
labels per case replaces the reference's thirteen boolean passes per label; the numbers are the same integers divided the same
way.

``advanced=True`` adds the reference's ``default_advanced_metrics`` (evaluator.py:53-59: "Hausdorff Distance 95", "Avg. Surface
Distance", "Avg. Symmetric Surface Distance") and, with ``nsd_tolerance``, "Normalized Surface Dice" (surface_dice.py:20-56).
Those are computed on the device (``surface_distance.py``, csrc/surface.hip) under the case's ``voxel_spacing``; the empty / full
rule of metrics.py:797-803 is applied from the voxel counts first, so a case without a scorable label needs no device.  With the
defaults the output is the thirteen confusion-matrix metrics, as ``evaluate(advanced=False)`` gives them.
"""
import hashlib
import json
from collections import OrderedDict
from datetime import datetime

import numpy as np

MAX_EVALUATED_VALUES = 63          # e2e_eval_census: 64 slots, one of them for every value nobody evaluates

DEFAULT_METRICS = ["False Positive Rate", "Dice", "Jaccard", "Precision", "Recall", "Accuracy", "False Omission Rate",
                   "Negative Predictive Value", "False Negative Rate", "True Negative Rate", "False Discovery Rate",
                   "Total Positives Test", "Total Positives Reference"]          # evaluator.py:37-51


def confusion_counts(test: np.ndarray, reference: np.ndarray, labels):
    """label -> (tp, fp, tn, fn) of the binary maps ``test == label`` / ``reference == label`` (metrics.py:67-80)."""
    assert test.shape == reference.shape, "Shape mismatch: {} and {}".format(test.shape, reference.shape)
    t = np.asarray(test).reshape(-1).astype(np.int64)
    r = np.asarray(reference).reshape(-1).astype(np.int64)
    lo = int(min(t.min(), r.min(), 0)) if t.size else 0
    n = int(max(t.max(), r.max(), max(int(l) for l in labels))) - lo + 1 if t.size else 1
    joint = np.bincount((r - lo) * n + (t - lo), minlength=n * n).reshape(n, n)      # [reference, test]
    size = int(t.size)
    out = OrderedDict()
    for l in labels:
        i = int(l) - lo
        tp = int(joint[i, i]) if 0 <= i < n else 0
        pos_t = int(joint[:, i].sum()) if 0 <= i < n else 0
        pos_r = int(joint[i, :].sum()) if 0 <= i < n else 0
        fp, fn = pos_t - tp, pos_r - tp
        out[l] = (tp, fp, size - tp - fp - fn, fn)
    return out


def metrics_from_counts(tp, fp, tn, fn, nan_for_nonexisting=True):
    """The thirteen default metrics of one binary pair, keyed and SORTED like the reference's result dicts
    (``self.metrics.sort()``, evaluator.py:166).  Empty / full rules: metrics.py:106-121, :601-790."""
    nan = float("NaN") if nan_for_nonexisting else 0.
    size = tp + fp + tn + fn
    test_empty, test_full = (tp + fp) == 0, (tp + fp) == size
    ref_empty, ref_full = (tp + fn) == 0, (tp + fn) == size
    dice = nan if (test_empty and ref_empty) else float(2. * tp / (2 * tp + fp + fn))
    jaccard = nan if (test_empty and ref_empty) else float(tp / (tp + fp + fn))
    precision = nan if test_empty else float(tp / (tp + fp))
    sensitivity = nan if ref_empty else float(tp / (tp + fn))
    specificity = nan if ref_full else float(tn / (tn + fp))
    fomr = nan if test_full else float(fn / (fn + tn))
    res = {"False Positive Rate": 1 - specificity, "Dice": dice, "Jaccard": jaccard, "Precision": precision,
           "Recall": sensitivity, "Accuracy": float((tp + tn) / (tp + fp + tn + fn)), "False Omission Rate": fomr,
           "Negative Predictive Value": 1 - fomr, "False Negative Rate": 1 - sensitivity, "True Negative Rate": specificity,
           "False Discovery Rate": 1 - precision, "Total Positives Test": tp + fp, "Total Positives Reference": tp + fn}
    return OrderedDict((k, res[k]) for k in sorted(res))


def evaluate_pair(test: np.ndarray, reference: np.ndarray, labels, nan_for_nonexisting=True, advanced=False, voxel_spacing=None,
                  nsd_tolerance=None):
    """label (str) -> metric dict: ``Evaluator.evaluate`` for a list of integer labels (evaluator.py:216-226).  ``advanced``: the
    surface-distance metrics under ``voxel_spacing`` (array-axis order, None = 1 mm) join each dict, keys sorted as before."""
    counts = confusion_counts(test, reference, labels)
    res = OrderedDict((str(l), metrics_from_counts(*counts[l], nan_for_nonexisting)) for l in labels)
    if advanced:
        from .surface_distance import surface_distance_metrics, ADVANCED_METRICS, NSD_KEY
        surf = surface_distance_metrics(test, reference, labels, voxel_spacing, nsd_tolerance, nan_for_nonexisting)
        names = ADVANCED_METRICS + ((NSD_KEY,) if nsd_tolerance is not None else ())
        for l in labels:
            d = dict(res[str(l)])
            d.update((k, surf[int(l)][k]) for k in names)
            res[str(l)] = OrderedDict((k, d[k]) for k in sorted(d))
    return res


def aggregate_scores(cases, labels, nanmean=True, json_output_file=None, json_name="", json_description="",
                     json_author="Fabian", json_task="", advanced=False, voxel_spacing=None, nsd_tolerance=None):
    """``cases``: iterable of (test array, reference array, test name, reference name[, voxel spacing]).  Returns the reference's
    ``all_scores`` ({"all": [per case], "mean": {label: {metric: mean}}}) and writes the reference's summary.json
    (evaluator.py:353-400) when ``json_output_file`` is given.  ``advanced``: see ``evaluate_pair``; a case's own fifth element
    overrides ``voxel_spacing``, and the case's entry records the spacing it was scored with under "voxel_spacing"."""
    results = []
    for case in cases:
        test, ref, test_name, ref_name = case[:4]
        if advanced:
            spacing = case[4] if len(case) > 4 and case[4] is not None else voxel_spacing
            spacing = [1., 1., 1.] if spacing is None else [float(v) for v in spacing]
            res = evaluate_pair(test, ref, labels, advanced=True, voxel_spacing=spacing, nsd_tolerance=nsd_tolerance)
            res["voxel_spacing"] = spacing
        else:
            res = evaluate_pair(test, ref, labels)
        if test_name is not None:
            res["test"] = test_name
        if ref_name is not None:
            res["reference"] = ref_name
        results.append(res)
    return summarise_scores(results, nanmean, json_output_file, json_name, json_description, json_author, json_task)


def summarise_scores(results, nanmean=True, json_output_file=None, json_name="", json_description="", json_author="Fabian",
                     json_task=""):
    """The second half of the reference's ``aggregate_scores`` (evaluator.py:366-400): ``results`` (one dict per case, as
    ``evaluate_pair`` returns it plus "test" / "reference" / "voxel_spacing") -> ``all_scores`` with the per-label means, and the
    summary.json when a file name is given."""
    all_scores = OrderedDict()
    all_scores["all"] = []
    all_scores["mean"] = OrderedDict()
    for res in results:
        all_scores["all"].append(res)
        for label, score_dict in res.items():
            if label in ("test", "reference", "voxel_spacing"):
                continue
            dst = all_scores["mean"].setdefault(label, OrderedDict())
            for score, value in score_dict.items():
                dst.setdefault(score, []).append(value)
    for label in all_scores["mean"]:
        for score in all_scores["mean"][label]:
            vals = all_scores["mean"][label][score]
            with np.errstate(all="ignore"):
                import warnings
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore", RuntimeWarning)          # (all-NaN slice: the reference prints the warning)
                    all_scores["mean"][label][score] = float(np.nanmean(vals)) if nanmean else float(np.mean(vals))
    if json_output_file is not None:
        json_dict = OrderedDict()
        json_dict["name"] = json_name
        json_dict["description"] = json_description
        json_dict["timestamp"] = str(datetime.today())
        json_dict["task"] = json_task
        json_dict["author"] = json_author
        json_dict["results"] = all_scores
        json_dict["id"] = hashlib.md5(json.dumps(json_dict).encode("utf-8")).hexdigest()[:12]
        with open(json_output_file, "w") as f:
            json.dump(json_dict, f, indent=4, sort_keys=True)            # (batchgenerators save_json: indent 4, sorted keys)
    return all_scores


# ---- the device path: one census pass per case (csrc/evaluate.hip) ------------------------------------------------------------
def label_entries(labels):
    """labels in any of the reference's forms (``Evaluator.set_labels``) -> [(result key, int label or tuple of ints)]"""
    def one(l):
        if hasattr(l, "__iter__") and not isinstance(l, (str, bytes)):
            return tuple(int(v) for v in l)
        return int(l)
    if isinstance(labels, dict):
        return [(str(name), one(l)) for l, name in labels.items()]
    if isinstance(labels, (list, tuple, set, frozenset, np.ndarray)):
        return [(str(l), int(l)) for l in labels]
    raise TypeError("Can only handle dict, list, tuple, set & numpy array, but input is of type {}".format(type(labels)))


def _evaluated_values(entries):
    """the distinct uint8 values the entries name (a value outside [0, 255] occurs in no volume and needs no slot)"""
    vals = set()
    for _, l in entries:
        vals.update(l if isinstance(l, tuple) else (l,))
    vals = sorted(v for v in vals if 0 <= v <= 255)
    if len(vals) > MAX_EVALUATED_VALUES:
        raise ValueError("%d distinct label values to evaluate: the device census holds at most %d per call"
                         % (len(vals), MAX_EVALUATED_VALUES))
    return vals


def _census_call(test, reference, lut, slots):
    """one e2e_eval_census over two device uint8 tensors -> (joint int64 [slots, slots], boxes int [slots, 6]) on the host"""
    import ctypes
    import torch
    from .._lib import lib
    D, H, W = (int(v) for v in test.shape)
    joint = torch.empty(slots * slots, dtype=torch.int64, device=test.device)
    boxes = torch.empty(slots * 6, dtype=torch.int32, device=test.device)
    lib().eval_census(test.data_ptr(), reference.data_ptr(), (ctypes.c_ubyte * 256)(*lut), slots, D, H, W, joint.data_ptr(),
                      boxes.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return joint.cpu().numpy().reshape(slots, slots), boxes.cpu().numpy().reshape(slots, 6)


def _device_pair(test, reference):
    """both label volumes as contiguous device uint8 tensors of one shape (host arrays are uploaded, device tensors used as they are)"""
    import torch
    from .surface_distance import _label_volume
    test, reference = _label_volume(test, "test"), _label_volume(reference, "reference")
    if tuple(test.shape) != tuple(reference.shape):
        raise ValueError("Shape mismatch: {} and {}".format(tuple(test.shape), tuple(reference.shape)))
    if not torch.cuda.is_available():
        raise RuntimeError("the label census runs on the GPU (csrc/evaluate.hip); there is no host fallback")
    # (np.array: a contiguous copy torch may wrap whatever the caller's array allows)
    up = lambda x: (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.array(x, order="C"))).to("cuda").contiguous()
    return up(test), up(reference)


def label_census(test, reference, labels=None):
    """One device pass over both label volumes of a case (two for ``labels=None`` when a value above 62 is present).
    ``labels``: the integer values to tell apart (at most 63), or None for every value present.  Returns
      joint    int64 [slots, slots]: voxels per (reference slot, test slot);
      slot_of  value -> slot; every other value shares the last slot, ``slots - 1``;
      boxes    value -> three slices around the voxels that carry it in either volume (``label_boxes``), present values only.
    Host arrays are uploaded once; device uint8 tensors are read where they are."""
    values = None if labels is None else _evaluated_values([(None, int(l)) for l in labels])
    return _census(*_device_pair(test, reference), values)


def _census(test, reference, values):
    if test.numel() == 0:
        values = values or []
        return np.zeros((len(values) + 1,) * 2, np.int64), {v: i for i, v in enumerate(values)}, {}
    done = None
    if values is None:
        # values 0..62 get a slot each; when nothing else is present (the last slot stays empty) that pass is the census
        first = _census_call(test, reference, [min(v, 63) for v in range(256)], 64)
        occupied = lambda j, k: bool(j[k, :].sum() or j[:, k].sum())
        if not occupied(first[0], 63):
            values, done = list(range(63)), first
        else:
            values = [v for v in range(63) if occupied(first[0], v)]
            for base in range(63, 256, 63):
                j, _ = _census_call(test, reference, [v - base if base <= v < base + 63 else 63 for v in range(256)], 64)
                values += [base + k for k in range(min(63, 256 - base)) if occupied(j, k)]
            if len(values) > MAX_EVALUATED_VALUES:
                raise ValueError("%d distinct label values are present: the device census holds at most %d per call"
                                 % (len(values), MAX_EVALUATED_VALUES))
    slot_of = {v: i for i, v in enumerate(values)}
    slots = len(values) + 1
    joint, raw = done if done is not None else _census_call(test, reference, [slot_of.get(v, slots - 1) for v in range(256)], slots)
    boxes = {v: tuple(slice(int(raw[i, a]), int(raw[i, 3 + a])) for a in range(3)) for v, i in slot_of.items() if raw[i, 0] < raw[i, 3]}
    return joint, slot_of, boxes


def counts_from_joint(joint, slot_of, label):
    """(tp, fp, tn, fn) of the binary maps "value is ``label``" (an int) or "value is one of ``label``" (a tuple) from a joint table
    [reference slot, test slot]; a value without a slot occurs in neither volume"""
    members = label if isinstance(label, (tuple, list, set, frozenset, np.ndarray)) else (label,)
    idx = sorted({slot_of[int(m)] for m in members if int(m) in slot_of})
    joint = np.asarray(joint)
    size = int(joint.sum())
    tp = int(joint[np.ix_(idx, idx)].sum())
    fp = int(joint[:, idx].sum()) - tp
    fn = int(joint[idx, :].sum()) - tp
    return tp, fp, size - tp - fp - fn, fn


def evaluate_pair_device(test, reference, labels, nan_for_nonexisting=True, advanced=False, voxel_spacing=None, nsd_tolerance=None):
    """``evaluate_pair`` with the counting and the boxes done on the device: result key -> metric dict, the same numbers.
    ``labels``: a list, tuple, set or array of ints (keys ``str(label)``); a dict ``label -> name`` whose keys may be tuples of
    ints -- regions, scored as the mask "value is in the tuple" -- keyed by ``str(name)`` (the reference's ``Evaluator.evaluate``);
    or None for every value present in either volume (``construct_labels``).  Both volumes are uploaded once (device uint8 tensors
    are used where they are); one ``e2e_eval_census`` pass gives the joint table every confusion count comes from and the label
    boxes the surface metrics of ``advanced=True`` are scored in.  More than 63 distinct values: ValueError, no host fallback."""
    from .surface_distance import _spacing, SurfaceScorer, ADVANCED_METRICS, NSD_KEY
    entries = None if labels is None else label_entries(labels)
    values = None if entries is None else _evaluated_values(entries)
    spacing = _spacing(voxel_spacing) if advanced else None
    test, reference = _device_pair(test, reference)
    joint, slot_of, boxes = _census(test, reference, values)
    if entries is None:
        present = sorted(v for v, i in slot_of.items() if joint[i, :].sum() or joint[:, i].sum())
        entries = [(str(v), v) for v in present]
    size = int(joint.sum())
    nan = float("NaN") if nan_for_nonexisting else 0.
    names = ADVANCED_METRICS + ((NSD_KEY,) if nsd_tolerance is not None else ())
    scorer, res = None, OrderedDict()
    for key, label in entries:
        tp, fp, tn, fn = counts_from_joint(joint, slot_of, label)
        res[key] = metrics_from_counts(tp, fp, tn, fn, nan_for_nonexisting)
        if not advanced:
            continue
        d = dict(res[key])
        if size == 0 or tp + fp in (0, size) or tp + fn in (0, size):           # metrics.py:797-803, from the counts
            d.update((k, nan) for k in names)
        else:
            if scorer is None:
                scorer = SurfaceScorer(test, reference, spacing, boxes=boxes)
            m = scorer.metrics(label, nsd_tolerance)
            d.update((k, m[k]) for k in names)
        res[key] = OrderedDict((k, d[k]) for k in sorted(d))
    return res
