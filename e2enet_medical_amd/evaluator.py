"""Evaluate a folder of predictions against a folder of ground truths: the reference's top-level ``evaluator.py``
(``python evaluator.py -ref <labels folder> -pred <output folder> -l 1 2 ...``) with the counting done on the device.

   python -m e2enet_medical_amd.evaluator -ref DIR -pred DIR -l 1 2 [--advanced] [--nsd_tolerance MM] [-tf N]

The names are the reference's: ``Evaluator`` (:31-268), ``NiftiEvaluator`` (:271-305), ``aggregate_scores`` (:323-402),
``evaluate_folder`` (:448-468).  What differs is how a case is scored: one census pass over both label volumes on the device
(``evaluation.evaluator.evaluate_pair_device``, csrc/evaluate.hip) gives every confusion count and the label boxes, and the surface
metrics of ``advanced=True`` come from the kernels of csrc/surface.hip -- instead of thirteen boolean passes and medpy's distance
transforms per label.  The metrics are the thirteen confusion-matrix ones the engine's ``validate`` writes (the reference's list
has a fourteenth, "surface_dice_at_tolerance": the surfel-area surface Dice, which is not built); ``nsd_tolerance`` adds "Normalized Surface
Dice".  One process owns the GPU; ``num_threads`` host threads only read and inflate the files ahead of it, so the file written does
not depend on their number.  ``to_pandas`` and ``aggregate_scores_for_experiment`` are not built.
"""
import os
from collections import OrderedDict
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from .evaluation.evaluator import DEFAULT_METRICS, evaluate_pair_device, summarise_scores
from .evaluation.surface_distance import ADVANCED_METRICS


class Evaluator:
    """Holds a test and a reference segmentation with label information and computes the metrics of the two.  ``labels``: a list,
    tuple, set or array of ints, or a dict ``label -> name`` whose keys may be tuples of ints (regions); None: the values present."""

    default_metrics = list(DEFAULT_METRICS)
    default_advanced_metrics = list(ADVANCED_METRICS)

    def __init__(self, test=None, reference=None, labels=None, nan_for_nonexisting=True):
        self.test = None
        self.reference = None
        self.labels = None
        self.nan_for_nonexisting = nan_for_nonexisting
        self.result = None
        self.set_reference(reference)
        self.set_test(test)
        if labels is not None:
            self.set_labels(labels)
        elif test is not None and reference is not None:
            self.construct_labels()

    def set_test(self, test):
        self.test = test

    def set_reference(self, reference):
        self.reference = reference

    def set_labels(self, labels):
        if isinstance(labels, dict):
            self.labels = OrderedDict(labels)
        elif isinstance(labels, set):
            self.labels = list(labels)
        elif isinstance(labels, np.ndarray):
            self.labels = [i for i in labels]
        elif isinstance(labels, (list, tuple)):
            self.labels = labels
        else:
            raise TypeError("Can only handle dict, list, tuple, set & numpy array, but input is of type {}".format(type(labels)))

    def construct_labels(self):
        """the label set from the unique entries of the segmentations (a host pass; ``evaluate`` with no labels set reads them
        from its device pass instead)"""
        if self.test is None and self.reference is None:
            raise ValueError("No test or reference segmentations.")
        host = lambda x: x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)
        if self.test is None:
            labels = np.unique(host(self.reference))
        else:
            labels = np.union1d(np.unique(host(self.test)), np.unique(host(self.reference)))
        self.labels = [int(x) for x in labels]

    def evaluate(self, test=None, reference=None, advanced=False, **metric_kwargs):
        """``metric_kwargs``: ``voxel_spacing`` (array-axis order), ``nsd_tolerance``, ``connectivity`` (1, the only value built)"""
        if test is not None:
            self.set_test(test)
        if reference is not None:
            self.set_reference(reference)
        if self.test is None or self.reference is None:
            raise ValueError("Need both test and reference segmentations.")
        unknown = set(metric_kwargs) - {"voxel_spacing", "nsd_tolerance", "connectivity"}
        if unknown:
            raise TypeError("unknown metric arguments %s" % sorted(unknown))
        if metric_kwargs.get("connectivity", 1) != 1:
            raise NotImplementedError("connectivity %r: only the 6-neighbour cross (connectivity=1) is built" % (metric_kwargs["connectivity"],))
        self.result = evaluate_pair_device(self.test, self.reference, self.labels, self.nan_for_nonexisting, advanced,
                                           metric_kwargs.get("voxel_spacing"), metric_kwargs.get("nsd_tolerance"))
        if self.labels is None:
            self.labels = [int(k) for k in self.result]
        return self.result

    def to_dict(self):
        if self.result is None:
            self.evaluate()
        return self.result

    def to_array(self):
        """the result as a numpy array (labels x metrics, the metrics sorted by name)"""
        if self.result is None:
            self.evaluate()
        keys = [str(n) for n in self.labels.values()] if isinstance(self.labels, dict) else [str(l) for l in self.labels]
        result_metrics = sorted(self.result[keys[0]].keys())
        a = np.zeros((len(keys), len(result_metrics)), dtype=np.float32)
        for i, k in enumerate(keys):
            for j, metric in enumerate(result_metrics):
                a[i][j] = self.result[k][metric]
        return a


def default_reader(path):
    """path -> (array, spacing in array-axis order or None).  ``.npy`` (what ``inference.predict.nifti_writer`` writes where
    SimpleITK is missing) is read natively and has no spacing; everything else goes through SimpleITK, spacing ``GetSpacing()[::-1]``
    as in the reference (:299-303)."""
    if path.endswith(".npy"):
        return np.load(path), None
    try:
        import SimpleITK as sitk
    except ImportError:
        raise ImportError("reading %s needs SimpleITK (only .npy volumes are read without it); pass a reader" % path)
    img = sitk.ReadImage(path)
    return sitk.GetArrayFromImage(img), tuple(float(v) for v in img.GetSpacing())[::-1]


def _decoded(volume):
    """what a reader returned as the volume: a ``nifti.NiftiRaw`` (the host half of ``nifti.evaluator_reader``, possibly from a
    read-ahead thread) is decoded here, on the calling thread, into a device uint8 tensor; anything else is the volume"""
    from . import nifti
    return nifti.decode_u8(volume) if isinstance(volume, nifti.NiftiRaw) else volume


class NiftiEvaluator(Evaluator):
    """``Evaluator`` whose test and reference are file names, read through ``reader(path) -> (array, spacing or None)``"""

    def __init__(self, *args, reader=None, **kwargs):
        self.reader = default_reader if reader is None else reader
        self.test_spacing = None
        self.reference_spacing = None
        super().__init__(*args, **kwargs)

    def set_test(self, test, loaded=None):
        """``loaded``: what ``reader(test)`` returned, when somebody read the file ahead"""
        if test is not None:
            array, self.test_spacing = self.reader(test) if loaded is None else loaded
            super().set_test(_decoded(array))
        else:
            self.test_spacing = None
            super().set_test(test)

    def set_reference(self, reference, loaded=None):
        if reference is not None:
            array, self.reference_spacing = self.reader(reference) if loaded is None else loaded
            super().set_reference(_decoded(array))
        else:
            self.reference_spacing = None
            super().set_reference(reference)

    def evaluate(self, test=None, reference=None, voxel_spacing=None, **metric_kwargs):
        if test is not None:
            self.set_test(test)
            test = None
        if voxel_spacing is None:
            voxel_spacing = self.test_spacing
        return super().evaluate(test, reference, voxel_spacing=voxel_spacing, **metric_kwargs)


def _read_ahead(pairs, reader, num_threads):
    """yields (test, reference, what reader gave for each) in the order of ``pairs``; at most 2 * num_threads cases are held"""
    if reader is None:
        for t, r in pairs:
            yield t, r, None, None
        return
    load = lambda x: reader(x) if isinstance(x, str) else None
    with ThreadPoolExecutor(max(1, int(num_threads))) as pool:
        window, pending = 2 * max(1, int(num_threads)), []
        it = iter(pairs)
        while True:
            while len(pending) < window:
                pair = next(it, None)
                if pair is None:
                    break
                pending.append((pair, pool.submit(load, pair[0]), pool.submit(load, pair[1])))
            if not pending:
                return
            (t, r), ft, fr = pending.pop(0)
            yield t, r, ft.result(), fr.result()


def aggregate_scores(test_ref_pairs, evaluator=NiftiEvaluator, labels=None, nanmean=True, json_output_file=None, json_name="",
                     json_description="", json_author="Fabian", json_task="", num_threads=2, **metric_kwargs):
    """``test_ref_pairs``: (prediction, ground truth) file names for a ``NiftiEvaluator``, arrays for an ``Evaluator``.  Returns the
    reference's ``all_scores`` and writes its summary.json.  ``metric_kwargs``: ``advanced``, ``voxel_spacing``, ``nsd_tolerance``.
    With ``advanced`` a case's entry records the spacing it was scored with under "voxel_spacing", as ``validate`` does."""
    if isinstance(evaluator, type):
        evaluator = evaluator()
    if labels is not None:
        evaluator.set_labels(labels)
    fixed_labels = evaluator.labels
    reader = getattr(evaluator, "reader", None)
    results = []
    for test, ref, lt, lr in _read_ahead(list(test_ref_pairs), reader, num_threads):
        evaluator.labels = fixed_labels                      # (None: every case constructs its own, as run_evaluation does)
        if reader is not None:
            evaluator.set_test(test, lt)
            evaluator.set_reference(ref, lr)
        else:
            evaluator.set_test(test)
            evaluator.set_reference(ref)
        kw = dict(metric_kwargs)
        if kw.get("advanced"):
            spacing = kw.get("voxel_spacing")
            if spacing is None:
                spacing = getattr(evaluator, "test_spacing", None)
            kw["voxel_spacing"] = [1., 1., 1.] if spacing is None else [float(v) for v in spacing]
        res = evaluator.evaluate(**kw)
        if kw.get("advanced"):
            res["voxel_spacing"] = kw["voxel_spacing"]
        if isinstance(test, str):
            res["test"] = test
        if isinstance(ref, str):
            res["reference"] = ref
        results.append(res)
    return summarise_scores(results, nanmean, json_output_file, json_name, json_description, json_author, json_task)


def pair_files(folder_with_gts, folder_with_predictions):
    """[(prediction path, ground-truth path)]: every prediction file with the ground-truth file of the same name with '_0000'
    removed (reference :461-464).  The suffix is .nii.gz, or .npy when the prediction folder holds no .nii.gz.  Every missing
    ground-truth file is named in one FileNotFoundError."""
    files = sorted(f for f in os.listdir(folder_with_predictions) if os.path.isfile(os.path.join(folder_with_predictions, f)))
    suffix = ".nii.gz" if any(f.endswith(".nii.gz") for f in files) else ".npy"
    pairs = [(os.path.join(folder_with_predictions, f), os.path.join(folder_with_gts, "".join(f.split("_0000"))))
             for f in files if f.endswith(suffix)]
    missing = [r for _, r in pairs if not os.path.isfile(r)]
    if missing:
        raise FileNotFoundError("%d ground-truth file(s) missing: %s" % (len(missing), ", ".join(missing)))
    return pairs


def evaluate_folder(folder_with_gts, folder_with_predictions, labels, num_threads=8, reader=None, **metric_kwargs):
    """writes summary.json into ``folder_with_predictions`` and returns the scores.  ``reader``: the ``NiftiEvaluator``'s (None:
    ``default_reader``)"""
    pairs = pair_files(folder_with_gts, folder_with_predictions)
    evaluator = NiftiEvaluator if reader is None else NiftiEvaluator(reader=reader)
    return aggregate_scores(pairs, evaluator=evaluator, json_output_file=os.path.join(folder_with_predictions, "summary.json"), num_threads=num_threads,
                            labels=labels, **metric_kwargs)


def build_parser():
    import argparse
    from . import nifti
    parser = argparse.ArgumentParser(description="Evaluates the segmentations located in the folder pred. Output of this script is a json "
                                                 "file. At the very bottom of the json file is going to be a 'mean' entry with averages "
                                                 "metrics across all cases")
    parser.add_argument("-ref", required=True, type=str, help="Folder containing the reference segmentations (.nii.gz, or .npy).")
    parser.add_argument("-pred", required=True, type=str, help="Folder containing the predicted segmentations. File names must match "
                                                              "between the folders ('_0000' in a prediction's name is dropped)!")
    parser.add_argument("-l", nargs="+", type=int, required=True, help="List of label IDs (integer values) that should be evaluated, "
                                                                       "for example -l 1 2 for LiTS (0: background, 1: liver, 2: tumor).")
    parser.add_argument("--advanced", action="store_true", help="add HD95, ASD and ASSD, scored under each prediction's voxel spacing")
    parser.add_argument("--nsd_tolerance", type=float, default=None, metavar="MM", help="add the Normalized Surface Dice at this "
                                                                                        "tolerance (implies --advanced)")
    parser.add_argument("-tf", type=int, default=8, metavar="N", help="host threads that read files ahead of the device (default 8)")
    nifti.add_argument(parser)
    return parser


def select_reader(args):
    """the ``reader`` handed to ``evaluate_folder``: None (``default_reader``); with ``--native_nifti``, ``nifti.evaluator_reader``"""
    from . import nifti
    cb = nifti.from_args(args)                         # (refuses --inflate_any without --native_nifti)
    return cb.evaluator_reader if args.native_nifti else None


def main(argv=None):
    args = build_parser().parse_args(argv)
    kw = {}
    if args.advanced or args.nsd_tolerance is not None:
        kw["advanced"] = True
    if args.nsd_tolerance is not None:
        kw["nsd_tolerance"] = args.nsd_tolerance
    return evaluate_folder(args.ref, args.pred, tuple(args.l), num_threads=args.tf, reader=select_reader(args), **kw)


if __name__ == "__main__":
    main()
