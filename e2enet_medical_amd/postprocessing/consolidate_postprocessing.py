"""One post-processing decision per experiment (reference e2enet/postprocessing/consolidate_postprocessing.py).

   python -m e2enet_medical_amd.postprocessing.consolidate_postprocessing -f FOLDER [--advanced] [--folds 0 1 2 3 4] [--native_nifti]

In the validation of a fold the search only sees that fold's cases, so the folds can reach different decisions.
``consolidate_folds`` collects the raw validation predictions of all folds into ``<FOLDER>/cv_niftis_raw``, runs the search over all
of them against ``<FOLDER>/gt_niftis`` (the folder form of ``determine_postprocessing``: one component table per case on the
device, the search on the tables) and leaves ``<FOLDER>/postprocessing.json``, which ``predict_from_folder`` applies, and the
post-processed predictions in ``<FOLDER>/cv_niftis_postprocessed``.

``<FOLDER>/cv_niftis_raw/summary.json``, which the search reads the classes and the number of cases from, is put together from the
folds' own ``summary.json`` files (the reference scores the collected files again to the same end)."""
import json
import os
import shutil

from .connected_components import determine_postprocessing, label_files, native_reader

join, isdir = os.path.join, os.path.isdir


def collect_cv_niftis(cv_folder, output_folder, validation_folder_name='validation_raw', folds=(0, 1, 2, 3, 4)):
    """reference :25-40: the label files of every ``<cv_folder>/fold_<i>/<validation_folder_name>`` copied into ``output_folder``"""
    validation_raw_folders = [join(cv_folder, "fold_%d" % i, validation_folder_name) for i in folds]
    exist = [isdir(i) for i in validation_raw_folders]
    if not all(exist):
        raise RuntimeError("some folds are missing. Please run the full 5-fold cross-validation. "
                           "The following folds seem to be missing: %s" % [i for j, i in enumerate(folds) if not exist[j]])
    os.makedirs(output_folder, exist_ok=True)
    for folder in validation_raw_folders:
        for f in label_files(folder):
            shutil.copy(join(folder, f), output_folder)


def _merged_summary(summaries, raw_folder, gt_folder, json_output_file):
    """the folds' score records as one summary.json of the collected folder, the file names pointing into it"""
    from ..evaluation.evaluator import summarise_scores
    records = []
    for name in summaries:
        with open(name, 'r') as f:
            for res in json.load(f)['results']['all']:
                if "test" in res:
                    name = os.path.basename(res["test"])
                    res["test"], res["reference"] = join(raw_folder, name), join(gt_folder, name)
                records.append(res)
    return summarise_scores(records, json_output_file=json_output_file, json_author="Fabian")


def consolidate_folds(output_folder_base, validation_folder_name='validation_raw', advanced_postprocessing=False,
                      folds=(0, 1, 2, 3, 4), num_threads=8, **folder_search):
    """reference :43-85.  ``output_folder_base``: the experiment's output folder (``fold_0``, ``fold_1``, ... are its subfolders and
    ``gt_niftis`` holds the ground truths).  ``folder_search``: ``reader``, ``writer`` (and the test hooks ``table``, ``remove``) of
    ``determine_postprocessing_folder``.  Returns ``pp_results``."""
    folds = tuple(int(f) for f in folds)
    output_folder_raw = join(output_folder_base, "cv_niftis_raw")
    if isdir(output_folder_raw):
        shutil.rmtree(output_folder_raw)
    output_folder_gt = join(output_folder_base, "gt_niftis")
    collect_cv_niftis(output_folder_base, output_folder_raw, validation_folder_name, folds)
    niftis = label_files(output_folder_raw)
    suffix = ".nii.gz" if niftis and niftis[0].endswith(".nii.gz") else ".npy"
    num_niftis_gt = len([f for f in os.listdir(output_folder_gt) if f.endswith(suffix)]) if isdir(output_folder_gt) else 0
    if len(niftis) != num_niftis_gt:
        raise AssertionError("If does not seem like you trained all the folds! Train all folds first!")
    _merged_summary([join(output_folder_base, "fold_%d" % i, validation_folder_name, "summary.json") for i in folds],
                    output_folder_raw, output_folder_gt, join(output_folder_raw, "summary.json"))
    return determine_postprocessing(output_folder_base, output_folder_gt, 'cv_niftis_raw', final_subf_name="cv_niftis_postprocessed",
                                    processes=num_threads, advanced_postprocessing=advanced_postprocessing, **folder_search)


def build_parser():
    import argparse
    from .. import nifti
    parser = argparse.ArgumentParser(description="Determines the postprocessing of an experiment from the validation predictions "
                                                 "of all its folds and writes postprocessing.json into the experiment's folder.")
    parser.add_argument("-f", type=str, required=True, help="experiment output folder (fold_0, fold_1, etc must be subfolders of "
                                                            "the given folder)")
    parser.add_argument("--advanced", action="store_true", default=False,
                        help="also determine a minimum valid object size per entry (advanced_postprocessing)")
    parser.add_argument("--folds", nargs="+", type=int, default=[0, 1, 2, 3, 4], help="the folds to collect (default 0 1 2 3 4)")
    parser.add_argument("-val", type=str, default="validation_raw", help="validation folder name (default validation_raw)")
    parser.add_argument("-tf", type=int, default=8, metavar="N", help="host threads that read files ahead of the device (default 8)")
    nifti.add_argument(parser)
    return parser


def select_callbacks(args):
    """the ``reader`` / ``writer`` keywords of the folder search: none (its defaults); with ``--native_nifti`` this package's own"""
    from .. import nifti
    inflate = nifti.inflate_from_args(args)            # (refuses --inflate_any without --native_nifti)
    if args.native_nifti:
        import functools
        return {"reader": native_reader if inflate == "host" else functools.partial(native_reader, inflate=inflate),
                "writer": nifti.writer}
    return {}


def main(argv=None):
    args = build_parser().parse_args(argv)
    return consolidate_folds(args.f, args.val, args.advanced, tuple(args.folds), num_threads=args.tf, **select_callbacks(args))


if __name__ == "__main__":
    main()
