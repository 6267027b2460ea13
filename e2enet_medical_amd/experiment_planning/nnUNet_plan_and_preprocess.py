"""``python -m e2enet_medical_amd.experiment_planning.nnUNet_plan_and_preprocess -t ID`` -- step 1 of the reference's README in one
command (e2enet/experiment_planning/nnUNet_plan_and_preprocess.py:27-168, the reference's argv): the raw task folder
``<nnUNet_raw_data_base>/nnUNet_raw_data/TaskID_*`` is verified (``--verify_dataset_integrity``), cropped and fingerprinted on the
device, planned on the host and preprocessed on the device into ``<nnUNet_preprocessed>/TaskID_*``: ``dataset_properties.pkl``,
``dataset.json``, ``nnUNetPlansv2.1_plans_3D.pkl``, ``gt_segmentations`` and one ``nnUNetData_plans_v2.1_stage<i>`` folder per stage,
which is what ``simple_main`` trains on.  ``-no_pp`` stops after the plans file.

It runs the functions ``crop_and_fingerprint`` and ``preprocess_dataset`` run; those two commands stay for doing one leg alone.
Built: the 3-D planners ``ExperimentPlanner3D_v21`` (default) and ``ExperimentPlanner``.  Not built, and refused before any work is
done: a 2-D planner (``-pl2d``; this package has no 2-D path) and ``-overwrite_plans`` (the reference's
``ExperimentPlanner3D_v21_Pretrained``).  The plans file is written whether or not it has a lowres stage; the trainer still refuses the
cascade."""
import argparse
import json
import os
import shutil

from .. import deflate, nifti, paths
from ..preprocessing.sanity_checks import verify_dataset_integrity
from ..utilities.task_name_id_conversion import convert_id_to_task_name
from .DatasetAnalyzer import DatasetAnalyzer
from .experiment_planner_baseline_3DUNet import ExperimentPlanner
from .experiment_planner_baseline_3DUNet_v21 import ExperimentPlanner3D_v21
from .utils import crop

PLANNERS_3D = {"ExperimentPlanner3D_v21": ExperimentPlanner3D_v21, "ExperimentPlanner": ExperimentPlanner}


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("-t", "--task_ids", nargs="+", type=int, required=True,
                        help="integer ids of the tasks to plan and preprocess; each needs a folder 'TaskXXX_...' in the raw data folder")
    parser.add_argument("-pl3d", "--planner3d", type=str, default="ExperimentPlanner3D_v21",
                        help="the planner class of the 3-D U-Net: ExperimentPlanner3D_v21 (default) or ExperimentPlanner; 'None' "
                             "plans nothing")
    parser.add_argument("-pl2d", "--planner2d", type=str, default=None,
                        help="the planner class of the 2-D U-Net: not built, anything but 'None' is refused")
    parser.add_argument("-no_pp", action="store_true",
                        help="only plan: write the plans file, do not preprocess")
    parser.add_argument("-tl", type=int, required=False, default=8,
                        help="host threads that compress and write the cases of a lowres stage (at most 16)")
    parser.add_argument("-tf", type=int, required=False, default=8,
                        help="host threads of the cropping, the fingerprint, the integrity check and the fullres stage (at most 16); the "
                             "GPU work is one process")
    parser.add_argument("--verify_dataset_integrity", required=False, default=False, action="store_true",
                        help="check the raw task folder first (files, geometry, NaNs, label values): should be done once for each "
                             "dataset")
    parser.add_argument("-overwrite_plans", type=str, default=None, required=False,
                        help="a plans file to use instead of planning: not built, refused")
    parser.add_argument("-overwrite_plans_identifier", type=str, default=None, required=False,
                        help="goes with -overwrite_plans: not built")
    nifti.add_argument(parser)
    deflate.add_argument(parser, what="the <case>.npz of every case")
    return parser


def select_planners(args):
    """``(3-D planner class or None)`` of the arguments; every refusal of the command is raised here, before any work is done"""
    name3d = None if args.planner3d == "None" else args.planner3d
    name2d = None if args.planner2d == "None" else args.planner2d
    if args.overwrite_plans is not None or args.overwrite_plans_identifier is not None:
        raise NotImplementedError("-overwrite_plans (planning with another task's plans file, the reference's "
                                  "ExperimentPlanner3D_v21_Pretrained) is not built")
    if name2d is not None:
        raise NotImplementedError("-pl2d %s: the 2-D planners (ExperimentPlanner2D_v21) are not built, this package has no 2-D path; "
                                  "leave -pl2d at None" % name2d)
    if name3d is not None and name3d not in PLANNERS_3D:
        raise RuntimeError("Could not find the Planner class %s. Make sure it is located somewhere in "
                           "e2enet_medical_amd.experiment_planning" % name3d)
    return PLANNERS_3D[name3d] if name3d is not None else None


def main(argv=None, reader=None):
    args = build_parser().parse_args(argv)
    planner_3d = select_planners(args)
    inflate = nifti.inflate_from_args(args)            # (refuses --inflate_any without --native_nifti)
    reader = nifti.callbacks(inflate).reader if (args.native_nifti and reader is None) else reader

    tasks = []
    for i in args.task_ids:
        task_name = convert_id_to_task_name(int(i))
        if args.verify_dataset_integrity:
            verify_dataset_integrity(os.path.join(paths.nnUNet_raw_data, task_name), args.tf, inflate=inflate)
        crop(task_name, False, args.tf, reader=reader, device_deflate=deflate.from_args(args))
        tasks.append(task_name)

    for t in tasks:
        print("\n\n\n", t)
        cropped_out_dir = os.path.join(paths.nnUNet_cropped_data, t)
        preprocessing_output_dir_this_task = os.path.join(paths.preprocessing_output_dir, t)
        # the intensity properties are collected only when one of the modalities is CT
        with open(os.path.join(cropped_out_dir, 'dataset.json'), 'r') as f:
            modalities = list(json.load(f)["modality"].values())
        collect_intensityproperties = ("CT" in modalities) or ("ct" in modalities)
        dataset_analyzer = DatasetAnalyzer(cropped_out_dir, overwrite=False, num_processes=args.tf)
        dataset_analyzer.analyze_dataset(collect_intensityproperties)

        os.makedirs(preprocessing_output_dir_this_task, exist_ok=True)
        shutil.copy(os.path.join(cropped_out_dir, "dataset_properties.pkl"), preprocessing_output_dir_this_task)
        shutil.copy(os.path.join(paths.nnUNet_raw_data, t, "dataset.json"), preprocessing_output_dir_this_task)

        threads = (args.tl, args.tf)
        print("number of threads: ", threads, "\n")
        if planner_3d is not None:
            exp_planner = planner_3d(cropped_out_dir, preprocessing_output_dir_this_task)
            exp_planner.plan_experiment()
            if not args.no_pp:
                exp_planner.run_preprocessing(threads, device_deflate=deflate.from_args(args))


if __name__ == "__main__":
    main()
