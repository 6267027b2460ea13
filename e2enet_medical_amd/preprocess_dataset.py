"""``python -m e2enet_medical_amd.preprocess_dataset -t TASK`` -- the preprocessing leg of the reference's
``nnUNet_plan_and_preprocess`` on the device: the task's cropped folder (``<nnUNet_raw_data_base>/nnUNet_cropped_data/<task>``) and its
3-D plans file (``<nnUNet_preprocessed>/<task>/<plans identifier>_plans_3D.pkl``, written by the reference's planner, e.g. with
``-no_pp``) into the stage folders ``<nnUNet_preprocessed>/<task>/<data_identifier>_stage<i>`` that ``simple_main`` trains on.
The cropped folder and its fingerprint come from ``python -m e2enet_medical_amd.crop_and_fingerprint``; experiment planning stays
with the reference."""
import argparse
import os

from . import deflate, paths
from .preprocessing.preprocessing import DEFAULT_NUM_THREADS, run_preprocessing
from .utilities.task_name_id_conversion import convert_id_to_task_name


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument('-t', '--task_name', required=True, help='task name or task ID')
    parser.add_argument('-p', '--plans_identifier', default=paths.default_plans_identifier, required=False)
    parser.add_argument('-tf', type=int, default=DEFAULT_NUM_THREADS, required=False,
                        help='host threads that compress and write finished cases (at most 16); the GPU work is one process')
    parser.add_argument('--unpack', action='store_true', help='also write <case>.npy, the file the training loader memory-maps')
    deflate.add_argument(parser, what="the <case>.npz of every case")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    task_name = args.task_name
    if not task_name.startswith("Task"):
        task_name = convert_id_to_task_name(int(task_name))
    cropped = os.path.join(paths.nnUNet_cropped_data, task_name)
    preprocessed = os.path.join(paths.preprocessing_output_dir, task_name)
    plans_file = os.path.join(preprocessed, args.plans_identifier + "_plans_3D.pkl")
    assert os.path.isdir(cropped), "cropped data folder not found. Expected: %s" % cropped
    assert os.path.isfile(plans_file), "plans file not found. Expected: %s" % plans_file
    print("preprocessing", cropped, "with", plans_file)
    run_preprocessing(plans_file, cropped, preprocessed, args.tf, unpack_npy=args.unpack, device_deflate=deflate.from_args(args))


if __name__ == "__main__":
    main()
