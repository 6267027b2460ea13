"""``python -m e2enet_medical_amd.simple_predict`` -- the reference's inference entry point (simple_predict.py:25-228) on the MI355X
engine: the same argv; the checkpoint name is prefixed with ``--Tconv`` (:152) and ``predict_from_folder`` runs the cases
``[part_id::num_parts]`` (one process per GPU; within a process ``SegmentationNetwork.shard_tiles`` can split the tiles of a case
over a process group instead).  The input folder holds preprocessed cases (``<case>.npz|.npy`` + ``<case>.pkl``) or raw cases
(``<case>_XXXX.nii.gz``); raw cases are read by a ``reader`` callback (default: SimpleITK) and preprocessed on the device.
``-m 3d_cascade_fullres`` picks the model of ``-ctr`` and reads the first stage's segmentations from ``-l``; without ``-l`` the
``3d_lowres`` model predicts the input folder into ``<output>/3d_lowres_predictions`` first (reference :192-216)."""
import argparse
import os

from . import deflate, nifti, paths
from .inference.predict import predict_from_folder
from .utilities.task_name_id_conversion import convert_id_to_task_name

join, isdir = os.path.join, os.path.isdir


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("-i", '--input_folder', required=False,
                        default='../nnUNet/nnUNet_raw_data_base/nnUNet_raw_data/Task216_AMOS2022_task1/imagesTs/')
    parser.add_argument('-o', "--output_folder", required=False, help="folder for saving predictions",
                        default='../nnUnet/results_imageTs/output_task216_d07_best_new')
    parser.add_argument('-t', '--task_name', help='task name or task ID, required.', default='17', required=False)
    parser.add_argument('-tr', '--trainer_class_name', required=False, default=paths.default_trainer)
    parser.add_argument('-ctr', '--cascade_trainer_class_name', required=False, default=paths.default_cascade_trainer)
    parser.add_argument('-m', '--model', default="3d_fullres", required=False)
    parser.add_argument('-p', '--plans_identifier', default=paths.default_plans_identifier, required=False)
    parser.add_argument('-f', '--folds', nargs='+', default='None')
    parser.add_argument('-z', '--save_npz', required=False, action='store_true')
    parser.add_argument('-l', '--lowres_segmentations', required=False, default='None')
    parser.add_argument("--part_id", type=int, required=False, default=0)
    parser.add_argument("--num_parts", type=int, required=False, default=1)
    parser.add_argument("--num_threads_preprocessing", required=False, default=6, type=int)
    parser.add_argument("--num_threads_nifti_save", required=False, default=2, type=int)
    parser.add_argument("--disable_tta", required=False, default=False, action="store_true")
    parser.add_argument("--overwrite_existing", required=False, default=False, action="store_true")
    parser.add_argument("--mode", type=str, default="normal", required=False, help="Hands off!")
    parser.add_argument("--all_in_gpu", type=str, default="False", required=False)
    parser.add_argument("--step_size", type=float, default=0.5, required=False, help="don't touch")
    parser.add_argument('-chk', help='checkpoint name, default: model_final_checkpoint', required=False,
                        default='model_final_checkpoint')
    parser.add_argument('--disable_mixed_precision', default=False, action='store_true', required=False)
    parser.add_argument('--Tconv', type=str, required=False, default='shiftConvPP', help='ori;shiftConvPP')
    nifti.add_argument(parser)
    deflate.add_argument(parser)
    return parser


def select_callbacks(args, reader=None, writer=None):
    """``(reader, writer)`` handed to ``predict_from_folder``: the caller's; with ``--native_nifti``, ``nifti.reader`` and
    ``nifti.writer`` where none was given"""
    cb = nifti.from_args(args)                         # (refuses --inflate_any without --native_nifti)
    if args.native_nifti:
        return (cb.reader if reader is None else reader), (nifti.writer if writer is None else writer)
    return reader, writer


def main(argv=None, reader=None, writer=None):
    """``reader`` / ``writer``: handed to ``predict_from_folder`` unchanged (None: its SimpleITK defaults)"""
    args = build_parser().parse_args(argv)
    reader, writer = select_callbacks(args, reader, writer)
    folds, lowres_segmentations, all_in_gpu, model = args.folds, args.lowres_segmentations, args.all_in_gpu, args.model
    task_name = args.task_name
    args.chk = f"{args.Tconv}_{args.chk}"                       # simple_predict.py:152
    print(args.chk)
    if not task_name.startswith("Task"):
        task_name = convert_id_to_task_name(int(task_name))
    if lowres_segmentations == "None":
        lowres_segmentations = None
    if isinstance(folds, list):
        if not (folds[0] == 'all' and len(folds) == 1):
            folds = [int(i) for i in folds]
    elif folds == "None":
        folds = None
    else:
        raise ValueError("Unexpected value for argument folds")
    assert all_in_gpu in ['None', 'False', 'True']
    all_in_gpu = {"None": None, "True": True, "False": False}[all_in_gpu]
    seg_reader = nifti.from_args(args).gt_reader if args.native_nifti else None
    if model == "3d_cascade_fullres" and lowres_segmentations is None:
        # reference :192-210: the first stage's predictions of the same input folder, into <output>/3d_lowres_predictions
        print("lowres_segmentations is None. Attempting to predict 3d_lowres first...")
        assert args.part_id == 0 and args.num_parts == 1, "if you don't specify a --lowres_segmentations folder for the " \
                                                          "inference of the cascade, custom values for part_id and num_parts " \
                                                          "are not supported. If you wish to have multiple parts, please " \
                                                          "run the 3d_lowres inference first (separately)"
        lowres_model = join(paths.network_training_output_dir, "3d_lowres", task_name, args.trainer_class_name + "__" + args.plans_identifier)
        assert isdir(lowres_model), "model output folder not found. Expected: %s" % lowres_model
        lowres_output_folder = join(args.output_folder, "3d_lowres_predictions")
        predict_from_folder(lowres_model, args.input_folder, lowres_output_folder, folds, False, args.num_threads_preprocessing,
                            args.num_threads_nifti_save, None, args.part_id, args.num_parts, not args.disable_tta,
                            overwrite_existing=args.overwrite_existing, mode=args.mode, overwrite_all_in_gpu=all_in_gpu,
                            mixed_precision=not args.disable_mixed_precision, step_size=args.step_size, checkpoint_name=args.chk,
                            writer=writer, reader=reader, device_deflate=deflate.from_args(args))
        lowres_segmentations = lowres_output_folder
        print("3d_lowres done")
    trainer_name = args.cascade_trainer_class_name if model == "3d_cascade_fullres" else args.trainer_class_name
    model_folder_name = join(paths.network_training_output_dir, model, task_name, trainer_name + "__" + args.plans_identifier)
    print("using model stored in ", model_folder_name)
    assert isdir(model_folder_name), "model output folder not found. Expected: %s" % model_folder_name
    return predict_from_folder(model_folder_name, args.input_folder, args.output_folder, folds, args.save_npz,
                               args.num_threads_preprocessing, args.num_threads_nifti_save, lowres_segmentations, args.part_id,
                               args.num_parts, not args.disable_tta, overwrite_existing=args.overwrite_existing, mode=args.mode,
                               overwrite_all_in_gpu=all_in_gpu, mixed_precision=not args.disable_mixed_precision,
                               step_size=args.step_size, checkpoint_name=args.chk, writer=writer, reader=reader,
                               device_deflate=deflate.from_args(args), seg_reader=seg_reader)


if __name__ == "__main__":
    main()
