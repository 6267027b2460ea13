"""``consolidate_folds`` for a model named the way ``simple_predict`` names it (reference
e2enet/postprocessing/consolidate_postprocessing_simple.py).

   python -m e2enet_medical_amd.postprocessing.consolidate_postprocessing_simple -m 3d_fullres -t 17 [-tr TRAINER] [-pl PLANS] [-val NAME]

The folder is ``<network_training_output_dir>/<model>/<task>/<trainer>__<plans>``, as ``simple_predict`` builds it."""
import os

from .. import paths
from ..utilities.task_name_id_conversion import convert_id_to_task_name
from .consolidate_postprocessing import consolidate_folds, select_callbacks


def build_parser():
    import argparse
    from .. import nifti
    parser = argparse.ArgumentParser(usage="Used to determine the postprocessing for a trained model. Useful for when the best "
                                           "configuration (2d, 3d_fullres etc) as selected manually.")
    parser.add_argument("-m", type=str, default='3d_fullres', help="U-Net model (2d, 3d_lowres, 3d_fullres or 3d_cascade_fullres)")
    parser.add_argument("-t", type=str, default='17', help="Task name or id")
    parser.add_argument("-tr", type=str, required=False, default=None,
                        help="nnUNetTrainer class. Default: %s, unless 3d_cascade_fullres (then it's %s)"
                             % (paths.default_trainer, paths.default_cascade_trainer))
    parser.add_argument("-pl", type=str, required=False, default=paths.default_plans_identifier,
                        help="Plans name, Default=%s" % paths.default_plans_identifier)
    parser.add_argument("-val", type=str, required=False, default="validation_nnunet_raw",
                        help="Validation folder name. Default: validation_nnunet_raw")
    nifti.add_argument(parser)
    return parser


def model_folder(args):
    """the experiment's output folder from the parsed arguments"""
    task = args.t
    if not task.startswith("Task"):
        task = convert_id_to_task_name(int(task))
    trainer = args.tr
    if trainer is None:
        trainer = paths.default_cascade_trainer if args.m == "3d_cascade_fullres" else paths.default_trainer
    return os.path.join(paths.network_training_output_dir, args.m, task, trainer + "__" + args.pl)


def main(argv=None):
    args = build_parser().parse_args(argv)
    return consolidate_folds(model_folder(args), args.val, **select_callbacks(args))


if __name__ == "__main__":
    main()
