"""``python -m e2enet_medical_amd.simple_main`` -- the reference's training entry point (simple_main.py:33-216) on the MI355X
engine: the same argv (incl. the sparse flags of ``add_sparse_args``), the same sequence

    get_default_configuration -> nnUNetTrainer_simple(...) -> initialize() -> CosineDecay / Masking / add_module
    -> [load_latest_checkpoint | pretrained weights] -> run_training(mask)      |  --validation_only: load checkpoint -> validate

Differences, all stated: ``--fp32`` / mixed precision is accepted and ignored (fp32 results); ``-c`` restores the DSFF masks and the
optimizer state from the checkpoint (the reference re-draws the masks before loading); ``--base_num_features``
is an extension (the reference hard-codes 48, nnUNetTrainer_simple.py:296); ``--synthetic_data`` trains on seeded noise when no
preprocessed data exists (benchmarks / smoke tests); ``--resident_data GIB`` keeps the preprocessed cases on the device and cuts the
training batches there; ``--validation_only`` really validates (the reference's call is commented out,
:200-208); after a ``3d_lowres`` run the validation cases are predicted for the cascade's next stage
(``training/cascade_stuff/predict_next_stage.py``) unless ``--disable_next_stage_pred``; ``--find_lr`` is outside the engine."""
import argparse
import os

import torch

from . import paths
from .run.default_configuration import get_default_configuration
from .training.network_training.nnUNetTrainer_simple import nnUNetTrainer_simple
from .training.network_training.sparselearning.core_channel import Masking, CosineDecay, add_sparse_args
from .utilities.task_name_id_conversion import convert_id_to_task_name


def str2bool(s):
    return True if s.lower() == 'true' else False


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("--network", type=str, default='3d_fullres')
    parser.add_argument("--network_trainer", type=str, default='nnUNetTrainerV2')
    parser.add_argument("--task", help="can be task name or task id", type=str, default='1')
    parser.add_argument("--fold", help='0, 1, ..., 5 or \'all\'', type=str, default='0')
    parser.add_argument("--validation_only", required=False, type=str2bool, default=False,
                        help="use this if you want to only run the validation")
    parser.add_argument("-c", "--continue_training", help="use this if you want to continue a training", action="store_true")
    parser.add_argument("-p", help="plans identifier. Only change this if you created a custom experiment planner",
                        default=paths.default_plans_identifier, required=False)
    parser.add_argument("--use_compressed_data", default=False, action="store_true", required=False)
    parser.add_argument("--deterministic", required=False, default=False, action="store_true")
    parser.add_argument("--npz", required=False, default=True, action="store_true")
    parser.add_argument("--find_lr", required=False, default=False, action="store_true", help="not used here, just for fun")
    parser.add_argument("--valbest", required=False, default=False, type=str2bool)
    parser.add_argument("--fp32", required=False, default=False, action="store_true",
                        help="disable mixed precision training and run old school fp32 (the engine always does)")
    parser.add_argument("--val_folder", required=False, default="validation_raw")
    parser.add_argument("--disable_saving", required=False, action='store_true')
    parser.add_argument("--disable_postprocessing_on_folds", required=False, action='store_true')
    parser.add_argument('--val_disable_overwrite', action='store_false', default=True,
                        help='Validation does not overwrite existing segmentations')
    parser.add_argument('--disable_next_stage_pred', action='store_true', default=False, help='do not predict next stage')
    parser.add_argument('--pretrained_weights', type=str, required=False, default=None)
    parser.add_argument('--Tconv', type=str, required=False, default='ori', help='ori;shiftConvPP')
    parser.add_argument('--max_num_epochs', type=int, required=False, default=5)
    parser.add_argument('--num_batches_per_epoch', type=int, required=False, default=5)
    # ---- extensions of this package (absent from the reference's parser) ----
    parser.add_argument('--base_num_features', type=int, required=False, default=None,
                        help='network width; default: the reference\'s hard-coded 48')
    parser.add_argument('--determine_postprocessing', action='store_true', default=False,
                        help='after the validation, search for which classes removing all but the largest connected component '
                             'improves the Dice and write postprocessing.json (on the device; the reference always does this)')
    parser.add_argument('--synthetic_data', action='store_true', default=False,
                        help='train on seeded Gaussian noise / random labels when no preprocessed data exists')
    parser.add_argument('--resident_data', type=float, required=False, default=None, metavar='GIB',
                        help='keep up to GIB GiB of preprocessed cases on the device and cut every training batch there with one '
                             'kernel launch (negative: no limit; 0: stage every case, still crop and pad on the device); '
                             'default: the host loader')
    parser.add_argument('--device_inflate', action='store_true', default=False,
                        help='with --resident_data: a case without an unpacked .npy is inflated from its .npz on the GPU (members '
                             'that --device_deflate wrote; others are inflated on the host as before) instead of on the host')
    from . import deflate, nifti
    nifti.add_argument(parser)
    deflate.add_argument(parser)
    add_sparse_args(parser)
    return parser


def select_validation_callbacks(args):
    """``(writer, gt_reader)`` handed to ``validate``: None, None (its own defaults); with ``--native_nifti``, ``nifti.writer`` and
    ``nifti.gt_reader``"""
    from . import nifti
    cb = nifti.from_args(args, also=("resident_data",))
    if args.native_nifti:
        return nifti.writer, cb.gt_reader
    return None, None


def select_trainer_class(network_trainer):
    """the reference forces nnUNetTrainer_simple whatever --network_trainer says (simple_main.py:145); the one other trainer of
    other trainers of this package, the region trainer nnUNetTrainerV2BraTSRegions and the cascade's second stage
    nnUNetTrainerV2CascadeFullRes, are selected by their names.  ``3d_cascade_fullres`` with any other name trains the last stage
    without the previous stage's segmentation, as the reference's simple_main does."""
    if network_trainer == 'nnUNetTrainerV2BraTSRegions':
        from .training.network_training.competitions_with_custom_Trainers.BraTS2020.nnUNetTrainerV2BraTSRegions import \
            nnUNetTrainerV2BraTSRegions
        return nnUNetTrainerV2BraTSRegions
    if network_trainer == 'nnUNetTrainerV2CascadeFullRes':
        from .training.network_training.nnUNetTrainerV2CascadeFullRes import nnUNetTrainerV2CascadeFullRes
        return nnUNetTrainerV2CascadeFullRes
    return nnUNetTrainer_simple


def load_pretrained_weights(network, fname, verbose=False):
    """reference e2enet/run/load_pretrained_weights.py: copy every checkpoint tensor whose name and shape match the network
    (segmentation heads may differ between tasks and are skipped)."""
    saved = torch.load(fname, map_location=torch.device('cpu'), weights_only=False)['state_dict']
    own = network.state_dict()
    new = {}
    for k, v in saved.items():
        key = k[7:] if k.startswith('module.') else k
        if key in own and tuple(own[key].shape) == tuple(v.shape):
            new[key] = v
    if not new:
        raise RuntimeError("Pretrained weights are not compatible with the current network architecture")
    own.update(new)
    print("################### Loading pretrained weights from file ", fname, '###################')
    network.load_state_dict(own)


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.device_inflate and args.resident_data is None:
        parser.error("--device_inflate needs --resident_data: it inflates the cases that are kept on the device")
    if args.inflate_any and args.resident_data is None and not args.native_nifti:
        parser.error("--inflate_any needs --resident_data (it inflates the zlib-written cases that are kept on the device) or "
                     "--native_nifti (it inflates the .nii.gz files that are read)")
    print(args)
    task, fold, network = args.task, args.fold, args.network
    if not task.startswith("Task"):
        task = convert_id_to_task_name(int(task))
    if fold != 'all':
        fold = int(fold)
    plans_file, output_folder_name, dataset_directory, batch_dice, stage, trainer_class = \
        get_default_configuration(network, task, args.network_trainer, args.p)
    trainer_class = select_trainer_class(args.network_trainer)
    trainer = trainer_class(plans_file, fold, output_folder=output_folder_name, dataset_directory=dataset_directory,
                            batch_dice=batch_dice, stage=stage, unpack_data=not args.use_compressed_data,
                            deterministic=args.deterministic, fp16=not args.fp32, Tconv=args.Tconv,
                            max_num_epochs=args.max_num_epochs, num_batches_per_epoch=args.num_batches_per_epoch, args=args)
    trainer.base_num_features_override = args.base_num_features
    trainer.synthetic_data = bool(args.synthetic_data)
    trainer.resident_data_gib = args.resident_data
    # (--inflate_any with --resident_data implies --device_inflate and extends it to members of other writers)
    trainer.device_inflate = "any" if (args.inflate_any and args.resident_data is not None) else bool(args.device_inflate)
    if args.disable_saving:
        trainer.save_final_checkpoint = False
        trainer.save_best_checkpoint = False
        trainer.save_intermediate_checkpoints = True
        trainer.save_latest_only = True
    model, optimizer = trainer.initialize(not args.validation_only)
    print("Total parameters count", sum(p.numel() for p in model.parameters() if p.requires_grad))
    mask = None
    if args.sparse:
        decay = CosineDecay(args.death_rate, args.max_num_epochs * args.num_batches_per_epoch)
        mask = Masking(optimizer, death_rate=args.death_rate, death_mode=args.death, death_rate_decay=decay,
                       growth_mode=args.growth, redistribution_mode=args.redistribution, args=args)
        mask.add_module(model, sparse_init=args.sparse_init, density=args.density)
    if args.find_lr:
        raise NotImplementedError("--find_lr (reference nnUNetTrainer_simple.find_lr, 'just for fun') is outside the engine")
    if not args.validation_only:
        if args.continue_training:
            # (the checkpoint written by run_training carries 'dsff_state': masks, schedule position and RNG continue where they were)
            try:
                trainer.load_latest_checkpoint(mask=mask)
            except KeyError:
                trainer.load_latest_checkpoint()          # a checkpoint of the reference: no DSFF state, fresh masks like the reference
        elif args.pretrained_weights is not None:
            load_pretrained_weights(trainer.network, args.pretrained_weights)
        trainer.run_training(mask)
    else:
        if args.valbest:
            trainer.load_best_checkpoint(train=False)
        else:
            trainer.load_final_checkpoint(train=False)
    trainer.network.eval()
    if args.validation_only:
        from . import deflate
        writer, gt_reader = select_validation_callbacks(args)
        trainer.validate(save_softmax=args.npz, validation_folder_name=args.val_folder,
                         run_postprocessing_on_folds=not args.disable_postprocessing_on_folds, overwrite=args.val_disable_overwrite,
                         determine_postprocessing=args.determine_postprocessing, writer=writer, gt_reader=gt_reader,
                         device_deflate=deflate.from_args(args))
    print(f'finish training {args.Tconv} !!!')
    if network == '3d_lowres' and not args.disable_next_stage_pred:
        # reference :213-215: the validation cases of this fold, predicted and resampled for the full-resolution stage
        from .training.cascade_stuff.predict_next_stage import predict_next_stage
        print("predicting segmentations for the next stage of the cascade")
        predict_next_stage(trainer, os.path.join(dataset_directory, trainer.plans['data_identifier'] + "_stage%d" % 1))
    return trainer


if __name__ == "__main__":
    main()
