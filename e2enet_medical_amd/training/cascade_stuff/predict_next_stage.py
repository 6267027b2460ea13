"""The hand-over of the cascade's first stage: the 3d_lowres network's prediction of every validation case, resampled to the case's
shape in the next stage and stored as a uint8 label volume (``<case>_segFromPrevStage.npz``, key ``data``).

Reference: e2enet/training/cascade_stuff/predict_next_stage.py:31-135.  There the softmax is downloaded, resampled on the host with
``resample_data_or_seg(is_seg=False, order=1)`` to a K x full-resolution float array (``force_separate_z=None`` arrives as
``do_separate_z``, which is falsy: order 1 in all three axes) and reduced by ``argmax(0)``.  Here the softmax stays on the device and one
kernel (``e2e_resample_argmax_u8``) evaluates the K interpolated values per output voxel and writes their first maximum: the large
tensor is never formed.
"""
import argparse
import os
from os.path import isfile, join

import numpy as np
import torch

from ..._lib import lib


def resample_argmax(softmax: torch.Tensor, new_shape, transpose_backward=None) -> torch.Tensor:
    """Softmax [K, X, Y, Z] (a device tensor with any strides; a host array is uploaded) -> device uint8 ``new_shape``: argmax over the classes of the order-1 resize, in the
    transposed-backward frame.  The bits of ``inference.predict.resample_softmax`` followed by ``e2e_export_argmax_u8``."""
    softmax = torch.as_tensor(softmax, dtype=torch.float32)
    if not softmax.is_cuda:
        softmax = softmax.cuda()
    assert softmax.dim() == 4
    tb = [0, 1, 2] if transpose_backward is None else [int(i) for i in transpose_backward]
    dims = [int(softmax.shape[1 + i]) for i in tb]
    strides = [int(softmax.stride(1 + i)) for i in tb]
    new_shape = [int(v) for v in new_shape]
    seg = torch.empty(new_shape, dtype=torch.uint8, device=softmax.device)
    lib().resample_argmax_u8(softmax.data_ptr(), seg.data_ptr(), int(softmax.shape[0]), int(softmax.stride(0)), dims[0], dims[1], dims[2],
                             strides[0], strides[1], strides[2], new_shape[0], new_shape[1], new_shape[2],
                             torch.cuda.current_stream().cuda_stream)
    return seg


def resample_and_save(predicted, target_shape, output_file, force_separate_z=False, interpolation_order=1, interpolation_order_z=0):
    """reference :31-43 for a softmax held in memory (a numpy array or a tensor [K, X, Y, Z]) or stored as ``.npy`` (the file is
    removed, as in the reference)."""
    if force_separate_z or interpolation_order != 1:
        raise NotImplementedError("resample_and_save: order 1 in all three axes is built (what predict_next_stage asks for: "
                                  "force_separate_z=None arrives as do_separate_z)")
    if isinstance(predicted, str):
        assert isfile(predicted), "If isinstance(segmentation_softmax, str) then isfile(segmentation_softmax) must be True"
        del_file = predicted
        predicted = np.load(predicted)
        os.remove(del_file)
    seg = resample_argmax(predicted, target_shape)
    np.savez_compressed(output_file, data=seg.cpu().numpy())


def next_stage_shape(stage_to_be_predicted_folder, data_file):
    """shape [X, Y, Z] of the case in the next stage's folder: from the header of the unpacked ``.npy`` when it is there, else
    from the ``.npz``"""
    name = os.path.basename(data_file)
    npy = join(stage_to_be_predicted_folder, name[:-4] + ".npy")
    if isfile(npy):
        return tuple(int(v) for v in np.load(npy, mmap_mode='r').shape[1:])
    return tuple(int(v) for v in np.load(join(stage_to_be_predicted_folder, name))['data'].shape[1:])


def predict_next_stage(trainer, stage_to_be_predicted_folder):
    """reference :46-87: every case of ``trainer.dataset_val`` predicted with mirroring as trained, the softmax kept on the device,
    resampled to the next stage's shape and written to ``<parent of output_folder>/pred_next_stage``.  Returns the files."""
    output_folder = join(os.path.dirname(os.path.abspath(trainer.output_folder)), "pred_next_stage")
    os.makedirs(output_folder, exist_ok=True)
    if 'segmentation_export_params' in trainer.plans.keys():
        p = trainer.plans['segmentation_export_params']
        if p['force_separate_z'] or p['interpolation_order'] != 1:
            raise NotImplementedError("predict_next_stage: segmentation_export_params other than order 1 in all axes are not built")
    if trainer.dataset_val is None:                                  # (a trainer that was not built for training)
        trainer.folder_with_preprocessed_data = join(trainer.dataset_directory, trainer.plans['data_identifier'] + "_stage%d" % trainer.stage)
        trainer.load_dataset()
        trainer.do_split()
    net = trainer.network
    keep = getattr(net, "keep_on_device", False)
    written = []
    try:
        for pat in trainer.dataset_val.keys():
            print(pat)
            data_file = trainer.dataset_val[pat]['data_file']
            npy = data_file[:-4] + ".npy"
            data = np.load(npy, mmap_mode='r') if isfile(npy) else np.load(data_file)['data']
            data_preprocessed = np.array(data[:-1])
            net.keep_on_device = True
            softmax = trainer.predict_preprocessed_data_return_seg_and_softmax(
                data_preprocessed, do_mirroring=trainer.data_aug_params["do_mirror"], mirror_axes=trainer.data_aug_params['mirror_axes'],
                verbose=False, mixed_precision=trainer.fp16)[1]
            net.keep_on_device = keep
            target_shp = next_stage_shape(stage_to_be_predicted_folder, data_file)
            output_file = join(output_folder, os.path.basename(data_file)[:-4] + "_segFromPrevStage.npz")
            seg = resample_argmax(softmax, target_shp)
            np.savez_compressed(output_file, data=seg.cpu().numpy())
            written.append(output_file)
    finally:
        net.keep_on_device = keep
    return written


def main(argv=None):
    """python -m e2enet_medical_amd.training.cascade_stuff.predict_next_stage TRAINERCLASS TASK FOLD (reference :90-135; usually not
    needed: simple_main runs the hand-over after a 3d_lowres training)"""
    parser = argparse.ArgumentParser()
    parser.add_argument("network_trainer")
    parser.add_argument("task")
    parser.add_argument("fold", type=int)
    args = parser.parse_args(argv)
    from ...run.default_configuration import get_default_configuration
    from ...simple_main import select_trainer_class
    plans_file, output_folder_name, dataset_directory, batch_dice, stage, _ = get_default_configuration("3d_lowres", args.task,
                                                                                                        args.network_trainer)
    trainer = select_trainer_class(args.network_trainer)(plans_file, args.fold, output_folder=output_folder_name,
                                                         dataset_directory=dataset_directory, batch_dice=batch_dice, stage=stage)
    trainer.initialize(False)
    trainer.folder_with_preprocessed_data = join(dataset_directory, trainer.plans['data_identifier'] + "_stage%d" % stage)
    trainer.load_dataset()
    trainer.do_split()
    trainer.load_best_checkpoint(train=False)
    return predict_next_stage(trainer, join(dataset_directory, trainer.plans['data_identifier'] + "_stage%d" % 1))


if __name__ == "__main__":
    main()
