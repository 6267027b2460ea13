"""The full-resolution stage of the two-stage cascade (nnU-Net's nnUNetTrainerV2CascadeFullRes, the class the reference names as
``default_cascade_trainer``, e2enet/paths.py:26) on the MI355X engine.

The network sees the case's modalities plus one channel per foreground class: the one-hot segmentation the ``3d_lowres`` stage predicted
for the case (``training/cascade_stuff/predict_next_stage.py`` writes ``<case>_segFromPrevStage.npz``).  During training the loader
cuts that segmentation as a second seg channel (``DataLoader3D(has_prev_stage=True)``) and the device augmenter expands and disturbs
it (``data_augmentation_moreDA.cascade_transforms``, csrc/cascade.hip); during validation the stored segmentation is expanded on the
host, once per case.

``ResidentDataLoader3D`` does not serve the previous-stage channel: ``--resident_data`` together with this trainer is refused.
"""
import os
from os.path import isdir, isfile, join

import numpy as np

from ... import paths
from .nnUNetTrainer_simple import nnUNetTrainer_simple


def to_one_hot(seg, all_seg_labels):
    """[len(all_seg_labels), *seg.shape], seg's dtype: channel i is seg == all_seg_labels[i]"""
    result = np.zeros((len(all_seg_labels),) + tuple(seg.shape), dtype=seg.dtype)
    for i, l in enumerate(all_seg_labels):
        result[i][seg == l] = 1
    return result


class nnUNetTrainerV2CascadeFullRes(nnUNetTrainer_simple):
    def __init__(self, plans_file, fold, output_folder=None, dataset_directory=None, batch_dice=True, stage=None,
                 unpack_data=True, deterministic=True, fp16=False, Tconv=None, max_num_epochs=200,
                 num_batches_per_epoch=100, args=None, previous_trainer="nnUNetTrainerV2"):
        super().__init__(plans_file, fold, output_folder, dataset_directory, batch_dice, stage, unpack_data, deterministic,
                         fp16, Tconv, max_num_epochs, num_batches_per_epoch, args)
        self.previous_trainer = previous_trainer
        if self.output_folder is not None:
            # <results>/3d_cascade_fullres/<task>/<trainer>__<plans>/fold_X -> <results>/3d_lowres/<task>/<previous>__<plans>/pred_next_stage
            parts = os.path.normpath(self.output_folder).split(os.sep)
            task = parts[-3]
            plans_identifier = parts[-2].split("__")[-1]
            self.folder_with_segs_from_prev_stage = join(paths.network_training_output_dir, "3d_lowres", task,
                                                         previous_trainer + "__" + plans_identifier, "pred_next_stage")
        else:
            self.folder_with_segs_from_prev_stage = None

    def do_split(self):
        super().do_split()
        for k in self.dataset:
            self.dataset[k]['seg_from_prev_stage_file'] = join(self.folder_with_segs_from_prev_stage, k + "_segFromPrevStage.npz")
            assert isfile(self.dataset[k]['seg_from_prev_stage_file']), \
                "seg from prev stage missing: %s. " \
                "Please run all 5 folds of the 3d_lowres configuration of this " \
                "task!" % (self.dataset[k]['seg_from_prev_stage_file'])
        for d in (self.dataset_val, self.dataset_tr):
            for k in d:
                d[k]['seg_from_prev_stage_file'] = join(self.folder_with_segs_from_prev_stage, k + "_segFromPrevStage.npz")

    def get_basic_generators(self):
        if self.resident_data_gib is not None:
            raise NotImplementedError("--resident_data together with nnUNetTrainerV2CascadeFullRes: ResidentDataLoader3D does not "
                                      "serve the previous stage's segmentation; train this stage with the host loader")
        from ..dataloading.dataset_loading import DataLoader3D
        self.load_dataset()
        self.do_split()
        dl_tr = DataLoader3D(self.dataset_tr, self.basic_generator_patch_size, self.patch_size, self.batch_size, True,
                             oversample_foreground_percent=self.oversample_foreground_percent, pad_mode="constant",
                             pad_sides=self.pad_all_sides, memmap_mode='r')
        dl_val = DataLoader3D(self.dataset_val, self.patch_size, self.patch_size, self.batch_size, True,
                              oversample_foreground_percent=self.oversample_foreground_percent, pad_mode="constant",
                              pad_sides=self.pad_all_sides, memmap_mode='r')
        return dl_tr, dl_val

    def process_plans(self, plans):
        super().process_plans(plans)
        self.num_input_channels += (self.num_classes - 1)          # for seg from prev stage

    def setup_DA_params(self):
        super().setup_DA_params()
        p = self.data_aug_params
        p["num_cached_per_thread"] = 2
        p['move_last_seg_chanel_to_data'] = True
        p['cascade_do_cascade_augmentations'] = True
        p['cascade_random_binary_transform_p'] = 0.4
        p['cascade_random_binary_transform_p_per_label'] = 1
        p['cascade_random_binary_transform_size'] = (1, 8)
        p['cascade_remove_conn_comp_p'] = 0.2
        p['cascade_remove_conn_comp_max_size_percent_threshold'] = 0.15
        p['cascade_remove_conn_comp_fill_with_other_class_p'] = 0.0
        # two seg channels until the augmenter moves the previous stage's segmentation to the data
        p['selected_seg_channels'] = [0, 1]
        p['all_segmentation_labels'] = list(range(1, self.num_classes))

    def initialize(self, training=True, force_load_plans=False):
        if training and not self.was_initialized and self.tr_gen is None and not self.synthetic_data:
            if self.folder_with_segs_from_prev_stage is None or not isdir(self.folder_with_segs_from_prev_stage):
                raise RuntimeError("Cannot run final stage of cascade. Run corresponding 3d_lowres first and predict the "
                                   "segmentations for the next stage")
        return super().initialize(training, force_load_plans)

    def _validation_network_input(self, key, data):
        prev = np.load(join(self.folder_with_segs_from_prev_stage, key + "_segFromPrevStage.npz"))['data']
        assert tuple(prev.shape) == tuple(data.shape[1:]), \
            "seg from prev stage of %s has shape %s, the case %s" % (key, tuple(prev.shape), tuple(data.shape[1:]))
        return np.concatenate((data[:-1], to_one_hot(prev, list(range(1, self.num_classes))).astype(data.dtype)))
