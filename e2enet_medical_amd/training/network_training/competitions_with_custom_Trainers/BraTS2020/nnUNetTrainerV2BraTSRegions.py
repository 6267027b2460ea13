"""Training on overlapping label regions (reference e2enet/training/network_training/competitions_with_custom_Trainers/BraTS2020/
nnUNetTrainerV2BraTSRegions.py:66-189) on the MI355X engine.

The network has one sigmoid output per region; the loss is MultipleOutputLoss2(DC_and_BCE_loss({}, batch_dice=False, do_bg=True,
smooth=0)), fused in ``e2e_dc_bce_reduce`` / ``e2e_dc_bce_grad``.  The reference converts the label map into R target channels
on the CPU (ConvertSegmentationToRegionsTransform) and ships those to the GPU; here the trainer's own generators keep yielding
the label map and the engine gets one 32-bit word per region, from which the kernels form the region targets on load.

Targets of a batch handed to ``run_iteration``:
  * one channel  -> always a label map (also when the trainer has a single region);
  * R > 1 channels -> multi-hot region targets, as the reference's transform yields them (a foreign generator built with
    ``get_moreDA_augmentation(..., regions=...)``);
  * anything else is refused (ValueError).

The ``_Dice``, ``_BN`` and ``_DDP`` variants of the reference are not built.
"""
import json

import numpy as np
from torch import nn

from .....evaluation.region_based_evaluation import evaluate_case, get_brats_regions
from ....data_augmentation.custom_transforms import region_label_sets, region_words
from ....loss_functions.dice_loss import DC_and_BCE_loss
from ...nnUNetTrainer_simple import nnUNetTrainer_simple


class nnUNetTrainerV2BraTSRegions(nnUNetTrainer_simple):
    def __init__(self, plans_file, fold, output_folder=None, dataset_directory=None, batch_dice=True, stage=None,
                 unpack_data=True, deterministic=True, fp16=False, Tconv=None, max_num_epochs=200,
                 num_batches_per_epoch=100, args=None):
        super().__init__(plans_file, fold, output_folder, dataset_directory, batch_dice, stage, unpack_data, deterministic,
                         fp16, Tconv, max_num_epochs, num_batches_per_epoch, args)
        self.regions = get_brats_regions()
        self.regions_class_order = (1, 2, 3)
        # reference :73: the constructor's batch_dice is recorded (init_args) and not used by the loss
        self.batch_dice = False
        self.loss_smooth = 0.
        self.loss = DC_and_BCE_loss({}, {'batch_dice': self.batch_dice, 'do_bg': True, 'smooth': self.loss_smooth})

    def process_plans(self, plans):
        super().process_plans(plans)
        self.num_classes = len(self.regions)          # the network has as many outputs as there are regions

    def initialize_network(self):
        super().initialize_network()
        self.network.inference_apply_nonlin = nn.Sigmoid()

    def _num_labels(self):
        return max(max(s) for s in region_label_sets(self.regions)) + 1

    def _engine_loss_kwargs(self):
        return {'smooth': self.loss_smooth, 'regions': region_words(self.regions)}

    def _online_eval_regions(self):
        return region_words(self.regions)

    def _online_eval_multi_hot(self, tgt, b, r, spatial):
        if r != len(self.regions):
            raise ValueError("%d output channels for %d regions" % (r, len(self.regions)))
        if tgt.numel() == b * spatial:
            return False
        if r > 1 and tgt.numel() == b * r * spatial:
            return True
        raise ValueError("target must be a label map [B,1,...] or multi-hot [B,%d,...] over the logits' voxels" % r)

    def _validation_extra(self, cases, summary_file):
        """reference :155-166 runs evaluate_regions over the exported folder; here the Dice per region of every case and the
        means over the cases (nan = region empty in prediction and ground truth, left out of the mean) go into summary.json
        as results["regions"], keyed by the region names."""
        names = list(self.regions.keys())
        rows = []
        for seg, gt, pred_file, gt_file in cases:
            dcs = evaluate_case(seg, gt, self.regions)
            row = {n: float(d) for n, d in zip(names, dcs)}
            row["test"], row["reference"] = pred_file, gt_file
            rows.append(row)
        mean = {}
        for n in names:
            vals = [r[n] for r in rows if not np.isnan(r[n])]
            mean[n] = float(np.mean(vals)) if vals else float("nan")
        with open(summary_file) as f:
            summary = json.load(f)
        summary["results"]["regions"] = {"all": rows, "mean": mean}
        with open(summary_file, "w") as f:
            json.dump(summary, f, indent=4, sort_keys=True)
        self.print_to_log_file("region Dice (mean over the validation cases):", mean)
