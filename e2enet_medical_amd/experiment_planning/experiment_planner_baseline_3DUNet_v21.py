"""``ExperimentPlanner3D_v21``, the planner the command uses by default (the reference's
e2enet/experiment_planning/experiment_planner_baseline_3DUNet_v21.py:24-184): plans file ``nnUNetPlansv2.1_plans_3D.pkl``, data
identifier ``nnUNetData_plans_v2.1``, 32 base features.  It differs from ``ExperimentPlanner`` in three places: the target spacing of a
thick-slice dataset, pooling by spacing instead of pooling late, and a patch budget scaled by 32 / 30."""
import os

import numpy as np

from ..network_architecture.generic_UNet import Generic_UNet
from .common_utils import get_pool_and_conv_props
from .experiment_planner_baseline_3DUNet import ExperimentPlanner


class ExperimentPlanner3D_v21(ExperimentPlanner):
    def __init__(self, folder_with_cropped_data, preprocessed_output_folder):
        super(ExperimentPlanner3D_v21, self).__init__(folder_with_cropped_data, preprocessed_output_folder)
        self.data_identifier = "nnUNetData_plans_v2.1"
        self.plans_fname = os.path.join(self.preprocessed_output_folder, "nnUNetPlansv2.1_plans_3D.pkl")
        self.unet_base_num_features = 32

    def get_target_spacing(self):
        """The median spacing -- except for a dataset whose coarsest axis is more than 3 times coarser than the others and has fewer
        than a third of their voxels (thick slices): resampling such an axis to its median would interpolate across few slices, so it
        gets the 10th percentile of its spacings instead, but never a spacing finer than the other axes (then: theirs + 1e-5)."""
        spacings = self.dataset_properties['all_spacings']
        sizes = self.dataset_properties['all_sizes']
        target = np.percentile(np.vstack(spacings), self.target_spacing_percentile, 0)
        target_size = np.percentile(np.vstack(sizes), self.target_spacing_percentile, 0)

        worst_spacing_axis = np.argmax(target)
        other_axes = [i for i in range(len(target)) if i != worst_spacing_axis]
        other_spacings = [target[i] for i in other_axes]
        other_sizes = [target_size[i] for i in other_axes]
        has_aniso_spacing = target[worst_spacing_axis] > (self.anisotropy_threshold * max(other_spacings))
        has_aniso_voxels = target_size[worst_spacing_axis] * self.anisotropy_threshold < min(other_sizes)
        if has_aniso_spacing and has_aniso_voxels:
            spacings_of_that_axis = np.vstack(spacings)[:, worst_spacing_axis]
            target_spacing_of_that_axis = np.percentile(spacings_of_that_axis, 10)
            if target_spacing_of_that_axis < max(other_spacings):
                target_spacing_of_that_axis = max(max(other_spacings), target_spacing_of_that_axis) + 1e-5
            target[worst_spacing_axis] = target_spacing_of_that_axis
        return target

    # get_properties_for_stage is the base class's walk; the reference's override differs from it in these two places only
    def _pool_and_conv_props(self, spacing, patch_size):
        """pool by spacing"""
        return get_pool_and_conv_props(spacing, patch_size, self.unet_featuremap_min_edge_length, self.unet_max_numpool)

    def _reference_vram(self):
        """the stock budget was found with 30 base features: scaled to this planner's 32"""
        return Generic_UNet.use_this_for_batch_size_computation_3D * self.unet_base_num_features / Generic_UNet.BASE_NUM_FEATURES_3D
