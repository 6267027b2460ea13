"""``ExperimentPlanner``: a cropped folder's fingerprint (``dataset_properties.pkl``) into the 3-D plans file -- target spacing, patch
size, pooling layout, batch size, normalisation schemes, transposes, one or two stages.  The reference's
e2enet/experiment_planning/experiment_planner_baseline_3DUNet.py:32-445 under the reference's names; this base class pools late
(``get_pool_and_conv_props_poolLateV2``) and writes ``nnUNetPlansfixed_plans_3D.pkl``.  ``ExperimentPlanner3D_v21`` (the default of the
command) derives from it.

Everything here is deterministic fp64 / integer numpy arithmetic on a handful of numbers, kept in the reference's order of operations
(the percentiles of ``np.vstack``, the ``*= 1.01`` walk of the lowres spacing, the rounding of the median shape): the plans dict equals
the reference's value for value and type for type, and the pickled file loads in the reference as it is.  The patch is sized with the
stock U-Net's estimate (``network_architecture/generic_UNet.py``), as in the reference.  ``determine_postprocessing`` (deprecated
there, a no-op) is not part of this package."""
import os
import pickle
from collections import OrderedDict
from copy import deepcopy

import numpy as np

from ..network_architecture.generic_UNet import Generic_UNet
from ..paths import default_data_identifier
from ..preprocessing.preprocessing import run_preprocessing
from .common_utils import get_pool_and_conv_props_poolLateV2


def get_case_identifier_from_npz(case):
    """e2enet/preprocessing/cropping.py:56-58"""
    return case.split("/")[-1][:-4]


class ExperimentPlanner(object):
    def __init__(self, folder_with_cropped_data, preprocessed_output_folder):
        self.folder_with_cropped_data = folder_with_cropped_data
        self.preprocessed_output_folder = preprocessed_output_folder
        # (full paths, sorted: the list goes into the plans as it is)
        self.list_of_cropped_npz_files = sorted(os.path.join(folder_with_cropped_data, f) for f in os.listdir(folder_with_cropped_data)
                                                if f.endswith(".npz") and os.path.isfile(os.path.join(folder_with_cropped_data, f)))
        self.preprocessor_name = "GenericPreprocessor"
        fingerprint = os.path.join(self.folder_with_cropped_data, "dataset_properties.pkl")
        assert os.path.isfile(fingerprint), "folder_with_cropped_data must contain dataset_properties.pkl"
        with open(fingerprint, 'rb') as f:
            self.dataset_properties = pickle.load(f)

        self.plans_per_stage = OrderedDict()
        self.plans = OrderedDict()
        self.plans_fname = os.path.join(self.preprocessed_output_folder, "nnUNetPlans" + "fixed_plans_3D.pkl")
        self.data_identifier = default_data_identifier

        self.transpose_forward = [0, 1, 2]
        self.transpose_backward = [0, 1, 2]

        self.unet_base_num_features = Generic_UNet.BASE_NUM_FEATURES_3D
        self.unet_max_num_filters = 320
        self.unet_max_numpool = 999
        self.unet_min_batch_size = 2
        self.unet_featuremap_min_edge_length = 4

        self.target_spacing_percentile = 50
        self.anisotropy_threshold = 3
        self.how_much_of_a_patient_must_the_network_see_at_stage0 = 4      # a patch of the lowres stage covers 1/4 of the median case
        self.batch_size_covers_max_percent_of_dataset = 0.05               # one batch holds at most 5 % of the dataset's voxels
        self.conv_per_stage = 2

    # ------------------------------------------------------------------------------------------------------------- plans file
    def save_my_plans(self):
        with open(self.plans_fname, 'wb') as f:
            pickle.dump(self.plans, f)

    def load_my_plans(self):
        with open(self.plans_fname, 'rb') as f:
            self.plans = pickle.load(f)
        self.plans_per_stage = self.plans['plans_per_stage']
        self.dataset_properties = self.plans['dataset_properties']
        self.transpose_forward = self.plans['transpose_forward']
        self.transpose_backward = self.plans['transpose_backward']

    def load_properties_of_cropped(self, case_identifier):
        with open(os.path.join(self.folder_with_cropped_data, "%s.pkl" % case_identifier), 'rb') as f:
            return pickle.load(f)

    def save_properties_of_cropped(self, case_identifier, properties):
        with open(os.path.join(self.folder_with_cropped_data, "%s.pkl" % case_identifier), 'wb') as f:
            pickle.dump(properties, f)

    # --------------------------------------------------------------------------------------------------------------- planning
    def get_target_spacing(self):
        """the median spacing of the dataset, axis by axis"""
        return np.percentile(np.vstack(self.dataset_properties['all_spacings']), self.target_spacing_percentile, 0)

    def _pool_and_conv_props(self, spacing, patch_size):
        """the pooling layout of this planner: pool late"""
        return get_pool_and_conv_props_poolLateV2(patch_size, self.unet_featuremap_min_edge_length, self.unet_max_numpool, spacing)

    def _reference_vram(self):
        """what the estimate of a patch may reach"""
        return Generic_UNet.use_this_for_batch_size_computation_3D

    def _approx_vram(self, patch_size, num_pool_per_axis, num_modalities, num_classes, pool_op_kernel_sizes):
        return Generic_UNet.compute_approx_vram_consumption(patch_size, num_pool_per_axis, self.unet_base_num_features,
                                                            self.unet_max_num_filters, num_modalities, num_classes,
                                                            pool_op_kernel_sizes, conv_per_stage=self.conv_per_stage)

    def get_properties_for_stage(self, current_spacing, original_spacing, original_shape, num_cases, num_modalities, num_classes):
        """One stage's plan.  The patch starts as 512 mm along the finest axis with the aspect of the spacing (an isotropic field of
        view in millimetres), clipped to the median case at this spacing and padded to what the pooling needs; while the stock
        U-Net's estimate exceeds the budget, the axis that is largest relative to the median case loses one divisor and the layout is
        derived again.  The batch grows from 2 by what the budget leaves, capped at 5 % of the dataset's voxels (never below 2)."""
        new_median_shape = np.round(original_spacing / current_spacing * original_shape).astype(int)
        dataset_num_voxels = np.prod(new_median_shape) * num_cases

        input_patch_size = 1 / np.array(current_spacing)          # voxels per millimetre
        input_patch_size /= input_patch_size.mean()
        input_patch_size *= 1 / min(input_patch_size) * 512
        input_patch_size = np.round(input_patch_size).astype(int)
        input_patch_size = [min(i, j) for i, j in zip(input_patch_size, new_median_shape)]

        num_pool_per_axis, pool_op_kernel_sizes, conv_kernel_sizes, new_shp, shape_must_be_divisible_by = \
            self._pool_and_conv_props(current_spacing, input_patch_size)

        ref = self._reference_vram()
        here = self._approx_vram(new_shp, num_pool_per_axis, num_modalities, num_classes, pool_op_kernel_sizes)
        while here > ref:
            axis_to_be_reduced = np.argsort(new_shp / new_median_shape)[-1]
            # the divisor the shrunken patch would need may be smaller than the current one: ask for it first
            tmp = deepcopy(new_shp)
            tmp[axis_to_be_reduced] -= shape_must_be_divisible_by[axis_to_be_reduced]
            shape_must_be_divisible_by_new = self._pool_and_conv_props(current_spacing, tmp)[4]
            new_shp[axis_to_be_reduced] -= shape_must_be_divisible_by_new[axis_to_be_reduced]
            num_pool_per_axis, pool_op_kernel_sizes, conv_kernel_sizes, new_shp, shape_must_be_divisible_by = \
                self._pool_and_conv_props(current_spacing, new_shp)
            here = self._approx_vram(new_shp, num_pool_per_axis, num_modalities, num_classes, pool_op_kernel_sizes)
        input_patch_size = new_shp

        batch_size = Generic_UNet.DEFAULT_BATCH_SIZE_3D
        batch_size = int(np.floor(max(ref / here, 1) * batch_size))
        max_batch_size = np.round(self.batch_size_covers_max_percent_of_dataset * dataset_num_voxels /
                                  np.prod(input_patch_size, dtype=np.int64)).astype(int)
        max_batch_size = max(max_batch_size, self.unet_min_batch_size)
        batch_size = max(1, min(batch_size, max_batch_size))

        do_dummy_2D_data_aug = (max(input_patch_size) / input_patch_size[0]) > self.anisotropy_threshold

        return {
            'batch_size': batch_size,
            'num_pool_per_axis': num_pool_per_axis,
            'patch_size': input_patch_size,
            'median_patient_size_in_voxels': new_median_shape,
            'current_spacing': current_spacing,
            'original_spacing': original_spacing,
            'do_dummy_2D_data_aug': do_dummy_2D_data_aug,
            'pool_op_kernel_sizes': pool_op_kernel_sizes,
            'conv_kernel_sizes': conv_kernel_sizes,
        }

    def plan_experiment(self):
        use_nonzero_mask_for_normalization = self.determine_whether_to_use_mask_for_norm()
        print("Are we using the nonzero mask for normalization?", use_nonzero_mask_for_normalization)
        spacings = self.dataset_properties['all_spacings']
        sizes = self.dataset_properties['all_sizes']
        all_classes = self.dataset_properties['all_classes']
        modalities = self.dataset_properties['modalities']
        num_modalities = len(list(modalities.keys()))
        num_cases = len(self.list_of_cropped_npz_files)

        target_spacing = self.get_target_spacing()
        new_shapes = [np.array(i) / target_spacing * np.array(j) for i, j in zip(spacings, sizes)]

        # the coarsest axis goes first
        max_spacing_axis = np.argmax(target_spacing)
        remaining_axes = [i for i in list(range(3)) if i != max_spacing_axis]
        self.transpose_forward = [max_spacing_axis] + remaining_axes
        self.transpose_backward = [np.argwhere(np.array(self.transpose_forward) == i)[0][0] for i in range(3)]

        median_shape = np.median(np.vstack(new_shapes), 0)
        print("the median shape of the dataset is ", median_shape)
        max_shape = np.max(np.vstack(new_shapes), 0)
        print("the max shape in the dataset is ", max_shape)
        min_shape = np.min(np.vstack(new_shapes), 0)
        print("the min shape in the dataset is ", min_shape)
        print("we don't want feature maps smaller than ", self.unet_featuremap_min_edge_length, " in the bottleneck")

        self.plans_per_stage = list()
        target_spacing_transposed = np.array(target_spacing)[self.transpose_forward]
        median_shape_transposed = np.array(median_shape)[self.transpose_forward]
        print("the transposed median shape of the dataset is ", median_shape_transposed)

        print("generating configuration for 3d_fullres")
        self.plans_per_stage.append(self.get_properties_for_stage(target_spacing_transposed, target_spacing_transposed,
                                                                  median_shape_transposed, num_cases, num_modalities,
                                                                  len(all_classes) + 1))

        # a lowres stage only when the fullres patch sees less than a quarter of the median case
        architecture_input_voxels_here = np.prod(self.plans_per_stage[-1]['patch_size'], dtype=np.int64)
        more = not (np.prod(median_shape) / architecture_input_voxels_here <
                    self.how_much_of_a_patient_must_the_network_see_at_stage0)
        if more:
            print("generating configuration for 3d_lowres")
            # coarsen in steps of 1 % -- the axes finer than half the coarsest one first, then all -- until the stage's patch covers
            # a quarter of the median case; every step plans the stage anew, because the patch changes with the spacing
            lowres_stage_spacing = deepcopy(target_spacing)
            num_voxels = np.prod(median_shape, dtype=np.float64)
            while num_voxels > self.how_much_of_a_patient_must_the_network_see_at_stage0 * architecture_input_voxels_here:
                max_spacing = max(lowres_stage_spacing)
                if np.any((max_spacing / lowres_stage_spacing) > 2):
                    lowres_stage_spacing[(max_spacing / lowres_stage_spacing) > 2] *= 1.01
                else:
                    lowres_stage_spacing *= 1.01
                num_voxels = np.prod(target_spacing / lowres_stage_spacing * median_shape, dtype=np.float64)

                lowres_stage_spacing_transposed = np.array(lowres_stage_spacing)[self.transpose_forward]
                new = self.get_properties_for_stage(lowres_stage_spacing_transposed, target_spacing_transposed,
                                                    median_shape_transposed, num_cases, num_modalities, len(all_classes) + 1)
                architecture_input_voxels_here = np.prod(new['patch_size'], dtype=np.int64)
            # kept only when it has less than half the voxels of the fullres stage
            if 2 * np.prod(new['median_patient_size_in_voxels'], dtype=np.int64) < np.prod(
                    self.plans_per_stage[0]['median_patient_size_in_voxels'], dtype=np.int64):
                self.plans_per_stage.append(new)

        self.plans_per_stage = self.plans_per_stage[::-1]
        self.plans_per_stage = {i: self.plans_per_stage[i] for i in range(len(self.plans_per_stage))}

        print(self.plans_per_stage)
        print("transpose forward", self.transpose_forward)
        print("transpose backward", self.transpose_backward)

        normalization_schemes = self.determine_normalization_scheme()
        # (the three post-processing entries are None in the reference too: its training-data based post-processing is gone)
        self.plans = {'num_stages': len(list(self.plans_per_stage.keys())), 'num_modalities': num_modalities,
                      'modalities': modalities, 'normalization_schemes': normalization_schemes,
                      'dataset_properties': self.dataset_properties, 'list_of_npz_files': self.list_of_cropped_npz_files,
                      'original_spacings': spacings, 'original_sizes': sizes,
                      'preprocessed_data_folder': self.preprocessed_output_folder, 'num_classes': len(all_classes),
                      'all_classes': all_classes, 'base_num_features': self.unet_base_num_features,
                      'use_mask_for_norm': use_nonzero_mask_for_normalization,
                      'keep_only_largest_region': None, 'min_region_size_per_class': None, 'min_size_per_class': None,
                      'transpose_forward': self.transpose_forward, 'transpose_backward': self.transpose_backward,
                      'data_identifier': self.data_identifier, 'plans_per_stage': self.plans_per_stage,
                      'preprocessor_name': self.preprocessor_name,
                      'conv_per_stage': self.conv_per_stage,
                      }
        self.save_my_plans()

    def determine_normalization_scheme(self):
        """per modality: "CT" for CT / ct, "noNorm" for noNorm, "nonCT" for everything else"""
        modalities = self.dataset_properties['modalities']
        schemes = OrderedDict()
        for i in range(len(list(modalities.keys()))):
            if modalities[i] in ("CT", "ct"):
                schemes[i] = "CT"
            elif modalities[i] == 'noNorm':
                schemes[i] = "noNorm"
            else:
                schemes[i] = "nonCT"
        return schemes

    def determine_whether_to_use_mask_for_norm(self):
        """Per modality, whether to normalise inside the nonzero mask only: never for a CT; otherwise when cropping to the nonzero
        region took more than a quarter of the median case away (brain MRI and the like).  The decision is also written into every
        cropped ``<case>.pkl`` (``use_nonzero_mask_for_norm``), where the preprocessor reads it."""
        modalities = self.dataset_properties['modalities']
        use_nonzero_mask_for_norm = OrderedDict()
        for i in range(len(list(modalities.keys()))):
            if "CT" in modalities[i]:
                use_nonzero_mask_for_norm[i] = False
                continue
            all_size_reductions = list(self.dataset_properties['size_reductions'].values())
            if np.median(all_size_reductions) < 3 / 4.:
                print("using nonzero mask for normalization")
                use_nonzero_mask_for_norm[i] = True
            else:
                print("not using nonzero mask for normalization")
                use_nonzero_mask_for_norm[i] = False
        self._write_mask_decision(use_nonzero_mask_for_norm)
        return use_nonzero_mask_for_norm

    def _write_mask_decision(self, use_nonzero_mask_for_norm):
        for c in self.list_of_cropped_npz_files:
            case_identifier = get_case_identifier_from_npz(c)
            properties = self.load_properties_of_cropped(case_identifier)
            properties['use_nonzero_mask_for_norm'] = use_nonzero_mask_for_norm
            self.save_properties_of_cropped(case_identifier, properties)

    def write_normalization_scheme_to_patients(self):
        """the plans' decision into every cropped ``<case>.pkl`` (for a test set cropped after planning)"""
        self._write_mask_decision(self.plans['use_mask_for_norm'])

    # ---------------------------------------------------------------------------------------------------------- preprocessing
    def run_preprocessing(self, num_threads, device_deflate=False):
        """``gt_segmentations`` copied and every stage preprocessed on the device (``preprocessing.run_preprocessing``, which holds the
        reference's handling of ``num_threads``: one number, or (lowres, fullres), and says what ``device_deflate`` does)"""
        run_preprocessing(self.plans, self.folder_with_cropped_data, self.preprocessed_output_folder, num_threads,
                          device_deflate=device_deflate)
