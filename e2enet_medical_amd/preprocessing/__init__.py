"""Preprocessing on the device (csrc/preprocess.hip, class_select.hip): the reference's e2enet/preprocessing/cropping.py and
preprocessing.py (GenericPreprocessor) with their names and signatures, for a case in memory and for a cropped training folder."""
from .class_sampling import draw_class_ranks, target_num_samples
from .cropping import (ImageCropper, create_nonzero_mask, crop_to_bbox, crop_to_nonzero, default_reader, get_bbox_from_mask,
                       get_case_identifier, get_patient_identifiers_from_cropped_files, load_case_from_list_of_files)
from .preprocessing import (GenericPreprocessor, GenericPreprocessor_linearResampling, RESAMPLING_SEPARATE_Z_ANISO_THRESHOLD,
                            class_locations, get_do_separate_z, get_lowres_axis, resample_data_or_seg, resample_patient,
                            run_preprocessing)
