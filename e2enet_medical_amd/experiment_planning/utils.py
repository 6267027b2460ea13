"""The reference's e2enet/experiment_planning/utils.py, the legs in front of the planner:

  create_lists_from_splitted_dataset   :82-97
  crop                                 :122-135, with a ``reader`` argument for the image files
  analyze_dataset                      :138-141

Folders come from paths.py.  ``split_4d`` and ``plan_and_preprocess`` are not part of this package."""
import json
import os
import shutil

from .. import paths
from ..preprocessing.cropping import ImageCropper
from .DatasetAnalyzer import DEFAULT_NUM_THREADS, DatasetAnalyzer


def create_lists_from_splitted_dataset(base_folder_splitted):
    """Reference :82-97: ``([[imagesTr/<case>_0000.nii.gz, ..., labelsTr/<case>.nii.gz], ...], {index: modality name})`` from the
    ``training`` and ``modality`` entries of the folder's dataset.json"""
    lists = []
    json_file = os.path.join(base_folder_splitted, "dataset.json")
    with open(json_file) as jsn:
        d = json.load(jsn)
        training_files = d['training']
    num_modalities = len(d['modality'].keys())
    for tr in training_files:
        cur_pat = []
        for mod in range(num_modalities):
            cur_pat.append(os.path.join(base_folder_splitted, "imagesTr", tr['image'].split("/")[-1][:-7] + "_%04.0d.nii.gz" % mod))
        cur_pat.append(os.path.join(base_folder_splitted, "labelsTr", tr['label'].split("/")[-1]))
        lists.append(cur_pat)
    return lists, {int(i): d['modality'][str(i)] for i in d['modality'].keys()}


def crop(task_string, override=False, num_threads=DEFAULT_NUM_THREADS, reader=None, device_deflate=False):
    """Reference :122-135: ``<nnUNet_raw_data>/<task>`` into ``<nnUNet_cropped_data>/<task>``; ``override`` empties that folder first
    and crops every case again.  ``reader``: see preprocessing/cropping.py (default: the SimpleITK loader).  ``device_deflate``: see
    ``ImageCropper.run_cropping``."""
    cropped_out_dir = os.path.join(paths.nnUNet_cropped_data, task_string)
    os.makedirs(cropped_out_dir, exist_ok=True)
    if override and os.path.isdir(cropped_out_dir):
        shutil.rmtree(cropped_out_dir)
        os.makedirs(cropped_out_dir, exist_ok=True)
    splitted_4d_output_dir_task = os.path.join(paths.nnUNet_raw_data, task_string)
    lists, _ = create_lists_from_splitted_dataset(splitted_4d_output_dir_task)
    imgcrop = ImageCropper(num_threads, cropped_out_dir)
    imgcrop.run_cropping(lists, overwrite_existing=override, reader=reader, device_deflate=device_deflate)
    shutil.copy(os.path.join(paths.nnUNet_raw_data, task_string, "dataset.json"), cropped_out_dir)


def analyze_dataset(task_string, override=False, collect_intensityproperties=True, num_processes=DEFAULT_NUM_THREADS):
    """Reference :138-141"""
    cropped_out_dir = os.path.join(paths.nnUNet_cropped_data, task_string)
    dataset_analyzer = DatasetAnalyzer(cropped_out_dir, overwrite=override, num_processes=num_processes)
    _ = dataset_analyzer.analyze_dataset(collect_intensityproperties)
