"""The dataset fingerprint on the device (csrc/fingerprint.hip): the reference's e2enet/experiment_planning/DatasetAnalyzer.py and the
cropping and fingerprint entry points of experiment_planning/utils.py, with their names and signatures; and the experiment planner
(host arithmetic: common_utils.py, experiment_planner_baseline_3DUNet.py, experiment_planner_baseline_3DUNet_v21.py) with the
reference's command, nnUNet_plan_and_preprocess.py."""
from .DatasetAnalyzer import DatasetAnalyzer
from .utils import analyze_dataset, create_lists_from_splitted_dataset, crop
