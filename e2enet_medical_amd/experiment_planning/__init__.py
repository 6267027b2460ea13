"""The dataset fingerprint on the device (csrc/fingerprint.hip): the reference's e2enet/experiment_planning/DatasetAnalyzer.py and the
cropping and fingerprint entry points of experiment_planning/utils.py, with their names and signatures.  The experiment planner is
not part of this package."""
from .DatasetAnalyzer import DatasetAnalyzer
from .utils import analyze_dataset, create_lists_from_splitted_dataset, crop
