"""The reference's e2enet/experiment_planning/DatasetAnalyzer.py on the device (csrc/fingerprint.hip): the dataset fingerprint of a
cropped folder, ``intensityproperties.pkl`` and ``dataset_properties.pkl`` with the reference's keys and nesting.

  DatasetAnalyzer (load_properties_of_cropped, get_classes, get_modalities, get_sizes_and_spacings_after_cropping,
                   get_size_reduction_by_cropping, _get_voxels_in_foreground, _compute_stats, collect_intensity_properties,
                   analyze_dataset)                                                                 :27-262, same names and arguments

A case's ``.npz`` is read and uploaded once for all modalities (the reference reads it once per modality); every tenth foreground
voxel is gathered on the device (e2e_fingerprint_sample_*), and the samples stay there: a case's seven numbers and the dataset's, over
the samples of all cases behind one another, come from e2e_fingerprint_stats and the rank rule of intensity_stats.py.  The two
percentiles follow that rule, not the bits of ``np.percentile`` on a list of fp32 scalars.  One process owns the GPU;
``num_processes`` (at most 16) host threads read and decompress the next cases meanwhile.  ``analyse_segmentations`` and the
region-size methods, which ``analyze_dataset`` never calls, are not part of this package.  There is no host fallback."""
import json
import os
import pickle
from collections import OrderedDict, deque

import numpy as np

from ..preprocessing.cropping import _device, _stream, get_patient_identifiers_from_cropped_files
from .intensity_stats import MAX_RANKS, STAT_NAMES, all_nan, requested_ranks, stats_from_order_statistics

DEFAULT_NUM_THREADS = 8              # reference e2enet/configuration.py
MAX_READER_THREADS = 16              # host threads that read cropped cases ahead (never sized from the machine)
FOREGROUND_STRIDE = 10               # reference :165: "no need to take every voxel"


def foreground_sample(all_data, stride=FOREGROUND_STRIDE):
    """``all_data[:-1][:, all_data[-1] > 0][:, ::stride]`` of a cropped case ``[C + 1, X, Y, Z]`` (seg last) as an fp32 device tensor
    ``[C, ceil(n_fg / stride)]``.  ``all_data``: an fp32 device tensor (it stays there) or a numpy array (uploaded once).  All
    modalities are gathered in one pass; a NaN in the seg is not foreground."""
    import torch
    from .._lib import lib, E2EError
    L = lib()
    if isinstance(all_data, torch.Tensor):
        if not all_data.is_cuda:
            raise ValueError("a tensor input must live on the device")
        dev = all_data.to(torch.float32).contiguous()
    else:
        dev = torch.from_numpy(np.ascontiguousarray(all_data, dtype=np.float32)).to(_device())
    assert dev.dim() >= 2 and dev.shape[0] >= 2, "a cropped case holds at least one modality and the seg"
    C = int(dev.shape[0]) - 1
    n = int(dev[0].numel())
    if n == 0:
        return torch.empty((C, 0), dtype=torch.float32, device=dev.device)
    nbytes = L.fingerprint_sample_ws_bytes(n)
    if nbytes <= 0:
        raise E2EError("fingerprint_sample_ws_bytes: a volume of %d voxels is not supported" % n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev.device)
    n_fg = torch.empty(1, dtype=torch.int64, device=dev.device)
    seg = dev[C]
    L.fingerprint_sample_count(seg.data_ptr(), n, n_fg.data_ptr(), ws.data_ptr(), _stream())
    out_len = -(-int(n_fg.item()) // int(stride))
    out = torch.empty((C, out_len), dtype=torch.float32, device=dev.device)
    L.fingerprint_sample_gather(dev.data_ptr(), seg.data_ptr(), C, n, int(stride), out.data_ptr(), out_len, ws.data_ptr(), _stream())
    return out


def order_statistics(values, ranks):
    """``(num_nan, min, max, sum, sum of (x - sum / n)**2, [sorted(values)[r] for r in ranks])`` of a flat fp32 device tensor with at
    least one element: fp64 sums, exact order statistics as stored (fp32); up to ``MAX_RANKS`` ranks in one call"""
    import torch
    from .._lib import lib
    L = lib()
    assert values.is_cuda and values.dtype == torch.float32 and values.dim() == 1 and values.is_contiguous()
    ranks = np.ascontiguousarray(ranks, dtype=np.int64)
    assert 1 <= len(ranks) <= min(MAX_RANKS, L.fingerprint_stats_max_ranks())
    ws = torch.empty(L.fingerprint_stats_ws_bytes(), dtype=torch.uint8, device=values.device)
    out = torch.empty(16, dtype=torch.float64, device=values.device)
    L.fingerprint_stats(values.data_ptr(), int(values.numel()), ranks.ctypes.data, len(ranks), out.data_ptr(), ws.data_ptr(), _stream())
    o = out.cpu().numpy()
    return int(o[0]), o[1], o[2], o[3], o[4], [np.float32(v) for v in o[8:8 + len(ranks)]]


def dataset_properties_dict(sizes, spacings, classes, modalities, intensityproperties, size_reductions):
    """Reference :253-259: the dict ``analyze_dataset`` pickles; ``classes`` is the ``labels`` entry of dataset.json"""
    dataset_properties = dict()
    dataset_properties['all_sizes'] = sizes
    dataset_properties['all_spacings'] = spacings
    dataset_properties['all_classes'] = [int(i) for i in classes.keys() if int(i) > 0]
    dataset_properties['modalities'] = modalities  # {idx: modality name}
    dataset_properties['intensityproperties'] = intensityproperties
    dataset_properties['size_reductions'] = size_reductions  # {patient_id: size_reduction}
    return dataset_properties


def intensity_properties_dict(patient_identifiers, global_stats, local_stats):
    """Reference :188-219: ``{modality: {'local_props': {case: {name: value}}, name: value}}`` from the seven numbers of the dataset
    (``global_stats[modality]``) and of every case (``local_stats[modality][i]``), each in ``_compute_stats`` order"""
    results = OrderedDict()
    for mod_id in range(len(global_stats)):
        results[mod_id] = OrderedDict()
        props_per_case = OrderedDict()
        for i, pat in enumerate(patient_identifiers):
            props_per_case[pat] = OrderedDict(zip(STAT_NAMES, local_stats[mod_id][i]))
        results[mod_id]['local_props'] = props_per_case
        for name, value in zip(STAT_NAMES, global_stats[mod_id]):
            results[mod_id][name] = value
    return results


class DatasetAnalyzer(object):
    """Reference :27-262"""

    def __init__(self, folder_with_cropped_data, overwrite=True, num_processes=DEFAULT_NUM_THREADS):
        """``overwrite=False`` reuses an existing ``intensityproperties.pkl`` (reference :28-43)"""
        self.num_processes = max(1, min(int(num_processes), MAX_READER_THREADS))
        self.overwrite = overwrite
        self.folder_with_cropped_data = folder_with_cropped_data
        self.sizes = self.spacings = None
        self.patient_identifiers = get_patient_identifiers_from_cropped_files(self.folder_with_cropped_data)
        assert os.path.isfile(os.path.join(self.folder_with_cropped_data, "dataset.json")), \
            "dataset.json needs to be in folder_with_cropped_data"
        self.props_per_case_file = os.path.join(self.folder_with_cropped_data, "props_per_case.pkl")
        self.intensityproperties_file = os.path.join(self.folder_with_cropped_data, "intensityproperties.pkl")

    def load_properties_of_cropped(self, case_identifier):
        with open(os.path.join(self.folder_with_cropped_data, "%s.pkl" % case_identifier), 'rb') as f:
            properties = pickle.load(f)
        return properties

    def _load_dataset_json(self):
        with open(os.path.join(self.folder_with_cropped_data, "dataset.json"), 'r') as f:
            return json.load(f)

    def get_classes(self):
        return self._load_dataset_json()['labels']

    def get_sizes_and_spacings_after_cropping(self):
        sizes = []
        spacings = []
        for c in self.patient_identifiers:
            properties = self.load_properties_of_cropped(c)
            sizes.append(properties["size_after_cropping"])
            spacings.append(properties["original_spacing"])
        return sizes, spacings

    def get_modalities(self):
        modalities = self._load_dataset_json()["modality"]
        modalities = {int(k): modalities[k] for k in modalities.keys()}
        return modalities

    def get_size_reduction_by_cropping(self):
        size_reduction = OrderedDict()
        for p in self.patient_identifiers:
            props = self.load_properties_of_cropped(p)
            shape_before_crop = props["original_size_of_raw_data"]
            shape_after_crop = props['size_after_cropping']
            size_red = np.prod(shape_after_crop) / np.prod(shape_before_crop)
            size_reduction[p] = size_red
        return size_reduction

    def _load_cropped(self, patient_identifier):
        return np.load(os.path.join(self.folder_with_cropped_data, patient_identifier) + ".npz")['data']

    def _get_voxels_in_foreground(self, patient_identifier, modality_id):
        """Reference :161-166: ``modality[seg > 0][::10]`` of one modality of a cropped case, as a numpy array (the reference makes a
        list of it).  collect_intensity_properties does not come through here: it samples all modalities of a case at once."""
        return foreground_sample(self._load_cropped(patient_identifier))[modality_id].cpu().numpy()

    @staticmethod
    def _compute_stats(voxels):
        """Reference :168-179: ``(median, mean, sd, mn, mx, percentile_99_5, percentile_00_5)`` of a sample, each an ``np.float32``
        (seven ``np.nan`` for an empty one).  ``voxels``: a flat fp32 device tensor (it stays there), or a numpy array or list
        (uploaded once)."""
        import torch
        if isinstance(voxels, torch.Tensor):
            if not voxels.is_cuda:
                raise ValueError("a tensor input must live on the device")
            dev = voxels.to(torch.float32).reshape(-1).contiguous()
        else:
            if len(voxels) == 0:
                return all_nan()
            dev = torch.from_numpy(np.ascontiguousarray(voxels, dtype=np.float32).reshape(-1)).to(_device())
        n = int(dev.numel())
        if n == 0:
            return all_nan()
        ranks = requested_ranks(n)
        num_nan, mn, mx, total, sq_dev, order = order_statistics(dev, ranks)
        return stats_from_order_statistics(n, num_nan, mn, mx, total, sq_dev, dict(zip(ranks, order)))

    def _foreground_samples(self):
        """one fp32 device tensor ``[C, m_case]`` per case, in case order; ``num_processes`` threads read the files ahead"""
        from concurrent.futures import ThreadPoolExecutor
        samples = []
        with ThreadPoolExecutor(max_workers=self.num_processes) as pool:
            pending, todo = deque(), deque(self.patient_identifiers)
            while todo or pending:
                while todo and len(pending) < self.num_processes:      # bounds the decompressed cases held in host memory
                    pending.append(pool.submit(self._load_cropped, todo.popleft()))
                samples.append(foreground_sample(pending.popleft().result()))
        return samples

    @staticmethod
    def _concatenate(parts):
        """the samples of all cases behind one another, on the device; a dataset too large for that raises, it is never moved to
        the host"""
        import torch
        try:
            return torch.cat(parts) if len(parts) > 1 else parts[0].contiguous()
        except torch.cuda.OutOfMemoryError as e:
            nbytes = 4 * sum(int(p.numel()) for p in parts)
            raise MemoryError("the foreground samples of one modality over the whole dataset need a device buffer of %d bytes, "
                              "which could not be allocated; there is no host fallback for the fingerprint" % nbytes) from e

    def collect_intensity_properties(self, num_modalities):
        """Reference :184-226"""
        if self.overwrite or not os.path.isfile(self.intensityproperties_file):
            samples = self._foreground_samples()
            global_stats, local_stats = [], []
            for mod_id in range(num_modalities):
                parts = [s[mod_id] for s in samples]
                local_stats.append([self._compute_stats(p) for p in parts])
                if sum(int(p.numel()) for p in parts) == 0:
                    global_stats.append(all_nan())
                    continue
                w = self._concatenate(parts)
                global_stats.append(self._compute_stats(w))
                del w
            results = intensity_properties_dict(self.patient_identifiers, global_stats, local_stats)
            with open(self.intensityproperties_file, 'wb') as f:
                pickle.dump(results, f)
        else:
            with open(self.intensityproperties_file, 'rb') as f:
                results = pickle.load(f)
        return results

    def analyze_dataset(self, collect_intensityproperties=True):
        """Reference :228-262: writes ``dataset_properties.pkl`` into the cropped folder and returns its dict"""
        sizes, spacings = self.get_sizes_and_spacings_after_cropping()
        classes = self.get_classes()
        modalities = self.get_modalities()
        if collect_intensityproperties:
            intensityproperties = self.collect_intensity_properties(len(modalities))
        else:
            intensityproperties = None
        size_reductions = self.get_size_reduction_by_cropping()
        dataset_properties = dataset_properties_dict(sizes, spacings, classes, modalities, intensityproperties, size_reductions)
        with open(os.path.join(self.folder_with_cropped_data, "dataset_properties.pkl"), 'wb') as f:
            pickle.dump(dataset_properties, f)
        return dataset_properties
