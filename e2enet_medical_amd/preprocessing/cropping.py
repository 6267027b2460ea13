"""The reference's e2enet/preprocessing/cropping.py on the device (csrc/preprocess.hip): non-zero mask with filled holes, its
bounding box and the crop, in memory or from a raw task folder into a cropped folder.

  create_nonzero_mask, get_bbox_from_mask, crop_to_bbox, crop_to_nonzero   :23-116, same names, arguments and return values
  ImageCropper.crop, ImageCropper.crop_from_list_of_files                  :139-155
  ImageCropper.load_crop_save, run_cropping, load_properties, ...          :157-217, with a ``reader`` argument
  get_patient_identifiers_from_cropped_files                               :119-120
  load_case_from_list_of_files                                             :61-81, the default ``reader``

Arrays are numpy arrays or device tensors; a numpy array is uploaded once and the results come back as numpy arrays, a device
tensor stays on the device.  Files are read by a ``reader(list_of_files) -> (data [C, X, Y, Z], properties)`` callback, the
counterpart of the ``writer`` of ``predict_cases``; the default is the reference's SimpleITK loader when SimpleITK is importable.
There is no host fallback for the arithmetic: without the library or a device these functions raise."""
import os
import pickle
import shutil
from collections import OrderedDict, deque

import numpy as np

MAX_WRITER_THREADS = 16              # host threads that compress and write finished cases (never sized from the machine)


def _device():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("preprocessing runs on the GPU (csrc/preprocess.hip); there is no host fallback")
    return torch.device("cuda")


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def to_device(a, dtype=None):
    """(contiguous device tensor, was_numpy)"""
    import torch
    dtype = torch.float32 if dtype is None else dtype
    if isinstance(a, torch.Tensor):
        if not a.is_cuda:
            raise ValueError("a tensor input must live on the device")
        return a.to(dtype).contiguous(), False
    return torch.from_numpy(np.ascontiguousarray(a)).to(_device()).to(dtype), True


def _nonzero_mask_device(data):
    """uint8 device mask [X, Y, Z] of a contiguous fp32 device tensor [C, X, Y, Z] (or [C, X, Y])"""
    import torch
    from .._lib import lib, E2EError
    L = lib()
    shape = tuple(int(v) for v in data.shape[1:])
    D, H, W = (1,) * (3 - len(shape)) + shape
    nbytes = L.pp_nonzero_ws_bytes(D, H, W)
    if nbytes <= 0:
        raise E2EError("pp_nonzero_ws_bytes: a volume of %d x %d x %d is not supported (more than 2^31 - 2 voxels)" % (D, H, W))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=data.device)
    mask = torch.empty((D, H, W), dtype=torch.uint8, device=data.device)
    result = torch.zeros(8, dtype=torch.int32, device=data.device)
    L.pp_nonzero_mask(data.data_ptr(), int(data.shape[0]), D, H, W, mask.data_ptr(), ws.data_ptr(), result.data_ptr(), _stream())
    return mask.reshape(shape), result


def _check_giveup(words):
    from .._lib import E2EError
    if int(words[6]) != 0:
        raise E2EError("pp_nonzero_mask gave up: the union-find met a broken link or spent its step budget")


def _bbox_device(mask, outside_value, result):
    """[[lo, hi), ...] of a uint8 device mask; ``result``: the call's 8 device words (one download, give-up word included)"""
    from .._lib import lib
    shape = tuple(int(v) for v in mask.shape)
    D, H, W = (1,) * (3 - len(shape)) + shape
    lib().pp_bbox(mask.data_ptr(), int(outside_value), D, H, W, result.data_ptr(), _stream())
    words = result.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    _check_giveup(words)
    if words[7] == 0:
        raise ValueError("the mask has no voxel != %r: the case is empty and has no bounding box" % (outside_value,))
    box = [[int(words[2 * a]), int(words[2 * a + 1])] for a in range(3)]
    return box[3 - len(shape):]


def create_nonzero_mask(data):
    """Reference :23-31: OR over the modalities of ``data != 0`` (a NaN is non-zero), then ``scipy.ndimage.binary_fill_holes``.
    Returns a bool numpy array for a numpy input, a bool device tensor for a device tensor."""
    assert len(data.shape) == 4 or len(data.shape) == 3, "data must have shape (C, X, Y, Z) or shape (C, X, Y)"
    dev, was_numpy = to_device(data)
    mask, result = _nonzero_mask_device(dev)
    _check_giveup(result.cpu().numpy())
    return mask.cpu().numpy().astype(bool) if was_numpy else mask.bool()


def get_bbox_from_mask(mask, outside_value=0):
    """Reference :34-42: ``[[lo, hi), ...]`` of the voxels ``mask != outside_value``.  An empty mask raises ValueError (the
    reference dies in ``np.min`` of an empty array)."""
    import torch
    if isinstance(mask, torch.Tensor) and mask.dtype in (torch.uint8, torch.bool) and outside_value in (0, 1):
        dev, outside_value = mask.to(torch.uint8).contiguous(), int(outside_value)
    elif isinstance(mask, torch.Tensor):
        dev, outside_value = (mask != outside_value).to(torch.uint8).contiguous(), 0
    else:
        dev, outside_value = torch.from_numpy(np.ascontiguousarray(np.asarray(mask) != outside_value).astype(np.uint8)).to(_device()), 0
    return _bbox_device(dev, outside_value, torch.zeros(8, dtype=torch.int32, device=dev.device))


def crop_to_bbox(image, bbox):
    """Reference :45-48 (a view, like the reference's)"""
    assert len(image.shape) == 3, "only supports 3d images"
    return image[tuple(slice(bbox[a][0], bbox[a][1]) for a in range(3))]


def crop_to_nonzero(data, seg=None, nonzero_label=-1):
    """Reference :84-116: crop ``data`` [C, X, Y, Z] (and ``seg`` [S, X, Y, Z]) to the bounding box of the non-zero mask; the seg gets
    ``nonzero_label`` where it is 0 and the mask is off; without a seg, the returned seg is ``nonzero_label`` off the mask and 0 on it.
    Returns ``(data, seg, bbox)``: numpy arrays for numpy inputs (the made-up seg is an integer array like the reference's), fp32
    device tensors for device tensors.  An all-zero case raises ValueError."""
    import torch
    from .._lib import lib
    assert len(data.shape) == 4, "data must have shape (C, X, Y, Z)"
    dev, was_numpy = to_device(data)
    sdev = None
    if seg is not None:
        assert tuple(seg.shape[1:]) == tuple(data.shape[1:]), "seg must have shape (S, X, Y, Z) on the data's grid"
        sdev, _ = to_device(seg)
    mask, result = _nonzero_mask_device(dev)
    bbox = _bbox_device(mask, 0, result)
    C, D, H, W = (int(v) for v in dev.shape)
    d, h, w = (b[1] - b[0] for b in bbox)
    S = int(sdev.shape[0]) if sdev is not None else 1
    out = torch.empty((C, d, h, w), dtype=torch.float32, device=dev.device)
    out_seg = torch.empty((S, d, h, w), dtype=torch.float32, device=dev.device)
    lib().pp_crop(dev.data_ptr(), sdev.data_ptr() if sdev is not None else None, mask.data_ptr(), out.data_ptr(), out_seg.data_ptr(),
                  C, S, D, H, W, bbox[0][0], bbox[1][0], bbox[2][0], d, h, w, float(nonzero_label), _stream())
    if was_numpy:
        s = out_seg.cpu().numpy()
        return out.cpu().numpy(), (s.astype(seg.dtype) if seg is not None else s.astype(int)), bbox
    return out, out_seg, bbox


def label_values(seg, fix_below=False):
    """``np.unique`` of a device fp32 seg that holds whole-number labels in [-256, 255], from a device histogram (one download of
    513 words); ``fix_below`` also writes ``seg[seg < -1] = 0`` in place."""
    import torch
    from .._lib import lib
    L = lib()
    bins = L.pp_label_hist_bins()
    hist = torch.zeros(bins, dtype=torch.int32, device=seg.device)
    assert seg.is_contiguous() and seg.dtype == torch.float32
    L.pp_label_hist(seg.data_ptr(), seg.numel(), hist.data_ptr(), 1 if fix_below else 0, _stream())
    h = hist.cpu().numpy()
    if h[bins - 1]:
        raise ValueError("the segmentation holds %d values that are no whole-number labels in [-256, 255]" % int(h[bins - 1]))
    return np.nonzero(h[:bins - 1])[0] - 256


def get_case_identifier(case):
    """Reference :51-53"""
    return case[0].split("/")[-1].split(".nii.gz")[0][:-5]


def load_case_from_list_of_files(data_files, seg_file=None):
    """Reference :61-81, the SimpleITK loader: ``(data [C, X, Y, Z] fp32, seg [1, X, Y, Z] fp32 or None, properties)``"""
    import SimpleITK as sitk
    assert isinstance(data_files, (list, tuple)), "case must be either a list or a tuple"
    properties = OrderedDict()
    data_itk = [sitk.ReadImage(f) for f in data_files]
    properties["original_size_of_raw_data"] = np.array(data_itk[0].GetSize())[[2, 1, 0]]
    properties["original_spacing"] = np.array(data_itk[0].GetSpacing())[[2, 1, 0]]
    properties["list_of_data_files"] = data_files
    properties["seg_file"] = seg_file
    properties["itk_origin"] = data_itk[0].GetOrigin()
    properties["itk_spacing"] = data_itk[0].GetSpacing()
    properties["itk_direction"] = data_itk[0].GetDirection()
    data_npy = np.vstack([sitk.GetArrayFromImage(d)[None] for d in data_itk]).astype(np.float32)
    seg_npy = sitk.GetArrayFromImage(sitk.ReadImage(seg_file))[None].astype(np.float32) if seg_file is not None else None
    return data_npy, seg_npy, properties


def default_reader():
    """``reader(list_of_files) -> (data, properties)`` on the reference's SimpleITK loader, or None when SimpleITK is not importable"""
    try:
        import SimpleITK  # noqa: F401
    except ImportError:
        return None

    def read(list_of_files):
        data, _, properties = load_case_from_list_of_files(list_of_files)
        return data, properties
    return read


def require_reader(reader, what):
    """``reader``, or the default one; without either, the refusal every entry point that is handed file paths gives"""
    reader = default_reader() if reader is None else reader
    if reader is None:
        raise NotImplementedError(
            "%s was given file paths, but no reader: the preprocessing itself (crop, resample, normalise) runs on the device, reading "
            "an image file does not.  Pass reader=callable(list_of_files) -> (data [C, X, Y, Z], properties with 'original_spacing'), "
            "or install SimpleITK for the reference's loader, or hand over the case in memory as (data, properties)" % (what,))
    return reader


def load_case(data_files, seg_file, reader, what):
    """``(data, seg or None, properties)`` of a list of files through ``reader`` (a seg file needs the SimpleITK loader)"""
    if seg_file is not None:
        require_reader(default_reader(), what + " with a seg file")
        return load_case_from_list_of_files(data_files, seg_file)
    data, properties = require_reader(reader, what)(data_files)
    return data, None, properties


def _as_float32(a):
    """what a reader returned as fp32: a device tensor stays where it is (``ImageCropper.crop`` and ``to_device`` take one), anything
    else becomes a numpy array"""
    if hasattr(a, "is_cuda"):
        return a.float()
    return np.asarray(a, dtype=np.float32)


def load_seg_with_reader(seg_file, reader):
    """``seg [1, X, Y, Z]`` fp32 of a segmentation file: ``reader`` is handed the one-file list and the first channel is kept"""
    seg, _ = reader([seg_file])
    return _as_float32(seg[0:1])


def load_case_with_reader(data_files, seg_file, reader, what):
    """``(data, seg or None, properties)`` like load_case_from_list_of_files (reference :61-81), every file read through ``reader``
    (default: the SimpleITK loader; without either, the refusal of require_reader)"""
    assert isinstance(data_files, (list, tuple)), "case must be either a list or a tuple"
    reader = require_reader(reader, what)
    data, properties = reader(list(data_files))
    data = _as_float32(data)
    properties.setdefault("original_size_of_raw_data", np.array([int(v) for v in data.shape[1:]]))
    properties.setdefault("list_of_data_files", data_files)
    properties["seg_file"] = seg_file
    seg = load_seg_with_reader(seg_file, reader) if seg_file is not None else None
    return data, seg, properties


def get_patient_identifiers_from_cropped_files(folder):
    """Reference :119-120: the sorted case names of the ``.npz`` files of a cropped folder"""
    return sorted(f[:-4] for f in os.listdir(folder) if f.endswith(".npz") and os.path.isfile(os.path.join(folder, f)))


class ImageCropper(object):
    """Reference :123-217.  The device crops one case after the other; ``num_threads`` (at most 16) host threads compress and write
    the finished ones meanwhile."""

    def __init__(self, num_threads=None, output_folder=None):
        self.num_threads, self.output_folder = num_threads, output_folder
        if self.output_folder is not None:
            os.makedirs(self.output_folder, exist_ok=True)

    @staticmethod
    def crop(data, properties, seg=None):
        """Reference :139-150: crop to the non-zero region and record ``crop_bbox``, ``classes`` (``np.unique`` of the cropped seg,
        from a device histogram) and ``size_after_cropping``; ``seg[seg < -1] = 0``."""
        import torch
        shape_before = tuple(data.shape)
        was_numpy = not isinstance(data, torch.Tensor)
        dev, _ = to_device(data)
        sdev = to_device(seg)[0] if seg is not None else None
        out, out_seg, bbox = crop_to_nonzero(dev, sdev, nonzero_label=-1)
        print("before crop:", shape_before, "after crop:", tuple(out.shape), "spacing:", np.array(properties["original_spacing"]), "\n")
        properties["crop_bbox"] = bbox
        classes = label_values(out_seg, fix_below=True)
        properties['classes'] = classes.astype(np.float32) if seg is not None else classes.astype(int)
        properties["size_after_cropping"] = tuple(int(v) for v in out.shape[1:])
        if was_numpy:
            s = out_seg.cpu().numpy()
            return out.cpu().numpy(), (s.astype(seg.dtype) if seg is not None else s.astype(int)), properties
        return out, out_seg, properties

    @staticmethod
    def crop_from_list_of_files(data_files, seg_file=None, reader=None):
        """Reference :152-155 through the ``reader`` callback (a seg file needs the SimpleITK loader)"""
        data, seg, properties = load_case(data_files, seg_file, reader, "ImageCropper.crop_from_list_of_files")
        return ImageCropper.crop(data, properties, seg)

    def _is_done(self, case_identifier):
        return all(os.path.isfile(os.path.join(self.output_folder, case_identifier + e)) for e in (".npz", ".pkl"))

    def _crop_case(self, case, reader, device_deflate=False):
        """the device half of load_crop_save: ``(vstack((data, seg)) as fp32 numpy, properties)``; with ``device_deflate`` the
        stacked array stays on the device and comes back deflated there, as a ``DeflatedCase``"""
        import torch
        from .. import deflate
        from .preprocessing import DeflatedCase
        codes = deflate.codes_of(device_deflate)
        data, seg, properties = load_case_with_reader(case[:-1], case[-1], reader, "ImageCropper.load_crop_save")
        data, seg, properties = self.crop(to_device(data)[0], properties, to_device(seg)[0] if seg is not None else None)
        all_data = torch.cat((data, seg))
        return DeflatedCase(all_data, codes) if codes is not None else all_data.cpu().numpy(), properties

    def _write_case(self, all_data, properties, case_identifier):
        """the host half: ``<case>.npz`` (key ``data``) with a fixed time stamp, ``<case>.pkl``.  Touches no device: a
        ``DeflatedCase`` brings the bytes of its ``.npz``."""
        from .preprocessing import DeflatedCase, save_npz
        if isinstance(all_data, DeflatedCase):
            all_data.write(os.path.join(self.output_folder, "%s.npz" % case_identifier))
        else:
            save_npz(os.path.join(self.output_folder, "%s.npz" % case_identifier), all_data)
        self.save_properties(case_identifier, properties)

    def load_crop_save(self, case, case_identifier, overwrite_existing=False, reader=None, device_deflate=False):
        """Reference :157-174.  ``case``: the modality files and, last, the segmentation file (or None)"""
        try:
            print(case_identifier)
            if overwrite_existing or not self._is_done(case_identifier):
                self._write_case(*self._crop_case(case, reader, device_deflate), case_identifier)
        except Exception as e:
            print("Exception in", case_identifier, ":")
            print(e)
            raise e

    def get_list_of_cropped_files(self):
        """Reference :176-177"""
        return [os.path.join(self.output_folder, c + ".npz") for c in get_patient_identifiers_from_cropped_files(self.output_folder)]

    def get_patient_identifiers_from_cropped_files(self):
        """Reference :179-180"""
        return [i.split("/")[-1][:-4] for i in self.get_list_of_cropped_files()]

    def run_cropping(self, list_of_files, overwrite_existing=False, output_folder=None, reader=None, device_deflate=False):
        """Reference :182-208: copies the ground-truth files into ``gt_segmentations`` and crops every case of ``list_of_files``
        (``[[modality files ..., seg file], ...]``) into ``<case>.npz`` (key ``data``: modalities and seg stacked, fp32) and
        ``<case>.pkl``.  ``overwrite_existing=False`` skips a case whose two files exist.  This process owns the GPU and walks the
        cases; the writer threads compress and write finished ones.  The files do not depend on their number.  ``device_deflate``
        (True: fixed codes, ``"dynamic"``: a Huffman code per chunk): the stacked array is deflated on the device by this thread and
        the writer threads only write; ``np.load`` gives the same ``data``, the ``.pkl`` is the same."""
        from concurrent.futures import ThreadPoolExecutor
        from .. import deflate
        deflate.codes_of(device_deflate)
        if output_folder is not None:
            self.output_folder = output_folder
        output_folder_gt = os.path.join(self.output_folder, "gt_segmentations")
        os.makedirs(output_folder_gt, exist_ok=True)
        for case in list_of_files:
            if case[-1] is not None:
                shutil.copy(case[-1], output_folder_gt)
        reader = require_reader(reader, "ImageCropper.run_cropping")
        workers = max(1, min(int(self.num_threads if self.num_threads is not None else 1), MAX_WRITER_THREADS))
        with ThreadPoolExecutor(max_workers=workers) as pool:
            pending = deque()
            for case in list_of_files:
                case_identifier = get_case_identifier(case)
                print(case_identifier)
                if not overwrite_existing and self._is_done(case_identifier):
                    continue
                done = self._crop_case(case, reader, device_deflate)
                while len(pending) >= workers:               # bounds the finished cases held in host memory
                    pending.popleft().result()
                pending.append(pool.submit(self._write_case, *done, case_identifier))
            while pending:
                pending.popleft().result()

    def load_properties(self, case_identifier):
        """Reference :210-213"""
        with open(os.path.join(self.output_folder, "%s.pkl" % case_identifier), 'rb') as f:
            properties = pickle.load(f)
        return properties

    def save_properties(self, case_identifier, properties):
        """Reference :215-217"""
        with open(os.path.join(self.output_folder, "%s.pkl" % case_identifier), 'wb') as f:
            pickle.dump(properties, f)
