"""The reference's e2enet/preprocessing/preprocessing.py (GenericPreprocessor) on the device (csrc/preprocess.hip, class_select.hip):
a case in memory, or a cropped training folder into the stage folders the trainer reads.

  get_do_separate_z, get_lowres_axis, resample_patient, resample_data_or_seg   :28-202, same names, arguments and return values
  GenericPreprocessor (load_cropped, resample_and_normalize, preprocess_test_case, _run_internal, run)   :205-407
  GenericPreprocessor_linearResampling                                         :410-415
  class_locations                                                              :343-361, the sampling inside _run_internal
  run_preprocessing                     experiment_planning/experiment_planner_baseline_3DUNet.py:425-445, from a plans dict or file

The data is resized like ``skimage.transform.resize(order=3, mode='edge', anti_aliasing=False, clip=True)`` (scikit-image >= 0.19:
``scipy.ndimage.zoom(order=3, mode='nearest', grid_mode=True)`` clipped to the input's range), the segmentation like
batchgenerators' ``resize_segmentation(order=1)``; with a separate low-resolution axis every slice across it is resized in 2-D and the
axis itself with order 0.  These are the reference's defaults; its other orders raise NotImplementedError, except ``order_data=1``
(GenericPreprocessor_linearResampling), which is ``e2e_resample_linear``.  The 2-D preprocessor and the custom preprocessors are not
part of this package."""
import os
import pickle
import shutil
import zipfile
from collections import deque

import numpy as np

from .class_sampling import MIN_PERCENT_COVERAGE, NUM_SAMPLES, SEED, draw_ranks, sort_ranks
from .cropping import MAX_WRITER_THREADS, ImageCropper, _stream, label_values, load_case, to_device

RESAMPLING_SEPARATE_Z_ANISO_THRESHOLD = 3        # reference e2enet/configuration.py
SPLINE_PAD = 12                                  # scipy's pre-padding for mode 'nearest' in front of the spline prefilter
SCHEMES = {"CT": 1, "CT2": 2, "noNorm": 3}       # every other name is the default scheme (0)
DEFAULT_NUM_THREADS = 8                          # reference e2enet/configuration.py
BUILT_PREPROCESSORS = ("GenericPreprocessor", "GenericPreprocessor_linearResampling")


def get_do_separate_z(spacing, anisotropy_threshold=RESAMPLING_SEPARATE_Z_ANISO_THRESHOLD):
    """Reference :28-30"""
    return (np.max(spacing) / np.min(spacing)) > anisotropy_threshold


def get_lowres_axis(new_spacing):
    """Reference :33-35"""
    return np.where(max(new_spacing) / np.array(new_spacing) == 1)[0]


def separate_z_plan(original_spacing, target_spacing, force_separate_z=None,
                    separate_z_anisotropy_threshold=RESAMPLING_SEPARATE_Z_ANISO_THRESHOLD):
    """``(do_separate_z, axis)`` as resample_patient decides them (:70-96); ``axis`` is the reference's array or None"""
    if force_separate_z is not None:
        do_separate_z = force_separate_z
        axis = get_lowres_axis(original_spacing) if force_separate_z else None
    elif get_do_separate_z(original_spacing, separate_z_anisotropy_threshold):
        do_separate_z, axis = True, get_lowres_axis(original_spacing)
    elif get_do_separate_z(target_spacing, separate_z_anisotropy_threshold):
        do_separate_z, axis = True, get_lowres_axis(target_spacing)
    else:
        do_separate_z, axis = False, None
    if axis is not None and len(axis) != 1:
        do_separate_z = False          # spacings like (0.24, 1.25, 1.25), or all equal: no separate out-of-plane axis
    return do_separate_z, axis


def resampled_shape(shape, original_spacing, target_spacing):
    """Reference :68"""
    return np.round(((np.array(original_spacing) / np.array(target_spacing)).astype(float) * np.array(shape))).astype(int)


def resample_patient(data, seg, original_spacing, target_spacing, order_data=3, order_seg=0, force_separate_z=False,
                     order_z_data=0, order_z_seg=0, separate_z_anisotropy_threshold=RESAMPLING_SEPARATE_Z_ANISO_THRESHOLD):
    """Reference :38-107"""
    assert not ((data is None) and (seg is None))
    if data is not None:
        assert len(data.shape) == 4, "data must be c x y z"
    if seg is not None:
        assert len(seg.shape) == 4, "seg must be c x y z"
    shape = np.array(data[0].shape if data is not None else seg[0].shape)
    new_shape = resampled_shape(shape, original_spacing, target_spacing)
    do_separate_z, axis = separate_z_plan(original_spacing, target_spacing, force_separate_z, separate_z_anisotropy_threshold)
    data_reshaped = seg_reshaped = None
    if data is not None:
        data_reshaped = resample_data_or_seg(data, new_shape, False, axis, order_data, do_separate_z, order_z=order_z_data)
    if seg is not None:
        seg_reshaped = resample_data_or_seg(seg, new_shape, True, axis, order_seg, do_separate_z, order_z=order_z_seg)
    return data_reshaped, seg_reshaped


def _grid(x):
    """(K, channel stride, shape, strides) of a device tensor [K, A, B, C] that may be a transposed view"""
    return int(x.shape[0]), int(x.stride(0)), [int(v) for v in x.shape[1:]], [int(x.stride(1 + a)) for a in range(3)]


def _is_dense(x):
    """the elements of the view fill ``numel`` consecutive words from ``data_ptr`` (a permutation of a contiguous tensor)"""
    expect = 1
    for size, stride in sorted(((int(n), int(s)) for n, s in zip(x.shape, x.stride()) if n > 1), key=lambda t: t[1]):
        if stride != expect:
            return False
        expect *= size
    return True


def _resize_cubic(x, new_shape, lowres):
    import torch
    from .._lib import lib
    L = lib()
    K, ks, n, st = _grid(x)
    st_ = _stream()
    groups = K * (1 if lowres < 0 else n[lowres])
    ws = torch.empty(L.pp_minmax_ws_bytes(K, n[0], n[1], n[2], lowres), dtype=torch.uint8, device=x.device)
    minmax = torch.empty(groups * 2, dtype=torch.float64, device=x.device)
    L.pp_minmax(x.data_ptr(), minmax.data_ptr(), ws.data_ptr(), K, ks, n[0], n[1], n[2], st[0], st[1], st[2], lowres, st_)
    pads = [0 if a == lowres else SPLINE_PAD for a in range(3)]
    P = [n[a] + 2 * pads[a] for a in range(3)]
    coef = torch.empty([K] + P, dtype=torch.float32, device=x.device)
    L.pp_pad_edge(x.data_ptr(), coef.data_ptr(), K, ks, n[0], n[1], n[2], st[0], st[1], st[2], pads[0], pads[1], pads[2], st_)
    for a in range(3):
        if a != lowres:
            L.aug_bspline_prefilter_axis(coef.data_ptr(), coef.data_ptr(), K, P[0], P[1], P[2], a, st_)
    out = torch.empty([K] + list(new_shape), dtype=torch.float32, device=x.device)
    L.pp_resize_cubic(coef.data_ptr(), out.data_ptr(), minmax.data_ptr(), K, n[0], n[1], n[2], new_shape[0], new_shape[1], new_shape[2],
                      SPLINE_PAD, lowres, st_)
    return out


def resample_data_or_seg(data, new_shape, is_seg, axis=None, order=3, do_separate_z=False, order_z=0):
    """Reference :113-202.  ``data`` [C, X, Y, Z]: a numpy array (returned as a numpy array of its dtype) or an fp32 device tensor,
    possibly a transposed view (returned as a contiguous fp32 device tensor).  Served: ``order`` 3 or 1 for data, 1 for a seg, and
    ``order_z`` 0.  A resampled seg comes back with its labels < -1 written as 0, which the reference does right afterwards, in
    resample_and_normalize."""
    import torch
    from .._lib import lib
    assert len(data.shape) == 4, "data must be (c, x, y, z)"
    assert len(new_shape) == len(data.shape) - 1
    new_shape = [int(v) for v in new_shape]
    if all(int(a) == b for a, b in zip(data.shape[1:], new_shape)):
        print("no resampling necessary")
        return data
    if order_z != 0 or order not in ((1,) if is_seg else (3, 1)):
        raise NotImplementedError("device resampling implements the reference's defaults: order 3 (or 1) for the data, order 1 for "
                                  "the segmentation, order 0 along a separate low-resolution axis (got order=%r, order_z=%r, "
                                  "is_seg=%r)" % (order, order_z, is_seg))
    lowres = -1
    if do_separate_z:
        assert len(axis) == 1, "only one anisotropic axis supported"
        lowres = int(axis[0])
        print("separate z, order in z is", order_z, "order inplane is", order)
    else:
        print("no separate z, order", order)
    was_numpy = not isinstance(data, torch.Tensor)
    x = torch.from_numpy(np.ascontiguousarray(data, dtype=np.float32)).cuda() if was_numpy else data
    assert x.is_cuda and x.dtype == torch.float32, "a tensor input must be an fp32 device tensor"
    K, ks, n, st = _grid(x)
    if is_seg or order == 1:
        out = torch.empty([K] + new_shape, dtype=torch.float32, device=x.device)
        fn = lib().pp_resize_seg if is_seg else lib().resample_linear
        fn(x.data_ptr(), out.data_ptr(), K, ks, n[0], n[1], n[2], st[0], st[1], st[2], new_shape[0], new_shape[1], new_shape[2],
           lowres, _stream())
    else:
        out = _resize_cubic(x, new_shape, lowres)
    return out.cpu().numpy().astype(data.dtype) if was_numpy else out


def class_locations(seg, all_classes, num_samples=NUM_SAMPLES, min_percent_coverage=MIN_PERCENT_COVERAGE, seed=SEED):
    """Reference :343-361: ``{c: np.argwhere(seg == c)[RandomState(seed).choice(n, t, replace=False)]}`` over ``all_classes`` in
    order (int64 ``[t, 3]``; ``[]`` for a class without a voxel, which draws nothing), one RandomState for all of them.  ``seg``: a
    label volume [X, Y, Z], a device tensor (it stays there) or a numpy array (uploaded once).  The device counts the classes
    (e2e_pp_select_count), the host draws the ranks with the reference's numpy calls (class_sampling.draw_ranks), the device turns
    them into coordinates (e2e_pp_select_coords): ``argwhere`` is never materialised."""
    import torch
    from .._lib import lib, E2EError
    L = lib()
    assert len(seg.shape) == 3, "seg must be (x, y, z)"
    s, _ = to_device(seg)
    all_classes = list(all_classes)
    shape = [int(v) for v in s.shape]
    n = int(s.numel())
    if n == 0 or not all_classes:
        return {c: [] for c in all_classes}
    kmax = L.pp_select_max_classes()
    groups = [all_classes[g:g + kmax] for g in range(0, len(all_classes), kmax)]
    st = _stream()
    counted = []
    for grp in groups:                               # one read of the volume per kmax classes
        cls = np.ascontiguousarray(grp, dtype=np.float32)
        nbytes = L.pp_select_ws_bytes(n, len(grp))
        if nbytes <= 0:
            raise E2EError("pp_select_ws_bytes: a volume of %d voxels is not supported" % n)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=s.device)
        counts = torch.empty(len(grp), dtype=torch.int64, device=s.device)
        L.pp_select_count(s.data_ptr(), n, cls.ctypes.data, len(grp), counts.data_ptr(), ws.data_ptr(), st)
        counted.append((cls, ws, counts))
    totals = torch.cat([c[2] for c in counted]).cpu().numpy()
    drawn = draw_ranks(totals, num_samples, min_percent_coverage, seed)
    locs, pos = {}, 0
    for grp, (cls, ws, _) in zip(groups, counted):
        pairs = [sort_ranks(r) for r in drawn[pos:pos + len(grp)]]
        pos += len(grp)
        class_offsets = np.zeros(len(grp) + 1, dtype=np.int64)
        class_offsets[1:] = np.cumsum([len(p[0]) for p in pairs])
        rows = None
        if class_offsets[-1]:
            ranks = torch.from_numpy(np.concatenate([p[0] for p in pairs])).to(s.device)
            slots = torch.from_numpy(np.concatenate([p[1] for p in pairs])).to(s.device)
            out = torch.empty((int(class_offsets[-1]), 3), dtype=torch.int64, device=s.device)
            L.pp_select_coords(s.data_ptr(), shape[0], shape[1], shape[2], cls.ctypes.data, len(grp), ranks.data_ptr(), slots.data_ptr(),
                               class_offsets.ctypes.data, out.data_ptr(), ws.data_ptr(), st)
            rows = out.cpu().numpy()
        for i, c in enumerate(grp):
            a, b = int(class_offsets[i]), int(class_offsets[i + 1])
            locs[c] = rows[a:b].copy() if b > a else []
    return locs


def save_npz(path, data):
    """``np.savez_compressed(path, data=data)`` with a fixed time stamp on the archive member: the file's bytes depend on the array
    alone, not on when or by which thread it was written"""
    info = zipfile.ZipInfo("data.npy", date_time=(1980, 1, 1, 0, 0, 0))
    info.compress_type = zipfile.ZIP_DEFLATED
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, allowZip64=True) as z:
        with z.open(info, "w", force_zip64=True) as f:
            np.lib.format.write_array(f, np.asanyarray(data), allow_pickle=False)


class DeflatedCase(object):
    """A finished case whose ``<case>.npz`` the device has already compressed (``device_deflate``): the byte strings of the file
    (``deflate.npz_parts(data=...)``), and the array itself only where ``--unpack`` needs it for the ``.npy``"""

    def __init__(self, all_data, codes, unpack_npy=False):
        from .. import deflate
        self.parts = deflate.npz_parts(codes=codes, data=all_data)
        self.array = all_data.cpu().numpy() if unpack_npy else None

    def write(self, npz_path):
        from .. import deflate
        deflate.write_parts(npz_path, self.parts)


def preprocessor_class(preprocessor_name, three_d=True):
    """The class the plans' ``preprocessor_name`` names (None: GenericPreprocessor); NotImplementedError for anything but the two
    built classes, or for 2-D plans"""
    if preprocessor_name is None:
        preprocessor_name = "GenericPreprocessor"
    if not three_d or preprocessor_name not in BUILT_PREPROCESSORS:
        raise NotImplementedError("preprocessor %r: the device preprocessing implements GenericPreprocessor and "
                                  "GenericPreprocessor_linearResampling on 3-D plans" % (preprocessor_name,))
    return globals()[preprocessor_name]


class GenericPreprocessor(object):
    """Reference :205-407"""

    def __init__(self, normalization_scheme_per_modality, use_nonzero_mask, transpose_forward, intensityproperties=None):
        self.transpose_forward = transpose_forward
        self.intensityproperties = intensityproperties
        self.normalization_scheme_per_modality = normalization_scheme_per_modality
        self.use_nonzero_mask = use_nonzero_mask
        self.resample_separate_z_anisotropy_threshold = RESAMPLING_SEPARATE_Z_ANISO_THRESHOLD
        self.resample_order_data = 3
        self.resample_order_seg = 1

    def _norm_params(self, num_modalities, have_seg):
        prm = np.zeros((num_modalities, 8), dtype=np.float64)
        for c in range(num_modalities):
            scheme = self.normalization_scheme_per_modality[c]
            prm[c, 0] = SCHEMES.get(scheme, 0)
            if scheme in ("CT", "CT2"):
                assert self.intensityproperties is not None, "ERROR: if there is a CT then we need intensity properties"
                ip = self.intensityproperties[c]
                prm[c, 1], prm[c, 2] = ip['percentile_00_5'], ip['percentile_99_5']
                if scheme == "CT":
                    prm[c, 3], prm[c, 4] = ip['mean'], ip['sd']
            if scheme == 'noNorm':
                print('no intensity normalization')
            elif self.use_nonzero_mask[c]:
                if not have_seg:
                    raise ValueError("use_nonzero_mask[%d] is set but there is no seg to take the mask from" % c)
                prm[c, 5] = 1.0
        return prm

    @staticmethod
    def load_cropped(cropped_output_dir, case_identifier):
        """Reference :223-229"""
        all_data = np.load(os.path.join(cropped_output_dir, "%s.npz" % case_identifier))['data']
        data = all_data[:-1].astype(np.float32)
        seg = all_data[-1:]
        with open(os.path.join(cropped_output_dir, "%s.pkl" % case_identifier), 'rb') as f:
            properties = pickle.load(f)
        return data, seg, properties

    def resample_and_normalize(self, data, target_spacing, properties, seg=None, force_separate_z=None):
        """Reference :231-319.  ``data`` [C, X, Y, Z] and ``seg`` [S, X, Y, Z] are already transposed by ``transpose_forward``,
        ``properties`` are not.  numpy in, numpy out; device tensors in (fp32, views allowed), contiguous device tensors out."""
        import torch
        from .._lib import lib
        L = lib()
        was_numpy = not isinstance(data, torch.Tensor)
        seg_dtype = seg.dtype if seg is not None and was_numpy else None
        x = torch.from_numpy(np.ascontiguousarray(data, dtype=np.float32)).cuda() if was_numpy else data
        s = None
        if seg is not None:
            s = torch.from_numpy(np.ascontiguousarray(seg, dtype=np.float32)).cuda() if not isinstance(seg, torch.Tensor) else seg
        original_spacing_transposed = np.array(properties["original_spacing"])[self.transpose_forward]
        before = {'spacing': properties["original_spacing"], 'spacing_transposed': original_spacing_transposed,
                  'data.shape (data is transposed)': tuple(x.shape)}
        # remove nans, in place like the reference (a transposed view of a dense tensor covers its storage: no copy)
        if not _is_dense(x):
            x = x.contiguous()
        L.pp_nan_to_zero(x.data_ptr(), x.numel(), _stream())
        x, s = resample_patient(x, s, np.array(original_spacing_transposed), target_spacing, self.resample_order_data,
                                self.resample_order_seg, force_separate_z=force_separate_z, order_z_data=0, order_z_seg=0,
                                separate_z_anisotropy_threshold=self.resample_separate_z_anisotropy_threshold)
        after = {'spacing': target_spacing, 'data.shape (data is resampled)': tuple(x.shape)}
        print("before:", before, "\nafter: ", after, "\n")
        x = x.contiguous()                                     # (a copy only when a transposed view was not resampled)
        if s is not None:
            s = s.contiguous()
            label_values(s, fix_below=True)                    # seg[seg < -1] = 0 (pp_resize_seg has done it when it ran)
        properties["size_after_resampling"] = tuple(int(v) for v in x.shape[1:])
        properties["spacing_after_resampling"] = target_spacing
        C = int(x.shape[0])
        assert len(self.normalization_scheme_per_modality) == C, "self.normalization_scheme_per_modality must have as many entries " \
                                                                 "as data has modalities"
        assert len(self.use_nonzero_mask) == C, "self.use_nonzero_mask must have as many entries as data has modalities"
        prm = torch.from_numpy(self._norm_params(C, s is not None)).to(x.device)
        stats = torch.zeros((C, 4), dtype=torch.float64, device=x.device)
        ws = torch.empty(L.pp_norm_ws_bytes(C), dtype=torch.uint8, device=x.device)
        vol = x.numel() // C
        mask_seg = s[-1].data_ptr() if s is not None else None
        L.pp_norm_stats(x.data_ptr(), mask_seg, prm.data_ptr(), stats.data_ptr(), ws.data_ptr(), C, vol, _stream())
        L.pp_normalize(x.data_ptr(), mask_seg, prm.data_ptr(), stats.data_ptr(), C, vol, _stream())
        if was_numpy:
            return x.cpu().numpy(), (s.cpu().numpy().astype(seg_dtype) if s is not None else None), properties
        return x, s, properties

    def preprocess_test_case(self, data_files, target_spacing, seg_file=None, force_separate_z=None, reader=None):
        """Reference :321-329.  ``data_files``: a list of file paths (read through ``reader``, default the SimpleITK loader) or an
        in-memory case ``(data [C, X, Y, Z], properties)`` whose properties hold at least ``original_spacing``.  Returns
        ``(data fp32, seg, properties)`` as numpy arrays."""
        import torch
        if isinstance(data_files, tuple) and len(data_files) == 2 and isinstance(data_files[1], dict):
            data, properties = data_files
            assert seg_file is None, "an in-memory case takes no seg file"
            properties.setdefault("original_size_of_raw_data", np.array([int(v) for v in data.shape[1:]]))
            data, seg, properties = ImageCropper.crop(to_device(data)[0], properties, None)
        else:
            data, seg, properties = load_case(data_files, seg_file, reader, "preprocess_test_case")
            data, seg, properties = ImageCropper.crop(to_device(data)[0], properties, to_device(seg)[0] if seg is not None else None)
        made_up_seg = seg_file is None
        perm = (0, *[i + 1 for i in self.transpose_forward])
        data, seg, properties = self.resample_and_normalize(data.permute(perm), target_spacing, properties, seg.permute(perm),
                                                            force_separate_z=force_separate_z)
        seg = seg.cpu().numpy()
        return data.cpu().numpy().astype(np.float32), (seg.astype(int) if made_up_seg else seg), properties


    def _preprocess_cropped(self, target_spacing, case_identifier, cropped_output_dir, force_separate_z, all_classes,
                            keep_on_device=False):
        """the device half of _run_internal (:333-361): ``(vstack((data, seg)) as fp32 numpy, properties with class_locations)``;
        ``keep_on_device``: the stacked array stays the device tensor it is"""
        import torch
        data, seg, properties = self.load_cropped(cropped_output_dir, case_identifier)
        perm = (0, *[i + 1 for i in self.transpose_forward])
        data, seg = to_device(data)[0].permute(perm), to_device(seg)[0].permute(perm)
        data, seg, properties = self.resample_and_normalize(data, target_spacing, properties, seg, force_separate_z)
        properties['class_locations'] = class_locations(seg[-1], all_classes)
        for c, locs in properties['class_locations'].items():
            if len(locs):
                print(c, len(locs))
        all_data = torch.cat((data, seg))
        return all_data if keep_on_device else all_data.cpu().numpy(), properties

    @staticmethod
    def _write_case(all_data, properties, output_folder_stage, case_identifier, unpack_npy=False):
        """the host half of _run_internal (:363-367): ``<case>.npz`` (key ``data``), ``<case>.pkl``; ``unpack_npy`` also writes the
        ``<case>.npy`` that DataLoader3D memory-maps (the reference's unpack_dataset).  Touches no device: a ``DeflatedCase`` brings
        the bytes of its ``.npz``."""
        print("saving: ", os.path.join(output_folder_stage, "%s.npz" % case_identifier))
        if isinstance(all_data, DeflatedCase):
            all_data.write(os.path.join(output_folder_stage, "%s.npz" % case_identifier))
            all_data = all_data.array
        else:
            save_npz(os.path.join(output_folder_stage, "%s.npz" % case_identifier), all_data)
        if unpack_npy:
            np.save(os.path.join(output_folder_stage, "%s.npy" % case_identifier), all_data)
        with open(os.path.join(output_folder_stage, "%s.pkl" % case_identifier), 'wb') as f:
            pickle.dump(properties, f)

    def _run_internal(self, target_spacing, case_identifier, output_folder_stage, cropped_output_dir, force_separate_z, all_classes,
                      unpack_npy=False, device_deflate=False):
        """Reference :331-367"""
        from .. import deflate
        codes = deflate.codes_of(device_deflate)
        all_data, properties = self._preprocess_cropped(target_spacing, case_identifier, cropped_output_dir, force_separate_z,
                                                        all_classes, keep_on_device=codes is not None)
        if codes is not None:
            all_data = DeflatedCase(all_data, codes, unpack_npy)
        self._write_case(all_data, properties, output_folder_stage, case_identifier, unpack_npy)

    def run(self, target_spacings, input_folder_with_cropped_npz, output_folder, data_identifier, num_threads=DEFAULT_NUM_THREADS,
            force_separate_z=None, unpack_npy=False, device_deflate=False):
        """Reference :369-407: every ``<case>.npz`` + ``<case>.pkl`` of a cropped folder into ``<output_folder>/<data_identifier>_stage<i>``
        for each target spacing.  This process owns the GPU and walks the cases; ``num_threads`` (one number, or one per stage; at most
        16) host threads compress and write finished cases while the device works on the next ones.  The files do not depend on it.
        ``device_deflate`` (True: fixed codes, ``"dynamic"``: a Huffman code per chunk): the stacked array stays on the device, this
        thread deflates it there (``deflate.npz_parts``) and the writer threads only write; ``np.load`` gives the same ``data``, the
        ``.pkl`` is the same, only the bytes of the ``.npz`` differ from the host route's."""
        from concurrent.futures import ThreadPoolExecutor
        from .. import deflate
        codes = deflate.codes_of(device_deflate)
        print("Initializing to run preprocessing")
        print("npz folder:", input_folder_with_cropped_npz)
        print("output_folder:", output_folder)
        cases = sorted(f[:-4] for f in os.listdir(input_folder_with_cropped_npz) if f.endswith(".npz"))
        os.makedirs(output_folder, exist_ok=True)
        num_stages = len(target_spacings)
        if not isinstance(num_threads, (list, tuple, np.ndarray)):
            num_threads = [num_threads] * num_stages
        assert len(num_threads) == num_stages
        # the classes of the dataset, so that every case records where they are: the loader's foreground oversampling needs it
        with open(os.path.join(input_folder_with_cropped_npz, 'dataset_properties.pkl'), 'rb') as f:
            all_classes = pickle.load(f)['all_classes']
        for i in range(num_stages):
            output_folder_stage = os.path.join(output_folder, data_identifier + "_stage%d" % i)
            os.makedirs(output_folder_stage, exist_ok=True)
            workers = max(1, min(int(num_threads[i]), MAX_WRITER_THREADS))
            with ThreadPoolExecutor(max_workers=workers) as pool:
                pending = deque()
                for case_identifier in cases:
                    done = self._preprocess_cropped(target_spacings[i], case_identifier, input_folder_with_cropped_npz,
                                                    force_separate_z, all_classes, keep_on_device=codes is not None)
                    if codes is not None:
                        done = (DeflatedCase(done[0], codes, unpack_npy), done[1])
                    while len(pending) >= workers:           # bounds the finished cases held in host memory
                        pending.popleft().result()
                    pending.append(pool.submit(self._write_case, *done, output_folder_stage, case_identifier, unpack_npy))
                while pending:
                    pending.popleft().result()


def run_preprocessing(plans, folder_with_cropped_data, preprocessed_output_folder, num_threads=DEFAULT_NUM_THREADS, unpack_npy=False,
                      device_deflate=False):
    """ExperimentPlanner.run_preprocessing (experiment_planner_baseline_3DUNet.py:425-445) from a plans dict or plans file: copies
    ``gt_segmentations`` when the cropped folder has one, then runs the plans' preprocessor over every stage's ``current_spacing``
    into ``<preprocessed_output_folder>/<data_identifier>_stage<i>``.  Plans that name another preprocessor than the two built
    classes, or 2-D plans, raise NotImplementedError before any file is touched.  ``device_deflate``: see ``GenericPreprocessor.run``."""
    if not isinstance(plans, dict):
        with open(plans, 'rb') as f:
            plans = pickle.load(f)
    stages = plans['plans_per_stage']
    three_d = all(len(stage['patch_size']) == 3 for stage in stages.values())
    cls = preprocessor_class(plans.get('preprocessor_name'), three_d)
    gt = os.path.join(folder_with_cropped_data, "gt_segmentations")
    if os.path.isdir(gt):
        gt_out = os.path.join(preprocessed_output_folder, "gt_segmentations")
        if os.path.isdir(gt_out):
            shutil.rmtree(gt_out)
        shutil.copytree(gt, gt_out)
    dataset_properties = plans.get('dataset_properties')
    intensityproperties = dataset_properties.get('intensityproperties') if isinstance(dataset_properties, dict) else None
    preprocessor = cls(plans['normalization_schemes'], plans['use_mask_for_norm'], plans.get('transpose_forward', [0, 1, 2]),
                       intensityproperties)
    target_spacings = [stage["current_spacing"] for stage in stages.values()]
    if len(stages) > 1 and not isinstance(num_threads, (list, tuple)):
        num_threads = (DEFAULT_NUM_THREADS, num_threads)
    elif len(stages) == 1 and isinstance(num_threads, (list, tuple)):
        num_threads = num_threads[-1]
    from ..paths import default_data_identifier
    preprocessor.run(target_spacings, folder_with_cropped_data, preprocessed_output_folder,
                     plans.get('data_identifier', default_data_identifier), num_threads, unpack_npy=unpack_npy,
                     device_deflate=device_deflate)


class GenericPreprocessor_linearResampling(GenericPreprocessor):
    """Reference :410-415"""

    def __init__(self, normalization_scheme_per_modality, use_nonzero_mask, transpose_forward, intensityproperties=None):
        super().__init__(normalization_scheme_per_modality, use_nonzero_mask, transpose_forward, intensityproperties)
        self.resample_order_data = 1
        self.resample_order_seg = 1
