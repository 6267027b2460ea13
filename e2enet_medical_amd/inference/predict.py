"""Fold ensembling and segmentation export with the softmax volume kept in HBM.

Reference: ``predict_cases`` (e2enet/inference/predict.py:194-359) runs, per case, one sliding-window prediction per
fold, sums the float32 softmax volumes on the HOST (:282-293), divides by the number of folds (:295-296), undoes the
plans' axis transposition (:298-301) and hands the multi-GB array to a worker process that takes the argmax (or the
region thresholds), places the result into the uncropped uint8 volume and writes NIfTI
(``save_segmentation_nifti_from_softmax``, e2enet/inference/segmentation_export.py:27-160).  Here the per-fold
probabilities never leave the device: accumulation, average, transposition, argmax / region thresholds and crop-box
placement are two HIP kernels (``e2e_ensemble_accumulate``, ``e2e_export_argmax_u8``); the host receives the final
uint8 label volume.  Arithmetic is bit-identical to the reference's numpy expressions (float32 adds in fold order,
float32 division by the fold count, first maximum).

Resampling to the grid the case had before preprocessing (segmentation_export.py:84-104: order 1, and order 0 along one
separate low-resolution axis when the spacing is anisotropic beyond ``RESAMPLING_SEPARATE_Z_ANISO_THRESHOLD``) is a third
kernel (``e2e_resample_linear``) with the arithmetic of ``scipy.ndimage.zoom(order=1, mode='nearest', grid_mode=True)`` --
what scikit-image 0.19.3's ``resize(order=1, mode='edge', anti_aliasing=False)`` evaluates.  Parity for that step is against
scipy (oracle/export.py; scikit-image is absent from the image: "parity unpinned").  The NIfTI writer (SimpleITK) is host
tooling; ``predict_cases`` therefore takes a ``writer`` callback.
"""
import os
import pickle
from typing import Callable, Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .._lib import lib
from ..preprocessing.preprocessing import RESAMPLING_SEPARATE_Z_ANISO_THRESHOLD, get_do_separate_z, get_lowres_axis  # noqa: F401


def _stream():
    return torch.cuda.current_stream().cuda_stream


def predict_case_ensemble(trainer, params: Sequence[dict], data: np.ndarray, do_tta: bool = True, step_size: float = 0.5,
                          all_in_gpu: bool = False, mixed_precision: bool = True) -> torch.Tensor:
    """Mean softmax of all folds for one preprocessed case, as a device tensor [K, X, Y, Z]
    (reference predict.py:282-296).  ``params``: the checkpoints of the folds (dicts as torch.load returns them)."""
    net = trainer.network
    keep = net.keep_on_device
    net.keep_on_device = True
    total = None
    try:
        for i, p in enumerate(params):
            trainer.load_checkpoint_ram(p, False)
            _, probs = trainer.predict_preprocessed_data_return_seg_and_softmax(
                data, do_mirroring=do_tta, mirror_axes=trainer.data_aug_params['mirror_axes'], use_sliding_window=True,
                step_size=step_size, use_gaussian=True, all_in_gpu=all_in_gpu, verbose=False, mixed_precision=mixed_precision)
            last = i + 1 == len(params)
            n_div = len(params) if (last and len(params) > 1) else 0
            if total is None:
                total = probs if len(params) == 1 else probs.clone()      # predict_3D reuses nothing, but later folds add in place
            else:
                lib().ensemble_accumulate(total.data_ptr(), probs.data_ptr(), total.numel(), 0, n_div, _stream())
    finally:
        net.keep_on_device = keep
    return total


def resample_plan(properties_dict: dict, force_separate_z: Optional[bool] = None):
    """(do_separate_z, lowres_axis or None): the decision of segmentation_export.py:85-106"""
    if force_separate_z is None:
        if get_do_separate_z(properties_dict.get('original_spacing')):
            do_separate_z, lowres_axis = True, get_lowres_axis(properties_dict.get('original_spacing'))
        elif get_do_separate_z(properties_dict.get('spacing_after_resampling')):
            do_separate_z, lowres_axis = True, get_lowres_axis(properties_dict.get('spacing_after_resampling'))
        else:
            do_separate_z, lowres_axis = False, None
    else:
        do_separate_z = force_separate_z
        lowres_axis = get_lowres_axis(properties_dict.get('original_spacing')) if do_separate_z else None
    if lowres_axis is not None and len(lowres_axis) != 1:
        do_separate_z = False          # spacings like (0.24, 1.25, 1.25): no separate out-of-plane axis (:102-105)
    return do_separate_z, (int(lowres_axis[0]) if do_separate_z else None)


def resample_softmax(softmax: torch.Tensor, new_shape: Sequence[int], transpose_backward: Optional[Sequence[int]] = None,
                     lowres_axis: Optional[int] = None) -> torch.Tensor:
    """Device softmax [K, X, Y, Z] -> contiguous [K] + new_shape in the transposed-backward frame, order 1 (order 0 along
    ``lowres_axis``): resample_data_or_seg(..., is_seg=False, order=1, order_z=0), preprocessing.py:113-202."""
    assert softmax.is_cuda and softmax.dtype == torch.float32 and softmax.dim() == 4
    tb = [0, 1, 2] if transpose_backward is None else [int(i) for i in transpose_backward]
    dims = [int(softmax.shape[1 + i]) for i in tb]
    strides = [int(softmax.stride(1 + i)) for i in tb]
    k = softmax.shape[0]
    new_shape = [int(v) for v in new_shape]
    out = torch.empty([k] + new_shape, dtype=torch.float32, device=softmax.device)
    lib().resample_linear(softmax.data_ptr(), out.data_ptr(), k, int(softmax.stride(0)), dims[0], dims[1], dims[2], strides[0],
                          strides[1], strides[2], new_shape[0], new_shape[1], new_shape[2],
                          -1 if lowres_axis is None else int(lowres_axis), _stream())
    return out


def softmax_to_f16(softmax: torch.Tensor, dims: Sequence[int], strides: Sequence[int]) -> torch.Tensor:
    """Contiguous device fp16 [K] + dims of a device fp32 softmax read through ``strides`` (those of ``softmax.transpose(...)``): the
    bits of ``softmax.transpose(...).astype(np.float16)`` (segmentation_export.py:118), rounded on the device."""
    assert softmax.is_cuda and softmax.dtype == torch.float32 and softmax.dim() == 4
    k = softmax.shape[0]
    out = torch.empty([k] + [int(v) for v in dims], dtype=torch.float16, device=softmax.device)
    lib().softmax_to_f16(softmax.data_ptr(), out.data_ptr(), k, int(softmax.stride(0)), int(dims[0]), int(dims[1]), int(dims[2]),
                         int(strides[0]), int(strides[1]), int(strides[2]), _stream())
    return out


def save_softmax_npz(softmax_f16: torch.Tensor, resampled_npz_fname: str, properties_dict: dict,
                     region_class_order: Optional[Sequence[int]] = None, device_deflate: Union[bool, str] = False):
    """``<case>.npz`` (key ``softmax``, fp16) and ``<case>.pkl`` as segmentation_export.py:117-122 leaves them for the ensembling
    step (inference/ensemble_predictions.py); the pickle names ``regions_class_order`` when there is one.  ``device_deflate``: the
    device tensor is deflated where it lies (``deflate.savez``) and only compressed bytes are downloaded; ``np.load`` reads the same
    array, the archive's bytes differ from the default route's.  A CPU or non-contiguous tensor is then a ValueError.  ``True``
    selects DEFLATE's fixed Huffman code, ``"dynamic"`` a code per chunk (``deflate.savez(codes=...)``)."""
    if device_deflate:
        from .. import deflate
        codes = deflate.codes_of(device_deflate, "save_softmax_npz: device_deflate")
        if not (softmax_f16.is_cuda and softmax_f16.is_contiguous()):
            raise ValueError("save_softmax_npz(device_deflate=True): the probabilities must be a contiguous device tensor (got %s)"
                             % ("a non-contiguous tensor" if softmax_f16.is_cuda else "a CPU tensor",))
        deflate.savez(resampled_npz_fname, codes=codes, softmax=softmax_f16)
    else:
        np.savez_compressed(resampled_npz_fname, softmax=softmax_f16.cpu().numpy())
    if region_class_order is not None:
        properties_dict = dict(properties_dict, regions_class_order=region_class_order)
    with open(resampled_npz_fname[:-4] + ".pkl", 'wb') as f:
        pickle.dump(properties_dict, f)


def export_segmentation(softmax: torch.Tensor, properties_dict: dict, transpose_backward: Optional[Sequence[int]] = None,
                        region_class_order: Optional[Sequence[int]] = None, force_separate_z: Optional[bool] = None,
                        order: int = 1, interpolation_order_z: int = 0, postprocessing=None,
                        resampled_npz_fname: Optional[str] = None, device_deflate: Union[bool, str] = False,
                        keep_on_device: bool = False) -> Union[np.ndarray, torch.Tensor]:
    """uint8 label volume in the ORIGINAL (uncropped) geometry from a device softmax [K, X, Y, Z]
    (reference predict.py:298-301 + segmentation_export.py:73-136).

    ``postprocessing``: ``(for_which_classes, min_valid_object_sizes or None)`` as ``load_postprocessing`` returns them; all but the
    largest connected component of those classes is then removed (reference predict.py:339-352, load_remove_save) on the device
    label volume, before its one download; ``volume_per_voxel`` is the product of ``properties_dict['itk_spacing']``.

    ``resampled_npz_fname`` (the reference's argument of that name): the probabilities the labels are taken from -- on the case's own
    grid, in its own axis order -- are also stored there as fp16, with the properties beside them (``save_softmax_npz``;
    ``device_deflate`` is handed on to it).  ``keep_on_device``: the label volume is returned as the device tensor it is, for a writer
    that compresses it there."""
    assert softmax.is_cuda and softmax.dtype == torch.float32 and softmax.dim() == 4 and softmax.is_contiguous()
    k = softmax.shape[0]
    tb = [0, 1, 2] if transpose_backward is None else [int(i) for i in transpose_backward]
    dims = [int(softmax.shape[1 + i]) for i in tb]                 # softmax.transpose([0] + [i + 1 for i in tb]).shape[1:]
    strides = [int(softmax.stride(1 + i)) for i in tb]
    after_crop = properties_dict.get('size_after_cropping')
    if after_crop is not None and any(int(a) != int(b) for a, b in zip(dims, after_crop)):
        # the network ran on a resampled grid: back to the case's own grid before the argmax (segmentation_export.py:84-104)
        if order != 1 or interpolation_order_z != 0:
            raise NotImplementedError("device resampling implements the reference's defaults: order 1 in the plane, order 0 "
                                      "along a separate low-resolution axis (predict.py:171-172)")
        _, lowres = resample_plan(properties_dict, force_separate_z)
        softmax = resample_softmax(softmax, after_crop, tb, lowres)
        dims = [int(v) for v in after_crop]
        strides = [int(softmax.stride(1 + i)) for i in range(3)]
    if resampled_npz_fname is not None:
        save_softmax_npz(softmax_to_f16(softmax, dims, strides), resampled_npz_fname, properties_dict, region_class_order,
                         device_deflate=device_deflate)
    bbox = properties_dict.get('crop_bbox')
    if bbox is not None:
        out_shape = tuple(int(v) for v in properties_dict.get('original_size_of_raw_data'))
        off = [int(bbox[c][0]) for c in range(3)]
    else:
        out_shape, off = tuple(dims), [0, 0, 0]
    seg = torch.zeros(out_shape, dtype=torch.uint8, device=softmax.device)
    regions = None
    if region_class_order is not None:
        regions = torch.tensor([int(c) for c in region_class_order], dtype=torch.int32, device=softmax.device)
    lib().export_argmax_u8(softmax.data_ptr(), seg.data_ptr(), k, int(softmax.stride(0)), dims[0], dims[1], dims[2], strides[0],
                           strides[1], strides[2], out_shape[0], out_shape[1], out_shape[2], off[0], off[1], off[2],
                           regions.data_ptr() if regions is not None else None, len(regions) if regions is not None else 0,
                           _stream())
    if postprocessing is not None:
        from ..postprocessing.connected_components import apply_postprocessing
        for_which_classes, min_valid_object_sizes = postprocessing
        volume_per_voxel = float(np.prod(properties_dict['itk_spacing'], dtype=np.float64))
        seg = apply_postprocessing(seg, for_which_classes, min_valid_object_sizes, volume_per_voxel)
    return seg if keep_on_device else seg.cpu().numpy()


def predict_cases(trainer, params: Sequence[dict], preprocessed: Iterable[Tuple[str, Tuple[np.ndarray, dict]]],
                  writer: Callable[[np.ndarray, str, dict], None], do_tta: bool = True, step_size: float = 0.5,
                  all_in_gpu: bool = False, mixed_precision: bool = True, postprocessing=None, save_npz: bool = False,
                  device_deflate: Union[bool, str] = False):
    """The per-case loop of reference predict_cases (predict.py:273-331) on preprocessed cases
    ``(output_filename, (data [C,X,Y,Z], properties_dict))``; ``writer(seg_uint8, output_filename, properties_dict)``
    stores the label volume (the reference's SimpleITK NIfTI writer, segmentation_export.py:144-148, is host tooling).
    ``postprocessing``: see ``export_segmentation``.  ``save_npz``: ``<case>.npz`` and ``<case>.pkl`` beside every label file
    (predict.py:303-304), what ``inference/ensemble_predictions.py`` merges.  ``device_deflate``: the ``.npz`` is deflated on the
    device, and a writer that carries ``accepts_device = True`` (``nifti.writer``) is called as ``writer(device_seg, output_filename,
    properties_dict, device_deflate=device_deflate)``: it receives the label volume as a device tensor and compresses it there.  Any
    other writer gets the host array as before.  ``True``: the fixed Huffman code; ``"dynamic"``: a code per chunk."""
    done = []
    to_writer = device_deflate and getattr(writer, "accepts_device", False)
    for output_filename, (d, dct) in preprocessed:
        if isinstance(d, str):
            d = np.load(d)
        softmax = predict_case_ensemble(trainer, params, d, do_tta, step_size, all_in_gpu, mixed_precision)
        tb = trainer.plans.get('transpose_backward') if trainer.plans.get('transpose_forward') is not None else None
        seg = export_segmentation(softmax, dct, tb, getattr(trainer, 'regions_class_order', None), postprocessing=postprocessing,
                                  resampled_npz_fname=output_filename[:-7] + ".npz" if save_npz else None,
                                  device_deflate=device_deflate, keep_on_device=to_writer)
        if to_writer:
            writer(seg.contiguous(), output_filename, dct, device_deflate=device_deflate)
        else:
            writer(seg, output_filename, dct)
        done.append(output_filename)
    return done


def nifti_writer():
    """writer(seg_uint8, path, properties) of predict_cases / predict_from_folder: the reference's SimpleITK export
    (segmentation_export.py:144-148) when SimpleITK is importable, else ``<case>.npy`` beside the requested ``.nii.gz`` path."""
    try:
        import SimpleITK as sitk
    except ImportError:
        sitk = None

    def write(seg, path, props):
        if sitk is None:
            np.save(path[:-7] + ".npy" if path.endswith(".nii.gz") else path + ".npy", seg)
            return
        img = sitk.GetImageFromArray(seg.astype(np.uint8))
        img.SetSpacing(props['itk_spacing'])
        img.SetOrigin(props['itk_origin'])
        img.SetDirection(props['itk_direction'])
        sitk.WriteImage(img, path)
    return write


def check_input_folder_and_return_caseIDs(input_folder: str, expected_num_modalities: int):
    """Case identifiers of an input folder.  Two layouts are served:
      * PREPROCESSED cases (what the reference's GenericPreprocessor writes): ``<case>.npz`` (or ``<case>.npy``) holding
        [modalities (+ seg), X, Y, Z] plus ``<case>.pkl`` with the properties dict -- returned as (ids, "preprocessed");
      * the reference's raw layout ``<case>_XXXX.nii.gz`` (predict.py:631-672) -- returned as (ids, "nifti"); these cases are
        read by a ``reader`` callback and preprocessed on the device (``trainer.preprocess_patient``)."""
    files = sorted(os.listdir(input_folder))
    nii = [f for f in files if f.endswith(".nii.gz")]
    if nii:
        ids = sorted({f[:-12] for f in nii})
        missing = [c + "_%04.0d.nii.gz" % n for c in ids for n in range(expected_num_modalities)
                   if not os.path.isfile(os.path.join(input_folder, c + "_%04.0d.nii.gz" % n))]
        if missing:
            print("Some files are missing:")
            print(missing)
            raise RuntimeError("missing files in input_folder")
        return ids, "nifti"
    ids = sorted({f[:-4] for f in files if (f.endswith(".npz") or (f.endswith(".npy") and not f.endswith("_segs.npy")))
                  and os.path.isfile(os.path.join(input_folder, f[:-4] + ".pkl"))})
    return ids, "preprocessed"


def default_seg_reader():
    """``seg_reader(path_nii_gz) -> label array`` of ``predict_from_folder(lowres_segmentations=...)``: SimpleITK when importable,
    else ``<case>.npy`` beside the requested ``.nii.gz`` path"""
    try:
        import SimpleITK as sitk
    except ImportError:
        sitk = None

    def read(path):
        if sitk is not None and os.path.isfile(path):
            return sitk.GetArrayFromImage(sitk.ReadImage(path))
        return np.load(path[:-7] + ".npy")
    return read


def append_lowres_segmentation(d, seg_prev, num_classes: int, transpose_forward: Sequence[int], original_shape=None, what: str = ""):
    """The cascade's network input of one case (reference predict.py:52-62): ``seg_prev``, the previous stage's label volume in the
    raw geometry, is checked against the image's array shape, transposed by ``transpose_forward``, resized to the preprocessed shape
    ``d.shape[1:]`` with the per-label linear resize (``resize_segmentation(order=1)``, ``e2e_pp_resize_seg``) and appended to ``d``
    [C, X, Y, Z] as ``num_classes - 1`` one-hot channels (``e2e_seg_onehot``).  Kept as the reference has it: the UNCROPPED volume is
    resized to the cropped-and-resampled shape.  ``d``: a numpy array (a numpy array comes back) or a device tensor."""
    from ..preprocessing.preprocessing import resample_data_or_seg
    from ..training.data_augmentation.pyramid_augmentations import seg_onehot
    s = torch.as_tensor(np.asarray(seg_prev.cpu()) if torch.is_tensor(seg_prev) else np.asarray(seg_prev))
    if original_shape is not None:
        assert all(int(i) == int(j) for i, j in zip(s.shape, original_shape)) and s.dim() == len(original_shape), \
            "image and segmentation from previous stage don't have the same pixel array shape! image: %s, seg_prev: %s (%s)" \
            % (tuple(int(v) for v in original_shape), tuple(s.shape), what)
    was_numpy = not torch.is_tensor(d)
    x = torch.as_tensor(d, dtype=torch.float32).cuda()
    s = s.to("cuda", torch.float32).permute(*[int(i) for i in transpose_forward])
    s = resample_data_or_seg(s[None], [int(v) for v in x.shape[1:]], is_seg=True, order=1).contiguous()
    labels = list(range(1, int(num_classes)))
    c = int(x.shape[0])
    out = torch.empty((1, c + len(labels)) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
    out[0, :c].copy_(x)
    seg_onehot(s[None], 0, labels, out, c)
    return out[0].cpu().numpy() if was_numpy else out[0]


def predict_from_folder(model: str, input_folder: str, output_folder: str, folds: Union[Tuple[int], List[int], None],
                        save_npz: bool, num_threads_preprocessing: int, num_threads_nifti_save: int,
                        lowres_segmentations: Union[str, None], part_id: int, num_parts: int, tta: bool,
                        mixed_precision: bool = True, overwrite_existing: bool = True, mode: str = 'normal',
                        overwrite_all_in_gpu: bool = None, step_size: float = 0.5,
                        checkpoint_name: str = "model_final_checkpoint", segmentation_export_kwargs: dict = None,
                        disable_postprocessing: bool = False, writer=None, reader=None, device_deflate: Union[bool, str] = False,
                        seg_reader=None):
    """reference predict.py:675-764 with the same arguments: the cases ``[part_id::num_parts]`` of ``input_folder`` through
    ``load_model_and_checkpoint_files`` (model_restore.py:108-154) -> fold ensemble -> export, written to ``output_folder``.
    The per-case work is ``predict_cases`` above (softmax resident in HBM).  ``num_threads_*`` are accepted and unused: there are
    no preprocessing / export worker processes here.  ``save_npz`` (``simple_predict -z``): the class probabilities of every case are
    stored beside its label file for ``inference/ensemble_predictions.py`` (``save_softmax_npz``).  Unless ``disable_postprocessing``, ``<model>/postprocessing.json`` is copied to
    ``output_folder`` and applied to every case on the device (reference :337-356); when the file is missing the reference's warning
    is printed and the raw label maps are written.  A folder of raw cases (``<case>_XXXX.nii.gz``) is read through
    ``reader(list_of_files) -> (data [C, X, Y, Z], properties)`` -- default: the reference's SimpleITK loader -- and preprocessed on
    the device by ``trainer.preprocess_patient``; without a reader such a folder is refused before anything is loaded.
    ``device_deflate`` (``simple_predict --device_deflate``): see ``predict_cases``.

    ``lowres_segmentations`` (the cascade's second stage, reference :714-719): a folder with ``<case_id>.nii.gz`` of every case, the
    ``3d_lowres`` model's prediction in the raw geometry, read through ``seg_reader(path) -> label array`` (default: SimpleITK, else
    ``<case_id>.npy`` of the same stem) and appended to the case as one-hot channels (``append_lowres_segmentation``)."""
    import shutil
    from ..training.model_restore import load_model_and_checkpoint_files
    if mode != "normal":
        raise NotImplementedError("mode=%r: the engine implements the reference's 'normal' mode (predict.py:729-737)" % (mode,))
    os.makedirs(output_folder, exist_ok=True)
    assert os.path.isfile(os.path.join(model, "plans.pkl")), "Folder with saved model weights must contain a plans.pkl file"
    shutil.copy(os.path.join(model, 'plans.pkl'), output_folder)
    with open(os.path.join(model, "plans.pkl"), 'rb') as f:
        expected_num_modalities = pickle.load(f)['num_modalities']
    case_ids, layout = check_input_folder_and_return_caseIDs(input_folder, expected_num_modalities)
    if layout == "nifti":
        from ..preprocessing.cropping import require_reader
        reader = require_reader(reader, "predict_from_folder(%s: raw cases, <case>_XXXX.nii.gz)" % input_folder)
    lowres_files = None
    if lowres_segmentations is not None:
        assert os.path.isdir(lowres_segmentations), "if lowres_segmentations is not None then it must point to a directory"
        lowres_files = [os.path.join(lowres_segmentations, i + ".nii.gz") for i in case_ids]
        assert all([os.path.isfile(i) or os.path.isfile(i[:-7] + ".npy") for i in lowres_files]), \
            "not all lowres_segmentations files are present. (I was searching for case_id.nii.gz in that folder)"
        lowres_files = lowres_files[part_id::num_parts]
        seg_reader = default_seg_reader() if seg_reader is None else seg_reader
    case_ids = case_ids[part_id::num_parts]
    output_files = [os.path.join(output_folder, c + ".nii.gz") for c in case_ids]
    if not overwrite_existing:
        keep = [i for i, o in enumerate(output_files) if not (os.path.isfile(o) or os.path.isfile(o[:-7] + ".npy"))
                or (save_npz and not os.path.isfile(o[:-7] + ".npz"))]          # (predict.py:233-234)
        case_ids, output_files = [case_ids[i] for i in keep], [output_files[i] for i in keep]
        lowres_files = [lowres_files[i] for i in keep] if lowres_files is not None else None
    print("number of cases that still need to be predicted:", len(case_ids))
    if not case_ids:
        return []
    trainer, params = load_model_and_checkpoint_files(model, folds, mixed_precision=mixed_precision, checkpoint_name=checkpoint_name)
    all_in_gpu = False if overwrite_all_in_gpu is None else overwrite_all_in_gpu
    postprocessing = None
    if not disable_postprocessing:
        pp_file = os.path.join(model, "postprocessing.json")
        if os.path.isfile(pp_file):
            from ..postprocessing.connected_components import load_postprocessing
            print("postprocessing...")
            shutil.copy(pp_file, os.path.abspath(output_folder))
            postprocessing = load_postprocessing(pp_file)
        else:
            print("WARNING! Cannot run postprocessing because the postprocessing file is missing. Make sure to run "
                  "consolidate_folds in the output folder of the model first!\nThe folder you need to run this in is "
                  "%s\n(python -m e2enet_medical_amd.postprocessing.consolidate_postprocessing -f %s)" % (model, model))

    def with_lowres(i, d, props):
        if lowres_files is None:
            return d
        return append_lowres_segmentation(d, seg_reader(lowres_files[i]), trainer.num_classes, trainer.plans['transpose_forward'],
                                          props.get('original_size_of_raw_data'), lowres_files[i])

    def cases():
        for i, (c, out) in enumerate(zip(case_ids, output_files)):
            if layout == "nifti":
                files = [os.path.join(input_folder, c + "_%04.0d.nii.gz" % n) for n in range(expected_num_modalities)]
                d, _, props = trainer.preprocess_patient(files, reader=reader)
                yield out, (with_lowres(i, d, props), props)
                continue
            npy, npz = os.path.join(input_folder, c + ".npy"), os.path.join(input_folder, c + ".npz")
            d = np.load(npy) if os.path.isfile(npy) else np.load(npz)['data']
            with open(os.path.join(input_folder, c + ".pkl"), 'rb') as f:
                props = pickle.load(f)
            d = np.asarray(d)[:expected_num_modalities]          # (preprocessed training cases carry their labels as a last channel)
            yield out, (with_lowres(i, d, props), props)
    return predict_cases(trainer, params, cases(), writer if writer is not None else nifti_writer(), do_tta=tta,
                         step_size=step_size, all_in_gpu=all_in_gpu, mixed_precision=mixed_precision, postprocessing=postprocessing,
                         save_npz=save_npz, device_deflate=device_deflate)
