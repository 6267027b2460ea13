"""``python -m e2enet_medical_amd.inference.ensemble_predictions -f F1 F2 ... -o OUT [-t N] [-pp FILE] [--npz]`` -- the reference's
ensembling of predictions that were made in separate runs (e2enet/inference/ensemble_predictions.py:26-124): every folder holds, per
case, the class probabilities ``<case>.npz`` (key ``softmax``, fp16) and the properties ``<case>.pkl`` that ``simple_predict -z``
leaves; the probabilities of a case are averaged over the folders and exported as a label volume.

Reference: ``np.vstack`` of the N volumes, ``np.mean`` over them, ``argmax`` (or the region thresholds), a pass for the crop box
(segmentation_export.py:124-140) and, with ``-pp``, one more over the written files for the connected components, all on the host.
Here one kernel (``e2e_merge_softmax_f16``) streams the N volumes once and writes the label byte into the crop box; the stored
post-processing runs on that device volume (``apply_postprocessing``) and the host receives uint8 volumes only.  The mean is numpy's to
the bit -- fp32 sum in folder order, fp32 division, one rounding to fp16 -- and the labels are decided on the fp16 mean, as there.

Only this process opens the GPU.  ``threads`` host threads read and decompress the next cases' ``.npz`` files and write finished cases
while the device works; the files written do not depend on their number."""
import os
import pickle
import shutil
from collections import deque

import numpy as np

from .._lib import E2EError

join, isfile = os.path.join, os.path.isfile

MAX_SOURCES = 16          # E2E_MERGE_MAX_SOURCES: the device pointers travel in the launch arguments
PREFETCH_CASES = 2        # cases whose .npz files are being read ahead of the device: bounds the host memory held
MAX_THREADS = 16


def _refuse_too_many(n):
    if n > MAX_SOURCES:
        raise E2EError("merge_softmax_f16: %d sources, at most %d are merged in one call" % (n, MAX_SOURCES))


def merge_softmax(softmaxes, properties, regions_class_order=None, postprocessing=None, return_mean=False, return_raw=False):
    """The device work for one case: uint8 label volume in the original (uncropped) geometry from N class-probability volumes
    ``[K, A, B, C]`` -- fp16 host arrays or fp16 device tensors -- in the case's own axis order; ``properties`` (of the first source)
    place it.  ``postprocessing``: ``(for_which_classes, min_valid_object_sizes or None)``, applied on the device before the download.
    Returns the volume; with ``return_raw`` the volume before post-processing follows it, with ``return_mean`` the fp16 mean
    ``[K, A, B, C]`` (host array) follows those.

    A shape other than ``properties['size_after_cropping']``: the fp16 mean goes, as fp32, through ``export_segmentation``, i.e. the
    engine's order-1 resampling (the reference would ask for order 3 here and says it never happens)."""
    import ctypes
    import torch
    from .._lib import lib
    from .predict import export_segmentation, _stream
    if len(softmaxes) < 1:
        raise ValueError("merge_softmax: no sources")
    dev = []
    for s in softmaxes:
        if isinstance(s, torch.Tensor):
            if not s.is_cuda or s.dtype != torch.float16:
                raise TypeError("merge_softmax: tensors must be fp16 on the device, got %s on %s" % (s.dtype, s.device))
            dev.append(s.contiguous())
        else:
            s = np.asarray(s)
            if s.dtype != np.float16:
                raise TypeError("merge_softmax: arrays must be float16 (what -z stores), got %s" % s.dtype)
            s = np.ascontiguousarray(s)
            dev.append(torch.from_numpy(s if s.flags.writeable else s.copy()).cuda())          # (torch takes no read-only array)
    shape = tuple(dev[0].shape)
    if len(shape) != 4 or any(tuple(d.shape) != shape for d in dev):
        raise ValueError("merge_softmax: sources differ in shape: %s" % [tuple(d.shape) for d in dev])
    k, dims = shape[0], [int(v) for v in shape[1:]]
    srcs = ctypes.cast((ctypes.c_void_p * len(dev))(*[d.data_ptr() for d in dev]), ctypes.c_void_p)
    regions = None
    if regions_class_order is not None:
        regions = torch.tensor([int(c) for c in regions_class_order], dtype=torch.int32, device=dev[0].device)
    after_crop = properties.get('size_after_cropping')
    resample = after_crop is not None and any(int(a) != int(b) for a, b in zip(dims, after_crop))
    mean = torch.empty(shape, dtype=torch.float16, device=dev[0].device) if (return_mean or resample) else None
    pp = None
    if postprocessing is not None:
        from ..postprocessing.connected_components import apply_postprocessing
        volume_per_voxel = float(np.prod(properties['itk_spacing'], dtype=np.float64))
        pp = lambda v: apply_postprocessing(v, postprocessing[0], postprocessing[1], volume_per_voxel)
    if resample:
        lib().merge_softmax_f16(srcs, len(dev), k, dims[0], dims[1], dims[2], None, 0, 0, 0, 0, 0, 0, None, 0, mean.data_ptr(), _stream())
        raw = export_segmentation(mean.float(), properties, None, regions_class_order)
        seg = raw if pp is None else pp(torch.from_numpy(raw).cuda()).cpu().numpy()
    else:
        bbox = properties.get('crop_bbox')
        if bbox is not None:
            out_shape = tuple(int(v) for v in properties.get('original_size_of_raw_data'))
            off = [int(bbox[c][0]) for c in range(3)]
        else:
            out_shape, off = tuple(dims), [0, 0, 0]
        vol = torch.zeros(out_shape, dtype=torch.uint8, device=dev[0].device)
        lib().merge_softmax_f16(srcs, len(dev), k, dims[0], dims[1], dims[2], vol.data_ptr(), out_shape[0], out_shape[1], out_shape[2],
                                off[0], off[1], off[2], regions.data_ptr() if regions is not None else None,
                                len(regions) if regions is not None else 0, mean.data_ptr() if mean is not None else None, _stream())
        raw = vol.cpu().numpy() if (pp is None or return_raw) else None
        seg = raw if pp is None else pp(vol).cpu().numpy()
    out = (seg,) + ((raw,) if return_raw else ()) + ((mean.cpu().numpy(),) if return_mean else ())
    return out[0] if len(out) == 1 else out


def _load_softmax(f):
    return np.load(f)['softmax']


def _read_raw(f):
    """the read-ahead half of ``--device_inflate``: file bytes, zip directory and .npy headers; no device"""
    from .. import deflate
    return deflate.read_npz_raw(f)


def _inflate_softmax(raw, foreign="host"):
    """the other half, on the thread that owns the GPU: ``softmax`` of one file as a device tensor.  A file that the device
    encoder did not write is inflated on the host inside ``load_npz`` -- with ``foreign="device"`` only where ``inflate_any`` does
    not serve it."""
    from .. import deflate
    return deflate.load_npz(raw, keys=("softmax",), foreign=foreign)["softmax"]


def _load_properties(f):
    with open(f, 'rb') as fh:
        return pickle.load(fh)


def _common_regions_class_order(props, files):
    """ensemble_predictions.py:33-45"""
    reg_class_orders = [p['regions_class_order'] if 'regions_class_order' in p.keys() else None for p in props]
    if all(i is None for i in reg_class_orders):
        return None
    tmp = reg_class_orders[0]
    for r in reg_class_orders[1:]:
        assert tmp == r, 'If merging files with regions_class_order, the regions_class_orders of all ' \
                         'files must be the same. regions_class_order: %s, \n files: %s' % (str(reg_class_orders), str(files))
    return tmp


def _merge_loaded(softmax, props, files, store_npz, postprocessing):
    """device work of one case on what the loaders read: ``(seg, raw or None, mean or None)``"""
    shapes = [tuple(s.shape) for s in softmax]
    if any(s != shapes[0] for s in shapes):
        raise ValueError("the class probabilities of one case differ in shape: %s\n files: %s" % (str(shapes), str(files)))
    regions_class_order = _common_regions_class_order(props, files)
    res = merge_softmax(softmax, props[0], regions_class_order, postprocessing, return_mean=store_npz,
                        return_raw=postprocessing is not None)
    res = list(res) if isinstance(res, tuple) else [res]
    seg = res.pop(0)
    raw = res.pop(0) if postprocessing is not None else None
    return seg, raw, (res.pop(0) if store_npz else None)


def _write_case(seg, raw, mean, props, out_file, postprocessed_file, writer):
    if raw is None:
        writer(seg, out_file, props[0])
    else:
        writer(raw, out_file, props[0])
        writer(seg, postprocessed_file, props[0])
    if mean is not None:
        np.savez_compressed(out_file[:-7] + ".npz", softmax=mean)
        with open(out_file[:-7] + ".pkl", 'wb') as f:
            pickle.dump(props, f)


def _written(out_file):
    return isfile(out_file) or isfile(out_file[:-7] + ".npy")          # (nifti_writer without SimpleITK stores <case>.npy)


def merge_files(files, properties_files, out_file, override, store_npz, writer=None, postprocessing=None, postprocessed_file=None,
                device_inflate=False):
    """Reference :26-53 for one case.  ``postprocessing`` (as ``load_postprocessing`` returns it) with ``postprocessed_file``: the raw
    label volume goes to ``out_file`` and the post-processed one to ``postprocessed_file``.  ``device_inflate``: as in ``merge``."""
    from .predict import nifti_writer
    from .. import deflate
    foreign = deflate.foreign_of(device_inflate, "merge_files: device_inflate")
    _refuse_too_many(len(files))
    if not override and _written(out_file) and (postprocessing is None or _written(postprocessed_file)):
        return
    softmax = [_inflate_softmax(_read_raw(f), foreign) if device_inflate else _load_softmax(f) for f in files]
    props = [_load_properties(f) for f in properties_files]
    seg, raw, mean = _merge_loaded(softmax, props, files, store_npz, postprocessing)
    _write_case(seg, raw, mean, props, out_file, postprocessed_file, writer if writer is not None else nifti_writer())


def merge(folders, output_folder, threads, override=True, postprocessing_file=None, store_npz=False, writer=None,
          device_inflate=False):
    """Reference :56-95.  With ``postprocessing_file`` the raw results go to ``<output_folder>/not_postprocessed``, the post-processed
    ones to ``output_folder``, and the json is copied there.  ``device_inflate``: the read-ahead threads only read the files
    (``deflate.read_npz_raw``) and this thread inflates ``softmax`` on the device (``deflate.load_npz``) where the device encoder
    wrote the file; the files written are those of the default route byte for byte.  ``device_inflate="any"``: files of any other
    writer (``np.savez_compressed``: stock ``-z`` folders) are inflated on the device too (``deflate.inflate_any``)."""
    from concurrent.futures import ThreadPoolExecutor
    from .predict import nifti_writer
    from .. import deflate
    foreign = deflate.foreign_of(device_inflate, "merge: device_inflate")
    writer = writer if writer is not None else nifti_writer()
    _refuse_too_many(len(folders))
    os.makedirs(output_folder, exist_ok=True)
    postprocessing, output_folder_orig = None, None
    if postprocessing_file is not None:
        from ..postprocessing.connected_components import load_postprocessing
        postprocessing = load_postprocessing(postprocessing_file)
        output_folder_orig = output_folder
        output_folder = join(output_folder, 'not_postprocessed')
        os.makedirs(output_folder, exist_ok=True)

    patient_ids = sorted({f[:-4] for folder in folders for f in os.listdir(folder)
                          if f.endswith(".npz") and isfile(join(folder, f))})
    for f in folders:
        assert all([isfile(join(f, i + ".npz")) for i in patient_ids]), "Not all patient npz are available in " \
                                                                        "all folders"
        assert all([isfile(join(f, i + ".pkl")) for i in patient_ids]), "Not all patient pkl are available in " \
                                                                        "all folders"
    jobs = []
    for p in patient_ids:
        out_file = join(output_folder, p + ".nii.gz")
        pp_file = join(output_folder_orig, p + ".nii.gz") if postprocessing is not None else None
        if not override and _written(out_file) and (pp_file is None or _written(pp_file)):
            continue
        jobs.append(([join(f, p + ".npz") for f in folders], [join(f, p + ".pkl") for f in folders], out_file, pp_file))

    workers = max(1, min(int(threads), MAX_THREADS))
    with ThreadPoolExecutor(max_workers=workers) as pool:
        loading, writing, todo = deque(), deque(), iter(jobs)

        def read_ahead():
            job = next(todo, None)
            if job is not None:
                loading.append((job, [pool.submit(_read_raw if device_inflate else _load_softmax, f) for f in job[0]]))
        for _ in range(PREFETCH_CASES):
            read_ahead()
        while loading:
            (files, property_files, out_file, pp_file), reads = loading.popleft()
            softmax = [_inflate_softmax(r.result(), foreign) if device_inflate else r.result() for r in reads]
            read_ahead()
            props = [_load_properties(f) for f in property_files]
            seg, raw, mean = _merge_loaded(softmax, props, files, store_npz, postprocessing)
            del softmax
            while len(writing) >= workers:                   # bounds the finished cases held in host memory
                writing.popleft().result()
            writing.append(pool.submit(_write_case, seg, raw, mean, props, out_file, pp_file, writer))
        while writing:
            writing.popleft().result()

    if postprocessing_file is not None:
        shutil.copy(postprocessing_file, output_folder_orig)


def build_parser():
    import argparse
    parser = argparse.ArgumentParser(description="Average the class probabilities that several `simple_predict -z` runs stored and "
                                                 "export one label volume per case.  Connected-component post-processing is "
                                                 "applied only when a postprocessing.json is named with -pp.")
    parser.add_argument('-f', '--folders', nargs='+', required=True,
                        help="the prediction folders; each holds <case>.npz and <case>.pkl for every case")
    parser.add_argument('-o', '--output_folder', required=True, type=str, help="folder for the merged label volumes")
    parser.add_argument('-t', '--threads', required=False, default=2, type=int,
                        help="host threads that read the npz files ahead of the device and write its results")
    parser.add_argument('-pp', '--postprocessing_file', required=False, type=str, default=None,
                        help="postprocessing.json of the ensemble; the raw results then go to <output_folder>/not_postprocessed")
    parser.add_argument('--npz', action="store_true", required=False,
                        help="also store the averaged probabilities (<case>.npz) and the list of properties (<case>.pkl)")
    parser.add_argument('--device_inflate', action="store_true", required=False,
                        help="inflate the npz files that --device_deflate wrote on the GPU: the threads only read them (other "
                             "files are inflated on the host as before; the label volumes are the same)")
    from .. import nifti
    nifti.add_argument(parser)
    return parser


def select_writer(args, writer=None):
    """the ``writer`` handed to ``merge``: the caller's; with ``--native_nifti`` and none given, ``nifti.writer``"""
    if args.native_nifti and writer is None:
        from .. import nifti
        return nifti.writer
    return writer


def main(argv=None, writer=None):
    args = build_parser().parse_args(argv)
    merge(args.folders, args.output_folder, args.threads, override=True, postprocessing_file=args.postprocessing_file,
          store_npz=args.npz, writer=select_writer(args, writer),
          device_inflate="any" if args.inflate_any else args.device_inflate)           # (--inflate_any implies --device_inflate)


if __name__ == "__main__":
    main()
