"""``verify_dataset_integrity`` and its helpers under the reference's names (e2enet/preprocessing/sanity_checks.py:25-235): the checks of
``nnUNet_plan_and_preprocess --verify_dataset_integrity`` on a raw task folder, in the reference's order and with its outcomes.

The voxel passes of the reference -- ``np.isnan`` over every image and label, ``np.unique`` over every label, each on a host array
SimpleITK has converted -- are one kernel here: a file is inflated by ``nifti.read_raw`` (host threads, ahead of the device), its
stored bytes are uploaded once and ``nifti.scan`` brings back the NaN count, the count of values that are no labels and the 256
label counts (csrc/nifti.hip).  A label file is read once, for the NaN check and the label check both.  Files are read with this
package's NIfTI-1 reader whether or not ``--native_nifti`` is given: the scan needs the stored bytes; a file that reader refuses is
its ``ValueError``.  Geometry and orientation are host arithmetic on the headers.  ``reorient_to_RAS`` is not part of this package."""
import json
import os
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from .. import nifti
from .preprocessing import DEFAULT_NUM_THREADS

MAX_READER_THREADS = 16
AXIS_CODES = (("L", "R"), ("P", "A"), ("I", "S"))          # per world axis of RAS+: the voxel axis runs against it, with it


def axcodes_of_direction(itk_direction):
    """The axis codes of a volume from the 9 numbers of its ITK (LPS) direction matrix, e.g. ``('R', 'A', 'S')``: voxel axis by voxel
    axis (x first), the world axis of RAS+ along which that axis moves most, among those no earlier voxel axis took, and the sign of
    the movement.  (The reference asks nibabel's ``aff2axcodes`` of the affine; for a direction matrix whose columns each have one
    dominant component this is the same answer.)"""
    ras = np.diag([-1., -1., 1.]) @ np.array(itk_direction, dtype=np.float64).reshape(3, 3)
    free, codes = [0, 1, 2], []
    for voxel_axis in range(3):
        world = max(free, key=lambda w: abs(ras[w, voxel_axis]))
        free.remove(world)
        codes.append(AXIS_CODES[world][1 if ras[world, voxel_axis] > 0 else 0])
    return tuple(codes)


def _same_orientation(directions):
    if len(directions) == 0:
        return True, np.zeros((0, 3), dtype="<U1")
    orientations = np.array([axcodes_of_direction(d) for d in directions])
    unique_orientations = np.unique(orientations, axis=0)
    return len(unique_orientations) == 1, unique_orientations


def verify_all_same_orientation(folder):
    """``(all_same, unique_orientations)`` of the ``.nii.gz`` files of a folder"""
    nii_files = sorted(os.path.join(folder, f) for f in os.listdir(folder) if f.endswith(".nii.gz"))
    return _same_orientation([nifti.read_raw(n).itk_direction for n in nii_files])


def verify_same_geometry(img_1, img_2):
    """Two volumes (``NiftiRaw``, or anything with ``itk_origin``, ``itk_spacing``, ``itk_direction`` and ``shape``) share origin,
    spacing, direction and size within ``np.isclose``; what does not match is printed"""
    same = True
    for message, a, b in (("the origin does not match between the images:", img_1.itk_origin, img_2.itk_origin),
                          ("the spacing does not match between the images", img_1.itk_spacing, img_2.itk_spacing),
                          ("the direction does not match between the images", img_1.itk_direction, img_2.itk_direction),
                          # (the size as ITK reports it: x, y, z)
                          ("the size does not match between the images", tuple(img_1.shape)[::-1], tuple(img_2.shape)[::-1])):
        if not np.all(np.isclose(a, b)):
            print(message)
            print(a)
            print(b)
            same = False
    return same


def _value_at(raw, index):
    """the fp32 value of voxel ``index`` of a ``NiftiRaw``, from the host payload (numpy's arithmetic: the decode's rule)"""
    dt = np.dtype(nifti.DATATYPES[raw.datatype][0])
    if isinstance(raw.payload, nifti.DeferredPayload):
        raw = nifti.read_raw(raw.path)                 # (a report about one bad file: the host inflates it after all)
    stored = raw.payload[index * raw.elsize:(index + 1) * raw.elsize].view(dt.newbyteorder("S") if raw.swap else dt)[0]
    with np.errstate(over="ignore", invalid="ignore"):
        if raw.scale:
            return np.float32(np.float64(stored) * raw.slope + raw.inter)
        return np.float32(stored)


def _unexpected_labels(raw, scan, valid_labels):
    """``(ok, invalid_values)`` of a scanned label file: the label values that occur and are not expected, then the first value that is
    no label at all, then NaN"""
    invalid = [int(v) for v in np.nonzero(scan.histogram)[0] if int(v) not in valid_labels]
    if scan.non_label_count > 0:
        value = _value_at(raw, scan.first_non_label)
        print("%s: %d voxel(s) are no whole-number labels in [0, 255], the first at raster index %d with the value %r"
              % (raw.path, scan.non_label_count, scan.first_non_label, float(value)))
        invalid.append(float(value))
    if scan.nan_count > 0:
        invalid.append(float("nan"))
    return len(invalid) == 0, invalid


def verify_contains_only_expected_labels(itk_img, valid_labels):
    """``(ok, invalid_values)`` of a label file: ok when every voxel is one of ``valid_labels``"""
    raw = nifti.read_raw(itk_img)
    return _unexpected_labels(raw, nifti.scan(raw), valid_labels)


def _read_ahead(pool, depth, groups, inflate="host"):
    """``nifti.read_raw`` of a sequence of file groups on the threads of ``pool``, at most ``depth`` groups ahead of the consumer.
    ``groups`` yields (key, [files]) or (key, an exception: what is wrong with the group); this yields (key, [NiftiRaw]) or that pair
    as it is, in order; nothing behind an exception is read."""
    pending, groups, more = deque(), iter(groups), True
    while True:
        while more and len(pending) < depth:
            item = next(groups, None)
            if item is None or isinstance(item[1], Exception):
                more = False
            if item is not None:
                key, files = item
                pending.append((key, files if isinstance(files, Exception) else [pool.submit(nifti.read_raw, f, inflate) for f in files]))
        if not pending:
            return
        key, futures = pending.popleft()
        yield key, (futures if isinstance(futures, Exception) else [f.result() for f in futures])


def verify_dataset_integrity(folder, num_threads=DEFAULT_NUM_THREADS, inflate="host"):
    """The reference's checks of a raw task folder (``dataset.json``, ``imagesTr``, ``labelsTr``, ``imagesTs`` when there is a test
    set): every listed file is there and none besides; per training case the geometry of every modality against the label, NaNs in the
    label, NaNs in every image; the declared labels start at 0 and are consecutive; no label file holds another value; the modalities
    of a test case share one geometry; the axis orientations.  AssertionError for missing files and wrong labels, RuntimeError for
    NaNs (after every case was listed), ``Warning`` raised for a geometry mismatch -- as in the reference.  ``num_threads`` host
    threads (at most 16) inflate files ahead; this thread uploads and scans.  Neither the report nor the outcome depends on them.
    ``inflate="device"`` (``--inflate_any``): the threads only read the files, the payloads are inflated on the GPU
    (``nifti.read_raw``)."""
    join, isfile = os.path.join, os.path.isfile
    assert isfile(join(folder, "dataset.json")), "There needs to be a dataset.json file in folder, folder=%s" % folder
    assert os.path.isdir(join(folder, "imagesTr")), "There needs to be a imagesTr subfolder in folder, folder=%s" % folder
    assert os.path.isdir(join(folder, "labelsTr")), "There needs to be a labelsTr subfolder in folder, folder=%s" % folder
    with open(join(folder, "dataset.json")) as f:
        dataset = json.load(f)
    training_cases = dataset['training']
    num_modalities = len(dataset['modality'].keys())
    test_cases = dataset['test']
    expected_train_identifiers = [i['image'].split("/")[-1][:-7] for i in training_cases]
    expected_test_identifiers = [i.split("/")[-1][:-7] for i in test_cases]

    nii_files_in_imagesTr = sorted(f for f in os.listdir(join(folder, "imagesTr")) if f.endswith(".nii.gz"))
    nii_files_in_labelsTr = sorted(f for f in os.listdir(join(folder, "labelsTr")) if f.endswith(".nii.gz"))

    if len(expected_train_identifiers) != len(np.unique(expected_train_identifiers)):
        raise RuntimeError("found duplicate training cases in dataset.json")

    workers = max(1, min(int(num_threads), MAX_READER_THREADS))
    label_files, label_results, directions = [], [], []
    geometries_OK, has_nan = True, False

    def training_files():
        for c in expected_train_identifiers:
            expected_label_file = join(folder, "labelsTr", c + ".nii.gz")
            expected_image_files = [join(folder, "imagesTr", c + "_%04.0d.nii.gz" % i) for i in range(num_modalities)]
            if not isfile(expected_label_file):
                yield c, AssertionError("could not find label file for case %s. Expected file: \n%s" % (c, expected_label_file))
            elif not all([isfile(i) for i in expected_image_files]):
                yield c, AssertionError("some image files are missing for case %s. Expected files:\n %s" % (c, expected_image_files))
            else:
                yield c, [expected_label_file] + expected_image_files

    print("Verifying training set")
    with ThreadPoolExecutor(max_workers=workers) as pool:
        for c, raws in _read_ahead(pool, workers, training_files(), inflate):
            print("checking case", c)
            if isinstance(raws, Exception):
                raise raws
            label, images = raws[0], raws[1:]
            label_files.append(label.path)
            label_scan = nifti.scan(label)
            if label_scan.nan_count > 0:
                has_nan = True
                print("There are NAN values in segmentation %s" % label.path)
            for img in images:
                nans_in_image = nifti.scan(img).nan_count > 0
                has_nan = has_nan or nans_in_image
                directions.append(img.itk_direction)
                if not verify_same_geometry(img, label):
                    geometries_OK = False
                    print("The geometry of the image %s does not match the geometry of the label file. The pixel arrays "
                          "will not be aligned and nnU-Net cannot use this data. Please make sure your image modalities "
                          "are coregistered and have the same geometry as the label" % images[0].path[:-12])
                if nans_in_image:
                    print("There are NAN values in image %s" % img.path)
            for img in images:
                nii_files_in_imagesTr.remove(os.path.basename(img.path))
            nii_files_in_labelsTr.remove(os.path.basename(label.path))
            # (the stored bytes are kept only where the label check will quote a value from them)
            label_results.append((label if label_scan.non_label_count else label._replace(payload=None), label_scan))

        assert len(nii_files_in_imagesTr) == 0, \
            "there are training cases in imagesTr that are not listed in dataset.json: %s" % nii_files_in_imagesTr
        assert len(nii_files_in_labelsTr) == 0, \
            "there are training cases in labelsTr that are not listed in dataset.json: %s" % nii_files_in_labelsTr

        print("Verifying label values")
        expected_labels = sorted(int(i) for i in dataset['labels'].keys())
        assert expected_labels[0] == 0, 'The first label must be 0 and maps to the background'
        labels_valid_consecutive = np.ediff1d(expected_labels) == 1
        assert all(labels_valid_consecutive), \
            'Labels must be in consecutive order (0, 1, 2, ...). The labels %s do not satisfy this restriction' \
            % np.array(expected_labels)[1:][~labels_valid_consecutive]

        fail = False
        print("Expected label values are", expected_labels)
        for label, label_scan in label_results:
            ok, invalid = _unexpected_labels(label, label_scan, expected_labels)
            if not ok:
                print("Unexpected labels found in file %s. Found these unexpected values (they should not be there) %s"
                      % (label.path, invalid))
                fail = True
        if fail:
            raise AssertionError("Found unexpected labels in the training dataset. Please correct that or adjust your dataset.json "
                                 "accordingly")
        print("Labels OK")

        if len(expected_test_identifiers) > 0:
            print("Verifying test set")
            nii_files_in_imagesTs = sorted(f for f in os.listdir(join(folder, "imagesTs")) if f.endswith(".nii.gz"))

            def test_files():
                for c in expected_test_identifiers:
                    expected_image_files = [join(folder, "imagesTs", c + "_%04.0d.nii.gz" % i) for i in range(num_modalities)]
                    if not all([isfile(i) for i in expected_image_files]):
                        yield expected_image_files, AssertionError("some image files are missing for case %s. Expected files:\n %s"
                                                                   % (c, expected_image_files))
                    else:
                        # (a single modality has nothing to agree with: its file is not opened)
                        yield expected_image_files, (expected_image_files if num_modalities > 1 else [])

            for expected_image_files, raws in _read_ahead(pool, workers, test_files(), inflate):
                if isinstance(raws, Exception):
                    raise raws
                for i, img in enumerate(raws[1:]):
                    assert verify_same_geometry(img, raws[0]), "The modalities of the image %s do not seem to be registered. " \
                                                               "Please coregister your modalities." % (expected_image_files[i])
                for i in expected_image_files:
                    nii_files_in_imagesTs.remove(os.path.basename(i))
            assert len(nii_files_in_imagesTs) == 0, \
                "there are training cases in imagesTs that are not listed in dataset.json: %s" % nii_files_in_imagesTs

    all_same, unique_orientations = _same_orientation(directions)
    if not all_same:
        print("WARNING: Not all images in the dataset have the same axis ordering. We very strongly recommend you correct that by "
              "reorienting the data. fslreorient2std should do the trick")
    if not geometries_OK:
        raise Warning("GEOMETRY MISMATCH FOUND! CHECK THE TEXT OUTPUT! This does not cause an error at this point  but you should "
                      "definitely check whether your geometries are alright!")
    else:
        print("Dataset OK")

    if has_nan:
        raise RuntimeError("Some images have nan values in them. This will break the training. See text output above to see which ones")
