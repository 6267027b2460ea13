"""The dataset integrity check on the device: the scan kernel (csrc/nifti.hip, ``e2e_nifti_scan``, ``nifti.scan``) against numpy on
the same stored bytes, word for word; ``sanity_checks.verify_dataset_integrity`` on a tiny raw task folder; and the
``nnUNet_plan_and_preprocess`` command from that folder to the plans file and the stage folders.  The oracle of the voxel rule is
tests/nifti_oracle.py."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

from e2enet_medical_amd import nifti
from tests import nifti_oracle as no

pytestmark = pytest.mark.gpu

E2E_ERR_ARG = -1
WORDS = 4 + 256
SCALINGS = [(0, 1.0, 0.0), (1, 0.5, 1.0), (1, 1.0 / 3.0, 0.1)]       # stored as it is; whole for even values; hardly ever whole
BLOCK = 256                                                          # lanes of a workgroup of nifti_scan_kernel
VEC_BYTES = 16                                                       # its load per lane
UNROLL = 4                                                           # SCAN_UNROLL: loads a lane requests at a time
MAX_BLOCKS = 1024                                                    # SCAN_MAX_BLOCKS


def _lib():
    from e2enet_medical_amd._lib import lib
    return lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _oracle(stored, scale, slope, inter):
    """the 260 words numpy gives: voxel_rule for the value, np.isnan, the whole-number rule, np.bincount, the first indices"""
    v = no.voxel_rule(np.ascontiguousarray(stored).ravel(), scale, slope, inter)
    nan = np.isnan(v)
    with np.errstate(invalid="ignore"):
        label = ~nan & (v >= 0) & (v <= 255) & (v == np.trunc(v))
    other = ~nan & ~label
    words = np.zeros(WORDS, dtype=np.int64)
    words[0], words[2] = nan.sum(), other.sum()
    words[1] = np.argmax(nan) if nan.any() else -1
    words[3] = np.argmax(other) if other.any() else -1
    words[4:] = np.bincount(v[label].astype(np.int64), minlength=256)
    assert words[0] + words[2] + words[4:].sum() == v.size
    return words


def _scan_words(stored, datatype, order="<", scale=0, slope=1.0, inter=0.0, lead=0):
    """the stored values in the file's byte order -> upload -> e2e_nifti_scan -> the 260 words as int64 (~0 reads -1).  ``lead``:
    elements by which the payload starts behind a 16-byte boundary.  The words are pre-filled with a pattern the call must replace."""
    stored = np.ascontiguousarray(stored).ravel()
    payload = np.frombuffer(no.voxel_bytes(stored, order), dtype=np.uint8)
    skip = lead * stored.dtype.itemsize
    buf = torch.zeros(skip + payload.size + 64, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % VEC_BYTES == 0
    buf[skip:skip + payload.size] = torch.from_numpy(payload.copy()).cuda()
    out = torch.full((WORDS,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    swap = int((order == "<") != np.little_endian)
    _lib().nifti_scan(buf.data_ptr() + skip, stored.size, datatype, swap, scale, slope, inter, out.data_ptr(), _stream())
    return out.cpu().numpy()


def _label_like(dt, nvox, seed):
    """nvox stored values of a type: mostly labels (so that the histogram is busy), one in eight anything the type holds, and for
    the floats halves, infinities and NaNs in between"""
    dt = np.dtype(dt)
    rng = np.random.RandomState(seed)
    top = 127 if dt == np.int8 else 255
    vals = rng.randint(0, top + 1, nvox).astype(dt)
    wild = rng.rand(nvox) < 0.125
    if dt.kind in "iu":
        bits = rng.randint(0, 256, nvox * dt.itemsize, dtype=np.uint8).view(dt)
        vals[wild] = (bits >> rng.randint(0, 8 * dt.itemsize, nvox).astype(dt))[wild]
    else:
        pool = np.array([0.5, -1.0, 256.0, np.nan, np.inf, -np.inf, -0.0, 254.5, 1e9, -3.25], dtype=dt)
        vals[wild] = pool[rng.randint(0, len(pool), nvox)][wild]
    return vals


def _check(stored, datatype, order, scale, slope, inter, lead=0):
    want = _oracle(stored, scale, slope, inter)
    got = _scan_words(stored, datatype, order, scale, slope, inter, lead)
    diff = np.nonzero(got != want)[0]
    assert diff.size == 0, "datatype %d order %s nvox %d scale %d slope %r inter %r lead %d: %d words differ, first word %d: got %d want %d" % (
        datatype, order, stored.size, scale, slope, inter, lead, diff.size, diff[0], got[diff[0]], want[diff[0]])
    return want


@pytest.mark.parametrize("order", ["<", ">"])
@pytest.mark.parametrize("datatype", list(no.NUMPY))
def test_scan_equals_numpy_word_for_word(datatype, order):
    dt = np.dtype(no.NUMPY[datatype])
    per = VEC_BYTES // dt.itemsize                                # elements of one lane load
    block = BLOCK * UNROLL * per                                  # voxels of one workgroup in one step of its unrolled walk
    grid = _lib().nifti_scan_grid_voxels(datatype)                # voxels of the whole grid in one such step
    assert grid == MAX_BLOCKS * block
    # ... one lane load; one workgroup with the last lane's fourth vector missing / whole / one more voxel; several workgroups with
    # unrolled steps and single ones; 36465 voxels, no multiple of anything; one full grid, a second step for some lanes, a tail
    sizes = [1, 3 * 5 * 7, per - 1, per + 1, block - per, block - 1, block, block + 1, 3 * block - 5 * per - 3, 17 * 33 * 65,
             grid + 3 * block // 4 + per + 1]
    seen = np.zeros(WORDS, dtype=np.int64)
    for nvox in sizes:
        if nvox < 1:                                              # (16 / elsize - 1 of an 8-byte type is 1; never below 1)
            continue
        stored = _label_like(dt, nvox, seed=datatype + nvox)
        for scale, slope, inter in SCALINGS:
            seen += _check(stored, datatype, order, scale, slope, inter) > 0
    assert seen[4:4 + (128 if dt == np.int8 else 256)].all() and seen[2] > 0 and (dt.kind != "f" or seen[0] > 0)          # every word was exercised


@pytest.mark.parametrize("datatype", list(no.NUMPY))
def test_scan_of_a_payload_that_starts_off_a_vector_boundary(datatype):
    """the head: the elements in front of the first 16-byte boundary, also when they are the whole volume"""
    dt = np.dtype(no.NUMPY[datatype])
    per = VEC_BYTES // dt.itemsize
    for lead in sorted({1, per - 1}):
        for nvox in sorted({1, per - lead, per - lead + 1, 3 * per + 2, 5003}):
            stored = _label_like(dt, nvox, seed=7 * datatype + nvox + lead)
            _check(stored, datatype, "<", 0, 1.0, 0.0, lead=lead)
            _check(stored, datatype, ">", 1, 0.5, 1.0, lead=lead)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_scan_specials_of_the_floats(dtype):
    n = 3 * 4096 + 5
    vol = (np.arange(n) % 200).astype(dtype)
    places = {0: np.nan, n - 1: np.nan, 10: np.inf, 11: -np.inf, 12: -0.0, 13: 255.0, 14: 256.0, 15: -1.0, 16: 0.5, 5001: np.nan}
    for i, v in places.items():
        vol[i] = v
    w = _check(vol, [k for k, v in no.NUMPY.items() if v == dtype][0], "<", 0, 1.0, 0.0)
    assert w[0] == 3 and w[1] == 0 and w[2] == 5 and w[3] == 10 and w[4 + 255] == 1
    assert w[4 + 0] == np.count_nonzero(np.arange(n) % 200 == 0) - 1 + 1          # less the NaN at 0, plus the -0.0
    # the only NaN is the last voxel, the only non-label the one before it: both in the tail
    vol[0], vol[5001] = 3.0, 4.0
    vol[10:17] = 1.0
    vol[n - 2] = 0.5
    w = _check(vol, [k for k, v in no.NUMPY.items() if v == dtype][0], ">", 0, 1.0, 0.0)
    assert (w[0], w[1], w[2], w[3]) == (1, n - 1, 1, n - 2)


def test_scan_of_64_bit_integers_beyond_2_to_the_53():
    big = [2 ** 53 + 1, 2 ** 53 + 3, 2 ** 62, 2 ** 63 - 1, 255, 256, 0, 3]
    w = _check(np.array(big + [-1, -2 ** 63, -(2 ** 53 + 1)], dtype=np.int64), 1024, "<", 0, 1.0, 0.0)
    assert w[2] == 8 and w[3] == 0 and w[4 + 255] == w[4] == w[4 + 3] == 1
    w = _check(np.array(big + [2 ** 64 - 1, 2 ** 63 + 2 ** 39], dtype=np.uint64), 1280, ">", 0, 1.0, 0.0)
    assert w[2] == 7 and w[0] == 0
    # scaled back into the labels: (2^54 + 2^10) * 2^-50 is 16 + 2^-40 in fp64 and 16 in fp32
    w = _check(np.array([2 ** 54 + 2 ** 10, 2 ** 54], dtype=np.int64), 1024, "<", 1, 2.0 ** -50, 0.0)
    assert w[4 + 16] == 2 and w[2] == 0


def test_scan_of_a_scaled_int16():
    stored = (np.arange(5000) % 400 - 100).astype(np.int16)
    w = _check(stored, 4, "<", 1, 2.0, 100.0)                     # whole everywhere: -100 .. 698 in steps of 2
    assert w[2] == np.count_nonzero((2 * stored.astype(int) + 100 < 0) | (2 * stored.astype(int) + 100 > 255)) and w[4 + 101] == 0
    w = _check(stored, 4, ">", 1, 0.25, 0.0)                      # whole for one stored value in four
    assert w[4 + 5] == np.count_nonzero(stored == 20) and w[2] > w[4:].sum()
    w = _check(stored, 4, "<", 1, 0.3, 0.05)                      # whole nowhere
    assert w[4:].sum() == 0 and w[2] == stored.size and w[3] == 0


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.float32])
def test_scan_histogram_is_exact_under_contention(dtype):
    """2^20 voxels of one value (every lane of every wave adds to one bin), and of two alternating values"""
    n = 1 << 20
    datatype = [k for k, v in no.NUMPY.items() if v == dtype][0]
    w = _check(np.full(n, 3, dtype=dtype), datatype, "<", 0, 1.0, 0.0)
    assert w[4 + 3] == n and w.sum() == n - 2
    two = np.full(n, 0, dtype=dtype)
    two[1::2] = 7
    w = _check(two, datatype, "<", 0, 1.0, 0.0)
    assert w[4] == w[4 + 7] == n // 2


def test_scan_twice_gives_the_same_words():
    stored = _label_like(np.float32, 700001, seed=5)
    a = _scan_words(stored, 16)
    b = _scan_words(stored, 16)
    assert a.tobytes() == b.tobytes() and a[0] > 0 and a[2] > 0


def test_scan_of_an_empty_volume_and_the_refusals():
    dll = _lib()._dll
    st = _stream()
    out = torch.full((WORDS,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    _lib().nifti_scan(None, 0, 4, 0, 0, 1.0, 0.0, out.data_ptr(), st)
    w = out.cpu().numpy()
    assert w[1] == w[3] == -1 and w[0] == w[2] == 0 and not w[4:].any()
    raw = torch.zeros(64, dtype=torch.uint8, device="cuda")
    out.fill_(0x5A5A5A5A)
    call = lambda ptr, n, datatype, o=out.data_ptr(): dll.e2e_nifti_scan(ptr, n, datatype, 0, 0, 1.0, 0.0, o, st)
    assert call(raw.data_ptr(), 16, 128) == E2E_ERR_ARG and b"datatype 128" in dll.e2e_last_error()
    assert call(raw.data_ptr(), 16, 32) == E2E_ERR_ARG
    assert call(raw.data_ptr(), 16, 0) == E2E_ERR_ARG
    assert call(raw.data_ptr() + 1, 16, 4) == E2E_ERR_ARG and b"aligned" in dll.e2e_last_error()
    assert call(raw.data_ptr() + 4, 4, 64) == E2E_ERR_ARG
    assert call(raw.data_ptr(), -1, 4) == E2E_ERR_ARG
    assert call(None, 16, 4) == E2E_ERR_ARG
    assert call(raw.data_ptr(), 16, 4, None) == E2E_ERR_ARG
    assert call(raw.data_ptr(), 16, 4, out.data_ptr() + 4) == E2E_ERR_ARG
    assert _lib().nifti_scan_grid_voxels(128) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x5A5A5A5A).all()                # nothing ran
    from e2enet_medical_amd._lib import E2EError
    with pytest.raises(E2EError):
        _lib().nifti_scan(raw.data_ptr(), 16, 128, 0, 0, 1.0, 0.0, out.data_ptr(), st)


def _raw_of(array, slope=0.0, inter=0.0, order="<"):
    """an in-memory NiftiRaw of a numpy array, as read_raw would leave it"""
    datatype = [k for k, v in no.NUMPY.items() if np.dtype(v) == array.dtype][0]
    payload = np.frombuffer(no.voxel_bytes(array, order), dtype=np.uint8).copy()
    scale = slope != 0.0 and not (slope == 1.0 and inter == 0.0)
    return nifti.NiftiRaw("<memory>", tuple(array.shape), datatype, array.dtype.itemsize, (order == "<") != np.little_endian, scale,
                          slope, inter, payload, (1., 1., 1.), (0., 0., 0.), (1., 0., 0., 0., 1., 0., 0., 0., 1.))


def test_scan_agrees_with_decode_u8():
    rng = np.random.RandomState(3)
    labels = rng.randint(0, 256, (9, 31, 37))
    for dtype, order in ((np.uint8, "<"), (np.int16, ">"), (np.float32, "<"), (np.float64, ">")):
        raw = _raw_of(labels.astype(dtype), order=order)
        s = nifti.scan(raw)
        assert isinstance(s, nifti.NiftiScan) and s.histogram.dtype == np.int64 and s.histogram.shape == (256,)
        assert (s.nan_count, s.first_nan, s.non_label_count, s.first_non_label) == (0, -1, 0, -1)
        assert np.array_equal(s.histogram, np.bincount(nifti.decode_u8(raw).cpu().numpy().ravel(), minlength=256))
    # what decode_u8 rejects is what the scan counts in its two counters
    vol = labels.astype(np.float32)
    vol[0, 0, 5], vol[3, 3, 3], vol[8, 30, 36], vol[4, 0, 0] = 0.5, np.nan, 300.0, -2.0
    raw = _raw_of(vol)
    s = nifti.scan(raw)
    dev = torch.from_numpy(raw.payload).cuda()
    out = torch.empty(vol.size, dtype=torch.uint8, device="cuda")
    rejected = torch.zeros(1, dtype=torch.int64, device="cuda")
    _lib().nifti_decode_u8(dev.data_ptr(), vol.size, raw.datatype, 0, 0, 1.0, 0.0, out.data_ptr(), rejected.data_ptr(), _stream())
    assert int(rejected.item()) == s.nan_count + s.non_label_count == 4 and (s.nan_count, s.non_label_count) == (1, 3)
    assert s.first_nan == np.ravel_multi_index((3, 3, 3), vol.shape) and s.first_non_label == 5
    decoded = np.bincount(out.cpu().numpy(), minlength=256)
    decoded[0] -= 4                                               # decode_u8 writes 0 where it rejects
    assert np.array_equal(s.histogram, decoded)


# ------------------------------------------------------------------------------------------------------- verify_dataset_integrity
TASK_ID = "994"
TASK = "Task994_Verify"
TRAIN, TEST = ("vf_b", "vf_a", "vf_c"), ("vf_t",)
PIXDIM = (1., 0.7, 0.8, 2.5, 0., 0., 0., 0.)


def _write_volume(path, vol, order="<", pixdim=PIXDIM, **fields):
    datatype = [k for k, v in no.NUMPY.items() if np.dtype(v) == vol.dtype][0]
    hdr = no.build_header(vol.shape, datatype, order, pixdim=pixdim, qform_code=1, qoffset_x=-90.5, qoffset_y=126.0, qoffset_z=-72.25, **fields)
    no.write_file(path, no.file_bytes(hdr, no.voxel_bytes(vol, order)))


def _case_arrays(ci):
    """an int16 and a float32 modality and uint8 labels 0, 1, 2 of 12 x 14 x (16 - ci): a body inside a zero margin"""
    shape = (12, 14, 16 - ci)
    rng = np.random.RandomState(40 + ci)
    body = np.zeros(shape, dtype=bool)
    body[1:11, 1 + ci:13, 2:15 - ci] = True
    ct = (rng.randint(-1000, 1500, shape) * body).astype(np.int16)
    mr = ((rng.rand(*shape) * 900.0 + 1.0) * body).astype(np.float32)
    zz, yy, xx = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    seg = (((zz // 3 + yy // 4 + xx // 4 + ci) % 3) * body).astype(np.uint8)
    return ct, mr, seg


def _raw_task(base, labels=("0", "1", "2")):
    """the raw task folder under ``base``/nnUNet_raw_data; returns its path"""
    raw = os.path.join(str(base), "nnUNet_raw_data", TASK)
    for sub in ("imagesTr", "labelsTr", "imagesTs"):
        os.makedirs(os.path.join(raw, sub))
    for ci, c in enumerate(TRAIN):
        ct, mr, seg = _case_arrays(ci)
        _write_volume(os.path.join(raw, "imagesTr", c + "_0000.nii.gz"), ct, order=">" if ci else "<")
        _write_volume(os.path.join(raw, "imagesTr", c + "_0001.nii.gz"), mr)
        _write_volume(os.path.join(raw, "labelsTr", c + ".nii.gz"), seg)
    ct, mr, _ = _case_arrays(1)
    _write_volume(os.path.join(raw, "imagesTs", TEST[0] + "_0000.nii.gz"), ct)
    _write_volume(os.path.join(raw, "imagesTs", TEST[0] + "_0001.nii.gz"), mr)
    with open(os.path.join(raw, "dataset.json"), "w") as f:
        json.dump({"modality": {"0": "CT", "1": "MRI"}, "labels": {k: "label" + k for k in labels},
                   "training": [{"image": "./imagesTr/%s.nii.gz" % c, "label": "./labelsTr/%s.nii.gz" % c} for c in TRAIN],
                   "test": ["./imagesTs/%s.nii.gz" % c for c in TEST]}, f)
    return raw


def test_verify_dataset_integrity_outcomes(tmp_path, capsys):
    from e2enet_medical_amd.preprocessing.sanity_checks import verify_contains_only_expected_labels, verify_dataset_integrity
    raw = _raw_task(tmp_path / "clean")
    verify_dataset_integrity(raw, 1)
    report_1 = capsys.readouterr().out
    verify_dataset_integrity(raw, 4)
    report_4 = capsys.readouterr().out
    assert report_1 == report_4 and "Labels OK" in report_1 and report_1.rstrip().endswith("Dataset OK")
    assert [l for l in report_1.splitlines() if l.startswith("checking case")] == ["checking case " + c for c in TRAIN]
    assert "Expected label values are [0, 1, 2]" in report_1 and "WARNING" not in report_1
    label_b = os.path.join(raw, "labelsTr", "vf_b.nii.gz")
    assert verify_contains_only_expected_labels(label_b, [0, 1, 2]) == (True, [])
    assert verify_contains_only_expected_labels(label_b, [0, 2]) == (False, [1])

    ct, mr, seg = _case_arrays(1)
    # a NaN in one image: every case is still listed, then RuntimeError
    raw = _raw_task(tmp_path / "nan_image")
    mr_nan = mr.copy()
    mr_nan[5, 6, 7] = np.nan
    _write_volume(os.path.join(raw, "imagesTr", "vf_a_0001.nii.gz"), mr_nan)
    for threads in (1, 4):
        with pytest.raises(RuntimeError) as e:
            verify_dataset_integrity(raw, threads)
        assert "nan values" in str(e.value)
        out = capsys.readouterr().out
        assert "There are NAN values in image %s" % os.path.join(raw, "imagesTr", "vf_a_0001.nii.gz") in out
        assert "checking case vf_c" in out and "Labels OK" in out and "Dataset OK" in out
        assert threads == 1 or out == first
        first = out

    # a NaN in a float label file: np.unique finds it among the values, so the label check fails first
    raw = _raw_task(tmp_path / "nan_label")
    seg_nan = seg.astype(np.float32)
    seg_nan[0, 0, 0] = np.nan
    _write_volume(os.path.join(raw, "labelsTr", "vf_a.nii.gz"), seg_nan)
    with pytest.raises(AssertionError) as e:
        verify_dataset_integrity(raw, 2)
    assert "unexpected labels" in str(e.value)
    out = capsys.readouterr().out
    assert "There are NAN values in segmentation %s" % os.path.join(raw, "labelsTr", "vf_a.nii.gz") in out
    assert "Unexpected labels found in file %s" % os.path.join(raw, "labelsTr", "vf_a.nii.gz") in out and "nan" in out

    # a label value that dataset.json does not declare
    raw = _raw_task(tmp_path / "label_7")
    seg_7 = seg.copy()
    seg_7[3, 4, 5] = 7
    _write_volume(os.path.join(raw, "labelsTr", "vf_a.nii.gz"), seg_7)
    with pytest.raises(AssertionError) as e:
        verify_dataset_integrity(raw, 2)
    assert "unexpected labels" in str(e.value)
    out = capsys.readouterr().out
    assert "Unexpected labels found in file %s. Found these unexpected values (they should not be there) [7]" % os.path.join(
        raw, "labelsTr", "vf_a.nii.gz") in out and out.count("Unexpected labels found") == 1

    # a label 0.5: no label at all; the count and the value are reported
    raw = _raw_task(tmp_path / "label_half")
    seg_half = seg.astype(np.float64)
    seg_half[2, 3, 4] = 0.5
    seg_half[9, 9, 9] = 0.5
    _write_volume(os.path.join(raw, "labelsTr", "vf_c.nii.gz"), seg_half[:, :, :14], order=">")
    with pytest.raises(AssertionError):
        verify_dataset_integrity(raw, 2)
    out = capsys.readouterr().out
    index = np.ravel_multi_index((2, 3, 4), (12, 14, 14))
    assert "2 voxel(s) are no whole-number labels in [0, 255], the first at raster index %d with the value 0.5" % index in out
    assert "(they should not be there) [0.5]" in out
    assert verify_contains_only_expected_labels(os.path.join(raw, "labelsTr", "vf_c.nii.gz"), [0, 1, 2]) == (False, [0.5])

    # a modality with another spacing: the reference raises a Warning
    raw = _raw_task(tmp_path / "spacing")
    _write_volume(os.path.join(raw, "imagesTr", "vf_a_0000.nii.gz"), ct, pixdim=(1., 0.7, 0.85, 2.5, 0., 0., 0., 0.))
    with pytest.raises(Warning) as e:
        verify_dataset_integrity(raw, 2)
    assert "GEOMETRY MISMATCH" in str(e.value)
    out = capsys.readouterr().out
    assert "the spacing does not match between the images" in out and "The geometry of the image %s does not match" % os.path.join(
        raw, "imagesTr", "vf_a") in out

    # the modalities of a test case disagree
    raw = _raw_task(tmp_path / "test_set")
    _write_volume(os.path.join(raw, "imagesTs", "vf_t_0001.nii.gz"), mr, pixdim=(1., 0.7, 0.8, 3.0, 0., 0., 0., 0.))
    with pytest.raises(AssertionError) as e:
        verify_dataset_integrity(raw, 2)
    assert "do not seem to be registered" in str(e.value)
    capsys.readouterr()

    # a file the reader refuses is the reader's ValueError
    raw = _raw_task(tmp_path / "refused")
    _write_volume(os.path.join(raw, "imagesTr", "vf_c_0000.nii.gz"), ct[:, :, :14], magic=b"ni1\0")
    with pytest.raises(ValueError) as e:
        verify_dataset_integrity(raw, 2)
    assert "vf_c_0000.nii.gz" in str(e.value) and "magic" in str(e.value)


# ------------------------------------------------------------------------------------------------------------------ end to end
def _same_plans(a, b, where="plans"):
    if isinstance(a, dict):
        assert type(a) is type(b) and list(a) == list(b), where
        for k in a:
            _same_plans(a[k], b[k], "%s[%r]" % (where, k))
    elif isinstance(a, (list, tuple)):
        assert type(a) is type(b) and len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _same_plans(x, y, "%s[%d]" % (where, i))
    elif isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), where
    else:
        assert type(a) is type(b) and (a == b or (a != a and b != b)), where


def test_plan_and_preprocess_from_a_raw_folder(tmp_path):
    from e2enet_medical_amd.experiment_planning.experiment_planner_baseline_3DUNet_v21 import ExperimentPlanner3D_v21
    from e2enet_medical_amd.experiment_planning.nnUNet_plan_and_preprocess import main
    mp = pytest.MonkeyPatch()
    try:
        for run, extra in (("full", []), ("plans_only", ["-no_pp"])):
            base, pre = tmp_path / run / "raw_base", tmp_path / run / "preprocessed"
            mp.setenv("nnUNet_raw_data_base", str(base))
            mp.setenv("nnUNet_preprocessed", str(pre))
            mp.setenv("RESULTS_FOLDER", str(tmp_path / run / "results"))
            _raw_task(base)
            main(["-t", TASK_ID, "--verify_dataset_integrity", "--native_nifti", "-tf", "2"] + extra)
            out = os.path.join(str(pre), TASK)
            cropped = os.path.join(str(base), "nnUNet_cropped_data", TASK)
            plans_file = os.path.join(out, "nnUNetPlansv2.1_plans_3D.pkl")
            assert os.path.isfile(plans_file) and os.path.isfile(os.path.join(out, "dataset.json"))
            assert os.path.isfile(os.path.join(out, "dataset_properties.pkl"))
            with open(plans_file, "rb") as f:
                plans = pickle.load(f)
            # the planner run directly on the fingerprint the command wrote
            direct_out = str(tmp_path / run / "direct")
            os.makedirs(direct_out)
            direct = ExperimentPlanner3D_v21(cropped, direct_out)
            direct.plan_experiment()
            direct.plans['preprocessed_data_folder'] = plans['preprocessed_data_folder']
            _same_plans(plans, direct.plans)
            assert plans['num_modalities'] == 2 and plans['all_classes'] == [1, 2] and plans['num_stages'] >= 1
            assert plans['normalization_schemes'] == {0: "CT", 1: "nonCT"} and plans['data_identifier'] == "nnUNetData_plans_v2.1"
            assert sorted(os.path.basename(f)[:-4] for f in plans['list_of_npz_files']) == sorted(TRAIN)
            with open(os.path.join(cropped, "vf_a.pkl"), "rb") as f:
                assert pickle.load(f)['use_nonzero_mask_for_norm'] == plans['use_mask_for_norm']
            stage_folders = [os.path.join(out, "nnUNetData_plans_v2.1_stage%d" % i) for i in range(plans['num_stages'])]
            if extra:
                assert not any(os.path.exists(s) for s in stage_folders) and not os.path.exists(os.path.join(out, "gt_segmentations"))
                continue
            for s in stage_folders:
                assert sorted(os.listdir(s)) == sorted([c + ".npz" for c in TRAIN] + [c + ".pkl" for c in TRAIN])
                data = np.load(os.path.join(s, "vf_a.npz"))["data"]
                assert data.dtype == np.float32 and data.shape[0] == 3 and np.isfinite(data).all()
            assert sorted(os.listdir(os.path.join(out, "gt_segmentations"))) == sorted(c + ".nii.gz" for c in TRAIN)
    finally:
        mp.undo()
