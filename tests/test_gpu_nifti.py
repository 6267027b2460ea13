"""Device half of the native NIfTI-1 I/O (csrc/nifti.hip, e2enet_medical_amd/nifti.py): the decode kernels against numpy's
``astype`` rule bit for bit, the label decode and its rejections, the entry points' refusals, and the callbacks end to end through
``crop_and_fingerprint``, the ``evaluator`` and ``predict_cases``.  The oracle is tests/nifti_oracle.py."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

from e2enet_medical_amd import nifti
from tests import nifti_oracle as no

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
SCALINGS = [(0, 1.0, 0.0), (1, 0.00390625, -1024.0), (1, 1.0 / 3.0, 0.1)]
E2E_ERR_ARG = -1


def _lib():
    from e2enet_medical_amd._lib import lib
    return lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _specials(dt):
    """the values every type is tried on: extremes, values that are not exact in fp32 (ties to even in both directions, just above
    and just below a tie), and for the floats the infinities, NaN and -0.0"""
    dt = np.dtype(dt)
    if dt.kind in "iu":
        info = np.iinfo(dt)
        vals = [info.min, info.max, 0, 1, info.max - 1, info.min + 1]
        cand = [2 ** 24 + 1, 2 ** 24 + 3, 2 ** 24 + 2, 2 ** 25 + 2, 2 ** 25 + 6, 2 ** 31 - 1, 2 ** 31 - 64, 2 ** 31 - 65, 2 ** 31 + 2 ** 7,
                2 ** 31 + 3 * 2 ** 7, 2 ** 32 - 1, 2 ** 32 - 128, 2 ** 32 - 129, 2 ** 53 + 1, 2 ** 53 + 3, 2 ** 40 + 2 ** 16, 2 ** 40 + 3 * 2 ** 16,
                2 ** 40 + 2 ** 16 + 1, 2 ** 40 + 2 ** 16 - 1, 2 ** 63 - 1, 2 ** 63 - 2 ** 38, 2 ** 63 - 2 ** 38 - 1, 2 ** 63, 2 ** 63 + 2 ** 39,
                2 ** 63 + 3 * 2 ** 39, 2 ** 64 - 1, 2 ** 64 - 2 ** 39, 2 ** 64 - 2 ** 39 - 1, 255, 256, 32767, 65535]
        for c in cand:
            vals += [v for v in (c, -c) if info.min <= v <= info.max]
        return np.array(vals, dtype=dt)
    if dt == np.float32:
        return np.array([np.inf, -np.inf, np.nan, -0.0, 0.0, 1.0, -1.0, 3.4028235e38, -3.4028235e38, 1.17549435e-38, 16777216.0, 0.1, 1e-3,
                         255.0, 1024.0, 262144.0], dtype=dt)
    # float64: fp32 halfway points (1 + 2^-24 lies between 1 and 1 + 2^-23) on both sides and exactly on them, overflow, the rest
    h = 2.0 ** -24
    return np.array([np.inf, -np.inf, np.nan, -0.0, 0.0, 1.0 + h, 1.0 + 3 * h, 1.0 + h + 2.0 ** -50, 1.0 + h - 2.0 ** -50, -(1.0 + h),
                     -(1.0 + 3 * h), 1.0 + 3 * h + 2.0 ** -50, 1.0 + 3 * h - 2.0 ** -50, 16777217.0, 16777219.0, 3.4028235e38,
                     3.4028235677973366e38, 3.5e38, -3.5e38, 1e300, -1e300, 0.1, 1.0 / 3.0, 1e-30, 262144.0, 1024.0], dtype=dt)


def _values(dt, nvox, seed):
    """nvox stored values of a type: random over its whole range, the special values at the start (the vector path of a long
    array) and again at the end (its scalar tail)"""
    dt = np.dtype(dt)
    rng = np.random.RandomState(seed)
    if dt.kind in "iu":
        bits = rng.randint(0, 256, nvox * dt.itemsize, dtype=np.uint8).view(dt).copy()
        shift = rng.randint(0, 8 * dt.itemsize, nvox).astype(dt)            # (every magnitude, not only the largest)
        vals = bits >> shift
    else:
        vals = (rng.standard_normal(nvox) * 10.0 ** rng.randint(-6, 7, nvox)).astype(dt)
    sp = _specials(dt)
    n = min(len(sp), nvox)
    vals[:n] = sp[:n]
    if nvox >= 2 * len(sp):
        vals[nvox - len(sp):] = sp
    return vals


def _decode_f32(stored, datatype, order, scale, slope, inter, channels=3):
    """the stored values in the file's byte order -> upload -> e2e_nifti_decode_f32 into channel 1 of a sentinel-filled tensor"""
    nvox = stored.size
    raw = torch.from_numpy(np.frombuffer(no.voxel_bytes(stored, order), dtype=np.uint8).copy()).cuda()
    out = torch.full((channels, nvox), SENTINEL, dtype=torch.float32, device="cuda")
    swap = int((order == "<") != np.little_endian)
    _lib().nifti_decode_f32(raw.data_ptr(), nvox, datatype, swap, scale, slope, inter, out[1].data_ptr(), _stream())
    return out.cpu().numpy()


@pytest.mark.parametrize("order", ["<", ">"])
@pytest.mark.parametrize("datatype", list(no.NUMPY))
def test_decode_f32_is_numpys_astype_bit_for_bit(datatype, order):
    dt = np.dtype(no.NUMPY[datatype])
    per = 16 // dt.itemsize
    sizes = [1, per - 1, per + 1, 4097, 3 * 5 * 7, 33 * 65 * 67]
    for nvox in sizes:
        if nvox < 1:                                              # (16 / elsize - 1 of a 1-byte type is 15; never below 1)
            continue
        stored = _values(dt, nvox, seed=datatype + nvox)
        for scale, slope, inter in SCALINGS:
            want = no.voxel_rule(stored, scale, slope, inter)
            got = _decode_f32(stored, datatype, order, scale, slope, inter)
            what = "datatype %d order %s nvox %d scale %d slope %r inter %r" % (datatype, order, nvox, scale, slope, inter)
            assert (got[0] == SENTINEL).all() and (got[2] == SENTINEL).all(), what + ": wrote outside its channel"
            bad = np.nonzero(got[1].view(np.uint32) != want.view(np.uint32))[0]
            assert bad.size == 0, "%s: %d differ, first at %d: stored %r got %r want %r" % (
                what, bad.size, bad[0], stored[bad[0]], got[1][bad[0]], want[bad[0]])


def test_decode_f32_of_an_empty_volume_launches_nothing():
    out = torch.full((4,), SENTINEL, dtype=torch.float32, device="cuda")
    _lib().nifti_decode_f32(None, 0, 4, 0, 0, 1.0, 0.0, out.data_ptr(), _stream())
    assert (out.cpu().numpy() == SENTINEL).all()


# ------------------------------------------------------------------------------------------------------------------- decode_u8
def _raw_of(array, slope=0.0, inter=0.0, order="<", shape=None):
    """an in-memory NiftiRaw of a numpy array, as read_raw would leave it"""
    datatype = [k for k, v in no.NUMPY.items() if np.dtype(v) == array.dtype][0]
    shape = tuple(array.shape) if shape is None else shape
    payload = np.frombuffer(no.voxel_bytes(array, order), dtype=np.uint8).copy()
    scale = slope != 0.0 and not (slope == 1.0 and inter == 0.0)
    return nifti.NiftiRaw("<memory>", shape, datatype, array.dtype.itemsize, (order == "<") != np.little_endian, scale, slope, inter,
                          payload, (1., 1., 1.), (0., 0., 0.), (1., 0., 0., 0., 1., 0., 0., 0., 1.))


@pytest.mark.parametrize("order", ["<", ">"])
@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.float32, np.float64])
def test_decode_u8_round_trips_every_label(dtype, order):
    labels = np.concatenate([np.arange(256), np.arange(255, -1, -1), np.arange(256)[::3]]).reshape(1, 13, -1)      # 598 = 13 * 46
    got = nifti.decode_u8(_raw_of(labels.astype(dtype), order=order))
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == labels.shape
    assert np.array_equal(got.cpu().numpy(), labels)
    # scaled: stored 2 v + 1 with slope 0.5 and inter -0.5 is v again
    if dtype != np.uint8:
        got = nifti.decode_u8(_raw_of((2 * labels + 1).astype(dtype), slope=0.5, inter=-0.5, order=order))
        assert np.array_equal(got.cpu().numpy(), labels)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_decode_u8_counts_and_zeroes_what_is_no_label(dtype):
    n = 5003                                                      # several workgroups of a 4- or 8-byte type, and a tail
    vol = (np.arange(n) % 251).astype(dtype)
    places = {3: 2.5, 1500: -1.0, 4096: 256.0, n - 1: np.nan}
    for i, v in places.items():
        vol[i] = v
    raw = _raw_of(vol.reshape(1, 1, n))
    dev = torch.from_numpy(raw.payload).cuda()
    out = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    rejected = torch.zeros(1, dtype=torch.int64, device="cuda")
    _lib().nifti_decode_u8(dev.data_ptr(), n, raw.datatype, 0, 0, 1.0, 0.0, out.data_ptr(), rejected.data_ptr(), _stream())
    want = (np.arange(n) % 251).astype(np.uint8)
    want[list(places)] = 0
    assert int(rejected.item()) == 4 and np.array_equal(out.cpu().numpy(), want)
    with pytest.raises(ValueError) as e:
        nifti.decode_u8(raw)
    assert "4 voxel" in str(e.value)
    # a scaling that makes every voxel a label again but the NaN
    ok = np.array([0.5, 1.5, 254.5, np.nan], dtype=dtype)
    with pytest.raises(ValueError) as e:
        nifti.decode_u8(_raw_of(ok.reshape(1, 1, 4), slope=1.0, inter=0.5))
    assert "1 voxel" in str(e.value)
    assert nifti.decode_u8(_raw_of(ok[:3].reshape(1, 1, 3), slope=1.0, inter=0.5)).cpu().tolist() == [[[1, 2, 255]]]


# --------------------------------------------------------------------------------------------------------------------- refusals
def test_entry_points_refuse_without_launching():
    dll = _lib()._dll
    raw = torch.zeros(64, dtype=torch.uint8, device="cuda")
    out = torch.full((16,), SENTINEL, dtype=torch.float32, device="cuda")
    out8 = torch.full((16,), 9, dtype=torch.uint8, device="cuda")
    rejected = torch.zeros(1, dtype=torch.int64, device="cuda")
    st = _stream()
    f32 = lambda ptr, n, datatype: dll.e2e_nifti_decode_f32(ptr, n, datatype, 0, 0, 1.0, 0.0, out.data_ptr(), st)
    u8 = lambda ptr, n, datatype: dll.e2e_nifti_decode_u8(ptr, n, datatype, 0, 0, 1.0, 0.0, out8.data_ptr(), rejected.data_ptr(), st)
    for call in (f32, u8):
        assert call(raw.data_ptr(), 16, 128) == E2E_ERR_ARG       # RGB24
        assert call(raw.data_ptr(), 16, 32) == E2E_ERR_ARG        # COMPLEX64
        assert call(raw.data_ptr(), 16, 0) == E2E_ERR_ARG
        assert call(raw.data_ptr() + 1, 16, 4) == E2E_ERR_ARG     # a 2-byte type one byte off
        assert call(raw.data_ptr() + 2, 8, 16) == E2E_ERR_ARG     # a 4-byte type two bytes off
        assert call(raw.data_ptr() + 4, 4, 64) == E2E_ERR_ARG     # an 8-byte type four bytes off
        assert call(raw.data_ptr(), -1, 4) == E2E_ERR_ARG
        assert call(None, 16, 4) == E2E_ERR_ARG
    assert dll.e2e_nifti_decode_u8(raw.data_ptr(), 16, 2, 0, 0, 1.0, 0.0, out8.data_ptr(), None, st) == E2E_ERR_ARG
    assert f32(raw.data_ptr() + 1, 16, 4) == E2E_ERR_ARG and b"aligned" in dll.e2e_last_error()
    assert f32(raw.data_ptr(), 16, 128) == E2E_ERR_ARG and b"datatype 128" in dll.e2e_last_error()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all() and (out8.cpu().numpy() == 9).all() and int(rejected.item()) == 0
    # a 1-byte type takes any address
    assert f32(raw.data_ptr() + 1, 16, 2) == 0 and (out.cpu().numpy() == 0).all()
    from e2enet_medical_amd._lib import E2EError
    with pytest.raises(E2EError):
        _lib().nifti_decode_f32(raw.data_ptr(), 16, 128, 0, 0, 1.0, 0.0, out.data_ptr(), st)


# -------------------------------------------------------------------------------------------------------------- end to end: crop
TASK = "Task995_NativeNifti"
CASES = ("nn_b", "nn_a")
PIXDIM = (1., 0.7, 0.8, 2.5, 0., 0., 0., 0.)                     # spacing (2.5, 0.8, 0.7) in array-axis order
F32 = lambda v: float(np.float32(v))


def _case_arrays(ci):
    """an int16 and a float32 modality and uint8 labels of 12 x 40 x (48 - 2 ci): a body inside a zero margin"""
    shape = (12, 40, 48 - 2 * ci)
    rng = np.random.RandomState(70 + ci)
    body = np.zeros(shape, dtype=bool)
    body[1 + ci:11, 3:36 - ci, 4:44 - 2 * ci] = True
    ct = (rng.randint(-1000, 1500, shape) * body).astype(np.int16)
    mr = ((rng.rand(*shape) * 900.0 + 1.0) * body).astype(np.float32)
    zz, yy, xx = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    seg = (((zz // 3 + yy // 5 + xx // 4 + ci) % 3) * body).astype(np.uint8)
    return ct, mr, seg


def _write_volume(path, vol, order="<", **fields):
    datatype = [k for k, v in no.NUMPY.items() if np.dtype(v) == vol.dtype][0]
    hdr = no.build_header(vol.shape, datatype, order, pixdim=PIXDIM, qform_code=1, qoffset_x=-90.5, qoffset_y=126.0, qoffset_z=-72.25, **fields)
    no.write_file(path, no.file_bytes(hdr, no.voxel_bytes(vol, order)))


class _ArrayReader(object):
    """the same files handed over as numpy arrays, read by the oracle: what a caller's own NIfTI parser would give"""

    def __call__(self, list_of_files):
        vols, h = [], None
        for f in list_of_files:
            hf, vol = no.read_file(f)
            h = hf if h is None else h
            vols.append(vol)
        spacing = tuple(float(v) for v in h["pixdim"][1:4])
        props = {"original_size_of_raw_data": np.array(vols[0].shape), "original_spacing": np.array(spacing)[[2, 1, 0]],
                 "list_of_data_files": list_of_files, "seg_file": None,
                 "itk_origin": (-float(h["qoffset_x"]), -float(h["qoffset_y"]), float(h["qoffset_z"])), "itk_spacing": spacing,
                 "itk_direction": (-1., 0., 0., 0., -1., 0., 0., 0., 1.)}
        return np.stack(vols), props


def _cropped_folder(folder):
    out = {}
    for c in CASES:
        with open(os.path.join(folder, c + ".pkl"), "rb") as f:
            out[c] = (np.load(os.path.join(folder, c + ".npz")), pickle.load(f))
        out[c] = ({k: out[c][0][k] for k in out[c][0].files}, out[c][1])
    return out


def _same(a, b):
    """two fingerprints hold the same keys, types and numbers"""
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and np.array_equal(np.asarray(a), np.asarray(b), equal_nan=np.asarray(a).dtype.kind == "f")


def test_crop_and_fingerprint_from_real_files_equals_the_array_route(tmp_path):
    from e2enet_medical_amd import paths
    from e2enet_medical_amd.crop_and_fingerprint import main
    mp = pytest.MonkeyPatch()
    try:
        mp.setenv("nnUNet_raw_data_base", str(tmp_path / "raw_base"))
        mp.setenv("nnUNet_preprocessed", str(tmp_path / "preprocessed"))
        raw = os.path.join(paths.nnUNet_raw_data, TASK)
        os.makedirs(os.path.join(raw, "imagesTr"))
        os.makedirs(os.path.join(raw, "labelsTr"))
        arrays = {}
        for ci, c in enumerate(CASES):
            ct, mr, seg = arrays[c] = _case_arrays(ci)
            _write_volume(os.path.join(raw, "imagesTr", c + "_0000.nii.gz"), ct, order=">" if ci else "<")
            _write_volume(os.path.join(raw, "imagesTr", c + "_0001.nii.gz"), mr)
            _write_volume(os.path.join(raw, "labelsTr", c + ".nii.gz"), seg)
        with open(os.path.join(raw, "dataset.json"), "w") as f:
            json.dump({"modality": {"0": "CT", "1": "MRI"}, "labels": {"0": "background", "1": "a", "2": "b"},
                       "training": [{"image": "./imagesTr/%s.nii.gz" % c, "label": "./labelsTr/%s.nii.gz" % c} for c in CASES]}, f)
        cropped = os.path.join(paths.nnUNet_cropped_data, TASK)
        main(["-t", TASK, "-tf", "1", "--native_nifti"])
        native = _cropped_folder(cropped)
        with open(os.path.join(cropped, "dataset_properties.pkl"), "rb") as f:
            native_dp = pickle.load(f)
        main(["-t", TASK, "-tf", "1", "--override"], reader=_ArrayReader())
        host = _cropped_folder(cropped)
        with open(os.path.join(cropped, "dataset_properties.pkl"), "rb") as f:
            host_dp = pickle.load(f)
    finally:
        mp.undo()
    for c in CASES:
        (n_npz, n_props), (h_npz, h_props) = native[c], host[c]
        assert list(n_npz) == list(h_npz) == ["data"]
        assert n_npz["data"].dtype == h_npz["data"].dtype == np.float32 and n_npz["data"].shape == h_npz["data"].shape
        assert n_npz["data"].tobytes() == h_npz["data"].tobytes()
        ct, mr, seg = arrays[c]
        assert n_npz["data"].shape[1:] != ct.shape and n_npz["data"].shape[0] == 3          # (it was cropped; 2 modalities + seg)
        assert list(n_props) == list(h_props)
        for k in n_props:
            if k == "list_of_data_files":
                assert [os.path.basename(f) for f in n_props[k]] == [c + "_0000.nii.gz", c + "_0001.nii.gz"]
                continue
            a, b = n_props[k], h_props[k]
            assert type(a) is type(b), k
            assert np.array_equal(np.asarray(a), np.asarray(b)), k
        assert list(n_props["original_spacing"]) == [F32(2.5), F32(0.8), F32(0.7)]
        assert n_props["itk_origin"] == (90.5, -126.0, -72.25) and list(n_props["original_size_of_raw_data"]) == list(ct.shape)
    assert _same(native_dp, host_dp) and list(native_dp['all_spacings'][0]) == [F32(2.5), F32(0.8), F32(0.7)]


# --------------------------------------------------------------------------------------------------------- end to end: evaluator
def _label_pair(seed):
    shape = (5, 33, 65)
    zz, yy, xx = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    gt = np.zeros(shape, np.uint8)
    gt[(yy - 14) ** 2 + (xx - 20) ** 2 < 90] = 1
    gt[(yy - 18) ** 2 + (xx - 45) ** 2 + 9 * (zz - 2) ** 2 < 60] = 2
    pred = np.roll(gt, (seed % 2, 1 + seed, -2), axis=(0, 1, 2))
    return pred, gt


def _strip(res):
    """a case's or the mean's metric numbers, the file names aside"""
    return {k: v for k, v in res.items() if k not in ("test", "reference")}


def test_evaluator_on_nifti_pairs_equals_the_npy_run(tmp_path):
    from e2enet_medical_amd import evaluator
    dirs = {k: str(tmp_path / k) for k in ("gt_nii", "pred_nii", "gt_npy", "pred_npy")}
    for d in dirs.values():
        os.makedirs(d)
    for i, (case, pred_name) in enumerate([("ev_a", "ev_a_0000"), ("ev_b", "ev_b")]):
        pred, gt = _label_pair(i)
        _write_volume(os.path.join(dirs["gt_nii"], case + ".nii.gz"), gt)
        _write_volume(os.path.join(dirs["pred_nii"], pred_name + ".nii.gz"), pred.astype(np.int16), order=">")
        np.save(os.path.join(dirs["gt_npy"], case + ".npy"), gt)
        np.save(os.path.join(dirs["pred_npy"], pred_name + ".npy"), pred)
    spacing = [F32(2.5), F32(0.8), F32(0.7)]
    native = evaluator.main(["-ref", dirs["gt_nii"], "-pred", dirs["pred_nii"], "-l", "1", "2", "--native_nifti", "--advanced"])
    host = evaluator.evaluate_folder(dirs["gt_npy"], dirs["pred_npy"], (1, 2), advanced=True, voxel_spacing=spacing)
    assert len(native["all"]) == len(host["all"]) == 2
    for n, h in zip(native["all"], host["all"]):
        assert n["voxel_spacing"] == spacing                      # from the header, array-axis order
        assert os.path.basename(n["test"])[:-7] == os.path.basename(h["test"])[:-4]
        assert os.path.basename(n["reference"])[:-7] == os.path.basename(h["reference"])[:-4]
        assert json.dumps(_strip(n), sort_keys=True) == json.dumps(_strip(h), sort_keys=True)
        assert 0.0 < n["1"]["Dice"] < 1.0 and np.isfinite(n["2"]["Hausdorff Distance 95"])
    assert json.dumps(native["mean"], sort_keys=True) == json.dumps(host["mean"], sort_keys=True)
    with open(os.path.join(dirs["pred_nii"], "summary.json")) as f:
        sn = json.load(f)["results"]
    with open(os.path.join(dirs["pred_npy"], "summary.json")) as f:
        sh = json.load(f)["results"]
    assert json.dumps(sn["mean"], sort_keys=True) == json.dumps(sh["mean"], sort_keys=True)
    assert [json.dumps(_strip(r), sort_keys=True) for r in sn["all"]] == [json.dumps(_strip(r), sort_keys=True) for r in sh["all"]]
    # a volume that is no label volume is refused by name
    bad, _ = _label_pair(0)
    _write_volume(os.path.join(dirs["pred_nii"], "ev_b.nii.gz"), bad.astype(np.float32) + 0.5)
    with pytest.raises(ValueError) as e:
        evaluator.main(["-ref", dirs["gt_nii"], "-pred", dirs["pred_nii"], "-l", "1", "2", "--native_nifti"])
    assert "ev_b.nii.gz" in str(e.value)


# ----------------------------------------------------------------------------------------------------------- end to end: predict
def test_predict_cases_writes_a_nifti_with_the_cases_geometry(tmp_path):
    """the tiny network of tests/golden/net_tiny.npz (closed-form parameters) in a trainer: predict_cases with writer=nifti.writer"""
    from e2enet_medical_amd.inference.predict import predict_cases
    from e2enet_medical_amd.training.network_training.nnUNetTrainer_simple import nnUNetTrainer_simple
    from tests.helpers import seeded_input
    from tests.test_gpu_net import TINY, load_closed_form
    plans = {'plans_per_stage': {0: {'batch_size': 2, 'patch_size': list(TINY["patch"]), 'num_pool_per_axis': [3, 5, 5],
                                     'pool_op_kernel_sizes': [list(p) for p in TINY["pools"]],
                                     'conv_kernel_sizes': [[3, 3, 3]] * 6, 'do_dummy_2D_data_aug': False}},
             'base_num_features': 32, 'num_modalities': TINY["cin"], 'num_classes': TINY["k"] - 1, 'all_classes': [1, 2],
             'transpose_forward': [0, 1, 2], 'transpose_backward': [0, 1, 2], 'conv_per_stage': 2}
    tr = nnUNetTrainer_simple(plans, 0, output_folder=None, Tconv='shiftConvPP', max_num_epochs=1, num_batches_per_epoch=1)
    tr.base_num_features_override = TINY["base"]
    tr.synthetic_data = True
    torch.manual_seed(0)
    net, _ = tr.initialize(True)
    load_closed_form(net)
    params = [{'epoch': 0, 'state_dict': {k: v.detach().cpu().clone() for k, v in net.state_dict().items()},
               'optimizer_state_dict': None, 'plot_stuff': ([], [], [], []), 'best_stuff': (None, None, None)}]
    vol = seeded_input((TINY["cin"], 16, 34, 37), seed=11).numpy()
    k = np.array([2., -1., 2.]) / 3.0                             # a rotation by 40 degrees about (2, -1, 2) / 3
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    D = np.eye(3) + np.sin(np.radians(40.)) * K + (1 - np.cos(np.radians(40.))) * (K @ K)
    props = {'size_after_cropping': np.array([16, 34, 37]), 'original_size_of_raw_data': np.array([18, 35, 41]),
             'crop_bbox': [[1, 17], [0, 34], [3, 40]], 'itk_spacing': (0.7, 0.8, 2.5), 'itk_origin': (-90.5, 126.0, -72.25),
             'itk_direction': tuple(float(v) for v in D.reshape(9))}
    handed = {}

    def writer(seg, path, properties):
        handed[path] = np.array(seg)
        nifti.writer(seg, path, properties)
    out = str(tmp_path / "case0.nii.gz")
    assert predict_cases(tr, params, [(out, (vol, props))], writer, do_tta=False) == [out]
    seg = handed[out]
    assert seg.dtype == np.uint8 and seg.shape == (18, 35, 41)
    h, vox = no.read_file(out)                                    # the test's own parser
    assert vox.dtype == np.uint8 and np.array_equal(vox, seg)
    raw = nifti.read_raw(out)
    assert raw.shape == seg.shape and np.array_equal(nifti.decode_u8(raw).cpu().numpy(), seg)
    assert np.array_equal(nifti.gt_reader(out), seg) and nifti.gt_reader(str(tmp_path / "missing.nii.gz")) is None
    np.testing.assert_allclose(raw.itk_spacing, props['itk_spacing'], rtol=1e-6)
    np.testing.assert_allclose(raw.itk_origin, props['itk_origin'], rtol=1e-6)
    np.testing.assert_allclose(raw.itk_direction, props['itk_direction'], rtol=0, atol=1e-6)
    # and the reader gives the file back as the fp32 case the preprocessing takes
    data, rprops = nifti.reader([out])
    assert data.is_cuda and data.dtype == torch.float32 and np.array_equal(data.cpu().numpy(), seg[None].astype(np.float32))
    assert list(rprops["original_size_of_raw_data"]) == [18, 35, 41] and rprops["itk_spacing"] == raw.itk_spacing
