"""Cropping a raw folder and the dataset fingerprint on the device: the foreground stride sample (csrc/fingerprint.hip) against numpy,
bit for bit; the sample statistics against np.sort and the bars of tests/test_fingerprint_cpu.py; crop + analyze_dataset from a
synthetic raw folder to the reference's file layout; and run_preprocessing on what they wrote."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

from tests.test_fingerprint_cpu import check_seven

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------- foreground stride sample
def _check_sample(all_data, stride=10):
    """foreground_sample of a device case == numpy on the same array, exactly, and the same bytes on a second run"""
    from e2enet_medical_amd.experiment_planning.DatasetAnalyzer import foreground_sample
    all_data = np.ascontiguousarray(all_data, dtype=np.float32)
    dev = torch.from_numpy(all_data).cuda()
    got = foreground_sample(dev, stride)
    with np.errstate(invalid='ignore'):
        want = all_data[:-1].reshape(all_data.shape[0] - 1, -1)[:, all_data[-1].reshape(-1) > 0][:, ::stride]
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape, (tuple(got.shape), want.shape)
    got = got.cpu().numpy()
    assert got.tobytes() == want.tobytes()
    assert foreground_sample(dev, stride).cpu().numpy().tobytes() == got.tobytes()
    return got


def _case(shape, C, fg_index=None, seed=0):
    """[C + 1, *shape]: distinct data values per voxel and modality; seg from {-1, 0, 2, NaN}, or 2 at ``fg_index`` of the flat volume
    and -1, 0, NaN in turn elsewhere"""
    rng = np.random.RandomState(seed)
    n = int(np.prod(shape))
    data = (np.arange(C * n, dtype=np.float32) * 0.5 - 1000.0).reshape(C, n)
    if fg_index is None:
        seg = rng.choice(np.array([-1.0, 0.0, 2.0, np.nan], dtype=np.float32), size=n, p=[0.2, 0.4, 0.3, 0.1])
    else:
        seg = np.array([-1.0, 0.0, np.nan], dtype=np.float32)[np.arange(n) % 3]
        seg[np.asarray(fg_index, dtype=np.int64)] = 2.0
    return np.concatenate((data, seg[None])).reshape((C + 1,) + tuple(shape))


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("stride", [10, 7, 1, 100000])
def test_sample_random_volume(C, stride):
    """3 x 50 x 70 voxels are two chunks of 4096 and a tail; a stride above n_fg keeps the first voxel only"""
    got = _check_sample(_case((3, 50, 70), C, seed=C), stride)
    assert got.shape[1] == 1 if stride == 100000 else got.shape[1] > 100


def _chunk():
    from e2enet_medical_amd._lib import lib
    return lib().fingerprint_sample_chunk()


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("n_fg", [0, 1, 9, 10, 11, 30])
def test_sample_foreground_counts(C, n_fg):
    """the foreground spread over all three chunks of a row of 2 chunks + 5 voxels: n_fg below, at and above multiples of 10"""
    q = _chunk()
    n = 2 * q + 5
    idx = np.linspace(3, n - 1, n_fg).astype(np.int64) if n_fg else []
    assert len(set(idx)) == n_fg
    got = _check_sample(_case((1, 1, n), C, fg_index=idx))
    assert got.shape == (C, -(-n_fg // 10))


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("layout", ["first_of_chunk", "last_of_chunk"])
def test_sample_chunk_boundaries(C, layout):
    """foreground on both sides of every chunk boundary; a sampled rank (0, 10, 20) is the first voxel of the volume, the first voxel
    of a chunk and the last voxel of a chunk; chunks with foreground but without a sampled rank leave early"""
    q = _chunk()
    n = 2 * q + 5
    if layout == "first_of_chunk":       # rank 10 = voxel q, rank 20 = voxel 2q - 1
        idx = list(range(0, 63, 7)) + [q - 1, q] + list(range(q + 100, q + 109)) + [2 * q - 1, 2 * q, n - 1]
        sampled = [0, q, 2 * q - 1]
    else:                                # rank 10 = voxel q - 1, rank 20 = voxel 2q
        idx = list(range(5, 75, 7)) + [q - 1, q] + list(range(q + 64, q + 71)) + [2 * q - 1, 2 * q, n - 1]
        sampled = [5, q - 1, 2 * q]
    assert idx == sorted(idx) and [idx[r] for r in (0, 10, 20)] == sampled
    case = _case((1, 1, n), C, fg_index=idx)
    got = _check_sample(case)
    assert np.array_equal(got[0], case[0].reshape(-1)[sampled])
    # the same voxels in a volume with odd planes, and a numpy input
    from e2enet_medical_amd.experiment_planning.DatasetAnalyzer import foreground_sample
    h, w = 11, 149                                              # 5 * 11 * 149 = 2 * 4096 + 3
    idx = [i for i in idx if i < 5 * h * w]
    case = _case((5, h, w), C, fg_index=idx)
    assert np.array_equal(_check_sample(case), foreground_sample(case).cpu().numpy())


def test_sample_indices_behind_two_to_the_31():
    """2^31 + 2^16 voxels, one modality (17 GiB with the seg): foreground on both sides of 2^31; stride 2 keeps ranks 0, 2 and 4"""
    from e2enet_medical_amd.experiment_planning.DatasetAnalyzer import foreground_sample
    q = _chunk()
    n = 2 ** 31 + 2 ** 16
    idx = torch.tensor([0, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + q + 1, n - 1], dtype=torch.int64, device="cuda")
    case = torch.zeros((2, n), dtype=torch.float32, device="cuda")
    case[1][idx] = 3.0
    case[0][idx] = torch.tensor([11.0, 12.0, 13.0, 14.0, 15.0], device="cuda")
    got = foreground_sample(case, 2).cpu().numpy()
    del case
    assert got.shape == (1, 3) and got[0].tolist() == [11.0, 13.0, 15.0]


def test_sample_refuses_bad_arguments():
    from e2enet_medical_amd._lib import lib, E2EError
    L = lib()
    assert L.fingerprint_sample_ws_bytes(0) == 0 and L.fingerprint_sample_ws_bytes((2 ** 24) * L.fingerprint_sample_chunk()) == 0
    x = torch.zeros(2, 64, device="cuda")
    ws = torch.empty(L.fingerprint_sample_ws_bytes(64), dtype=torch.uint8, device="cuda")
    n_fg = torch.empty(1, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    L.fingerprint_sample_count(x[1].data_ptr(), 64, n_fg.data_ptr(), ws.data_ptr(), st)
    assert int(n_fg.item()) == 0
    with pytest.raises(E2EError, match="stride 0"):
        L.fingerprint_sample_gather(x.data_ptr(), x[1].data_ptr(), 1, 64, 0, x.data_ptr(), 1, ws.data_ptr(), st)
    ranks = np.full(9, 64, dtype=np.int64)
    with pytest.raises(E2EError, match="9 ranks"):
        L.fingerprint_stats(x.data_ptr(), 64, ranks.ctypes.data, 9, x.data_ptr(), ws.data_ptr(), st)
    with pytest.raises(E2EError, match="rank 64"):
        L.fingerprint_stats(x.data_ptr(), 64, ranks.ctypes.data, 1, x.data_ptr(), ws.data_ptr(), st)


# ----------------------------------------------------------------------------------------------------------------- statistics
LONG = 1024 * 256 + 4099             # more than the reduction's 1024 workgroups of 256 threads take in one step


def _bits(words):
    return np.asarray(words, dtype=np.uint32).view(np.float32)


def _mixed(n, with_inf):
    """thirds: values that differ only in their lowest byte; the same with the sign flipped (they differ from the first third in the
    highest byte only); normal draws.  Then +-0 and, with_inf, +-inf"""
    rng = np.random.RandomState(n % 1000)
    low = _bits(0x42F6E900 + rng.randint(0, 256, size=n // 3))
    neg = _bits(0xC2F6E900 + rng.randint(0, 256, size=n // 3))
    v = np.concatenate((low, neg, (rng.randn(n - 2 * (n // 3)) * 40.0).astype(np.float32)))
    v[:4] = [0.0, -0.0, -0.0, 0.0]
    v[4] = _bits([0x42F6E9AB])[0]
    v[5] = _bits([0xC2F6E9AB])[0]                                # differs from v[4] in the highest byte only
    if with_inf:
        v[6:10] = [np.inf, -np.inf, np.inf, -np.inf]
    rng.shuffle(v)
    return v


def _check_stats(v):
    """_compute_stats of a device array within the CPU test's bars; the order statistics it is built on equal np.sort's; the same
    bytes on a second run"""
    from e2enet_medical_amd.experiment_planning import DatasetAnalyzer
    from e2enet_medical_amd.experiment_planning.DatasetAnalyzer import order_statistics
    from e2enet_medical_amd.experiment_planning.intensity_stats import requested_ranks
    v = np.ascontiguousarray(v, dtype=np.float32)
    dev = torch.from_numpy(v).cuda()
    got = DatasetAnalyzer._compute_stats(dev)
    check_seven(got, v)
    ranks = requested_ranks(v.size)
    first = order_statistics(dev, ranks)
    assert first[0] == 0 and np.array_equal(np.array(first[5]), np.sort(v)[ranks])
    assert first[1] == v.min() and first[2] == v.max()
    again = order_statistics(dev, ranks)
    assert np.array(first[:5]).tobytes() == np.array(again[:5]).tobytes() and np.array(first[5]).tobytes() == np.array(again[5]).tobytes()
    return got


@pytest.mark.parametrize("with_inf", [False, True], ids=["finite", "inf"])
def test_stats_long_mixed_array(with_inf):
    got = _check_stats(_mixed(LONG, with_inf))
    assert np.isfinite(got[1]) != with_inf                       # +inf and -inf together: numpy's mean is NaN, and so is this one


@pytest.mark.parametrize("n", [1, 2, 3, 200, 201, 4097])
def test_stats_small_odd_and_even_lengths(n):
    _check_stats(_mixed(max(n, 12), False)[:n])
    # a list and a numpy array are uploaded and give the same
    from e2enet_medical_amd.experiment_planning import DatasetAnalyzer
    v = _mixed(max(n, 12), False)[:n]
    assert [g.tobytes() for g in DatasetAnalyzer._compute_stats(list(v))] == [g.tobytes() for g in DatasetAnalyzer._compute_stats(v)]


def test_stats_all_equal_empty_and_nan():
    from e2enet_medical_amd.experiment_planning import DatasetAnalyzer
    from e2enet_medical_amd.experiment_planning.DatasetAnalyzer import order_statistics
    got = _check_stats(np.full(1000, 3.25, dtype=np.float32))
    assert [float(g) for g in got] == [3.25, 3.25, 0.0, 3.25, 3.25, 3.25, 3.25]
    for empty in ([], np.zeros(0, dtype=np.float32), torch.zeros(0, device="cuda")):
        out = DatasetAnalyzer._compute_stats(empty)
        assert len(out) == 7 and all(isinstance(e, float) and np.isnan(e) for e in out)
    v = _mixed(LONG, False)
    v[LONG // 2 + 1] = np.nan
    dev = torch.from_numpy(v).cuda()
    out = DatasetAnalyzer._compute_stats(dev)
    assert len(out) == 7 and all(type(e) is np.float32 and np.isnan(e) for e in out)
    num_nan, mn, mx, _, _, order = order_statistics(dev, [0, LONG - 1])
    finite = v[~np.isnan(v)]
    assert num_nan == 1 and mn == finite.min() and mx == finite.max() and order[0] == finite.min() and np.isnan(order[1])


def test_stats_eight_ranks_at_once_with_duplicates():
    from e2enet_medical_amd.experiment_planning.DatasetAnalyzer import order_statistics
    v = _mixed(LONG, True)
    dev = torch.from_numpy(v).cuda()
    s = np.sort(v)
    for ranks in ([0, 0, LONG - 1, LONG // 2, LONG // 2, 5, LONG - 1, 17], [LONG // 3] * 8, list(range(8)),
                  [int(r) for r in np.linspace(0, LONG - 1, 8)]):
        got = order_statistics(dev, ranks)[5]
        assert len(got) == 8 and np.array_equal(np.array(got), s[ranks]), ranks


# ----------------------------------------------------------------------------------------------------------------- end to end
TASK = "Task996_Fingerprint"
CASE_NAMES = ("fp_b", "fp_a", "fp_c")                            # dataset.json lists them unsorted
SPACING = np.array([2.0, 1.0, 1.0])


def _raw_arrays(ci):
    """two modalities and a label map of 24 x 40 x (40 + 2 ci): a body with a notch inside a zero margin, labels 0, 1, 2 in the body"""
    shape = (24, 40, 40 + 2 * ci)
    rng = np.random.RandomState(40 + ci)
    body = np.zeros(shape, dtype=bool)
    body[2 + ci:21, 4:35 - ci, 3:38] = True
    body[:8, :12] = False                                        # a notch: zero voxels inside the bounding box, off the mask
    ct = (rng.randn(*shape) * 120.0 + 40.0).astype(np.float32) * body
    mr = (rng.rand(*shape).astype(np.float32) * 900.0 + 1.0) * body
    zz, yy, xx = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    seg = (((zz // 3 + yy // 5 + xx // 4 + ci) % 3) * body).astype(np.float32)
    ct = ct + 300.0 * (seg == 2)
    return np.stack((ct, mr)), seg


class _Reader(object):
    """serves the in-memory arrays by file name, a fresh properties dict per call; counts its calls"""

    def __init__(self, store):
        self.store, self.calls = store, 0

    def __call__(self, list_of_files):
        self.calls += 1
        data = np.stack([self.store[os.path.basename(f)] for f in list_of_files])
        return data, {"original_spacing": SPACING.copy(), "itk_spacing": (1.0, 1.0, 2.0), "itk_origin": (0.0, 0.0, 0.0)}


def _files_bytes(folder, names):
    out = {}
    for name in names:
        with open(os.path.join(folder, name), "rb") as f:
            out[name] = f.read()
    return out


@pytest.fixture(scope="module")
def task(tmp_path_factory):
    """a raw task folder, cropped with one writer thread and fingerprinted: dict(raw, cropped, preprocessed, reader, lists, cases)"""
    from e2enet_medical_amd import paths
    from e2enet_medical_amd.experiment_planning import analyze_dataset, create_lists_from_splitted_dataset, crop
    root = tmp_path_factory.mktemp("fingerprint")
    mp = pytest.MonkeyPatch()
    mp.setenv("nnUNet_raw_data_base", str(root / "raw_base"))
    mp.setenv("nnUNet_preprocessed", str(root / "preprocessed"))
    raw = os.path.join(paths.nnUNet_raw_data, TASK)
    os.makedirs(os.path.join(raw, "labelsTr"))
    store, cases = {}, {}
    for ci, name in enumerate(CASE_NAMES):
        data, seg = _raw_arrays(ci)
        cases[name] = (data, seg)
        store[name + "_0000.nii.gz"], store[name + "_0001.nii.gz"], store[name + ".nii.gz"] = data[0], data[1], seg
        with open(os.path.join(raw, "labelsTr", name + ".nii.gz"), "wb") as f:
            f.write(b"gt of " + name.encode())
    with open(os.path.join(raw, "dataset.json"), "w") as f:
        json.dump({"modality": {"0": "CT", "1": "MRI"}, "labels": {"0": "background", "1": "a", "2": "b"},
                   "training": [{"image": "./imagesTr/%s.nii.gz" % c, "label": "./labelsTr/%s.nii.gz" % c} for c in CASE_NAMES]}, f)
    reader = _Reader(store)
    crop(TASK, False, 1, reader=reader)
    crop_calls = reader.calls
    analyze_dataset(TASK, True, True, 4)
    lists, _ = create_lists_from_splitted_dataset(raw)
    yield dict(raw=raw, cropped=os.path.join(paths.nnUNet_cropped_data, TASK), preprocessed=os.path.join(paths.preprocessing_output_dir, TASK),
               reader=reader, crop_calls=crop_calls, lists=lists, cases=cases)
    mp.undo()


def test_crop_writes_the_reference_layout(task):
    from e2enet_medical_amd.preprocessing import ImageCropper
    cropped = task["cropped"]
    names = sorted(CASE_NAMES)
    want_files = sorted([c + e for c in names for e in (".npz", ".pkl")] +
                        ["dataset.json", "gt_segmentations", "dataset_properties.pkl", "intensityproperties.pkl"])
    assert sorted(os.listdir(cropped)) == want_files
    assert sorted(os.listdir(os.path.join(cropped, "gt_segmentations"))) == [c + ".nii.gz" for c in names]
    assert _files_bytes(cropped, ["dataset.json"]) == _files_bytes(task["raw"], ["dataset.json"])
    assert task["crop_calls"] == 2 * len(names)                  # per case: the modalities in one call, the seg in another
    for c in names:
        npz = np.load(os.path.join(cropped, c + ".npz"))
        assert npz.files == ["data"]
        all_data = npz["data"]
        with open(os.path.join(cropped, c + ".pkl"), "rb") as f:
            props = pickle.load(f)
        data, seg = task["cases"][c]
        wd, ws, wprops = ImageCropper.crop(data.copy(), {"original_spacing": SPACING.copy()}, seg[None].copy())
        assert all_data.dtype == np.float32 and all_data.tobytes() == np.vstack((wd, ws)).astype(np.float32).tobytes()
        assert all_data.shape[1:] != data.shape[1:] and (all_data[-1] == -1).any()
        assert props["crop_bbox"] == wprops["crop_bbox"] and np.array_equal(props["classes"], wprops["classes"])
        assert tuple(props["size_after_cropping"]) == tuple(wprops["size_after_cropping"]) == all_data.shape[1:]
        assert list(props["original_size_of_raw_data"]) == list(data.shape[1:]) and np.array_equal(props["original_spacing"], SPACING)
        assert props["seg_file"] == os.path.join(task["raw"], "labelsTr", c + ".nii.gz")
        assert [os.path.basename(f) for f in props["list_of_data_files"]] == [c + "_0000.nii.gz", c + "_0001.nii.gz"]


def test_fingerprint_matches_a_numpy_restatement(task):
    from e2enet_medical_amd.experiment_planning import DatasetAnalyzer
    cropped = task["cropped"]
    names = sorted(CASE_NAMES)
    with open(os.path.join(cropped, "dataset_properties.pkl"), "rb") as f:
        dp = pickle.load(f)
    with open(os.path.join(cropped, "intensityproperties.pkl"), "rb") as f:
        ip_file = pickle.load(f)
    assert list(dp.keys()) == ['all_sizes', 'all_spacings', 'all_classes', 'modalities', 'intensityproperties', 'size_reductions']
    arrays = {c: np.load(os.path.join(cropped, c + ".npz"))["data"] for c in names}
    assert dp['all_sizes'] == [arrays[c].shape[1:] for c in names]
    assert len(dp['all_spacings']) == 3 and all(np.array_equal(s, SPACING) for s in dp['all_spacings'])
    assert dp['all_classes'] == [1, 2] and dp['modalities'] == {0: "CT", 1: "MRI"}
    assert list(dp['size_reductions'].keys()) == names
    for c in names:
        assert dp['size_reductions'][c] == np.prod(arrays[c].shape[1:]) / np.prod(task["cases"][c][0].shape[1:]) < 1
    ip = dp['intensityproperties']
    assert list(ip.keys()) == [0, 1]
    stat_names = ['median', 'mean', 'sd', 'mn', 'mx', 'percentile_99_5', 'percentile_00_5']
    an = DatasetAnalyzer(cropped, overwrite=False)
    for m in range(2):
        assert list(ip[m].keys()) == ['local_props'] + stat_names and list(ip[m]['local_props'].keys()) == names
        samples = [arrays[c][m][arrays[c][-1] > 0][::10] for c in names]
        assert all(len(s) > 100 for s in samples)
        for c, s in zip(names, samples):
            assert list(ip[m]['local_props'][c].keys()) == stat_names
            check_seven(tuple(ip[m]['local_props'][c][k] for k in stat_names), s)
            got = an._get_voxels_in_foreground(c, m)
            assert isinstance(got, np.ndarray) and got.tobytes() == s.tobytes()
        check_seven(tuple(ip[m][k] for k in stat_names), np.concatenate(samples))
        for k in stat_names:
            assert ip_file[m][k].tobytes() == ip[m][k].tobytes()
    # overwrite=False reuses the file: nothing is computed again
    assert pickle.dumps(an.collect_intensity_properties(2)) == pickle.dumps(ip_file)


def test_files_do_not_depend_on_the_thread_count_and_existing_cases_are_skipped(task, tmp_path):
    from e2enet_medical_amd.preprocessing import ImageCropper
    names = [c + e for c in sorted(CASE_NAMES) for e in (".npz", ".pkl")]
    out4 = str(tmp_path / "cropped4")
    ImageCropper(4, out4).run_cropping(task["lists"], reader=task["reader"])
    assert _files_bytes(out4, names) == _files_bytes(task["cropped"], names)
    assert sorted(os.listdir(os.path.join(out4, "gt_segmentations"))) == [c + ".nii.gz" for c in sorted(CASE_NAMES)]
    # overwrite_existing=False: no case is read, no file is touched; one missing file brings that case back
    stamps = {n: os.stat(os.path.join(out4, n)).st_mtime_ns for n in names}
    calls = task["reader"].calls
    cropper = ImageCropper(2, out4)
    cropper.run_cropping(task["lists"], overwrite_existing=False, reader=task["reader"])
    cropper.load_crop_save(task["lists"][0], CASE_NAMES[0], overwrite_existing=False, reader=task["reader"])
    assert task["reader"].calls == calls and {n: os.stat(os.path.join(out4, n)).st_mtime_ns for n in names} == stamps
    os.remove(os.path.join(out4, "fp_a.pkl"))
    cropper.run_cropping(task["lists"], overwrite_existing=False, reader=task["reader"])
    assert task["reader"].calls == calls + 2 and _files_bytes(out4, names) == _files_bytes(task["cropped"], names)
    assert cropper.get_patient_identifiers_from_cropped_files() == sorted(CASE_NAMES)
    assert cropper.load_properties("fp_a")["crop_bbox"] == ImageCropper(1, task["cropped"]).load_properties("fp_a")["crop_bbox"]


def test_command_line_copies_the_fingerprint_to_the_preprocessed_folder(task):
    from e2enet_medical_amd.crop_and_fingerprint import main
    calls = task["reader"].calls
    with open(os.path.join(task["cropped"], "dataset_properties.pkl"), "rb") as f:
        before = pickle.load(f)
    stamp = os.stat(os.path.join(task["cropped"], "intensityproperties.pkl")).st_mtime_ns
    main(["-t", TASK, "-tf", "2"], reader=task["reader"])
    assert task["reader"].calls == calls                          # every case is there already: nothing is cropped again ...
    assert os.stat(os.path.join(task["cropped"], "intensityproperties.pkl")).st_mtime_ns == stamp      # ... or analysed again
    assert sorted(os.listdir(task["preprocessed"])) == ["dataset.json", "dataset_properties.pkl"]
    assert _files_bytes(task["preprocessed"], ["dataset_properties.pkl", "dataset.json"]) == \
        _files_bytes(task["cropped"], ["dataset_properties.pkl", "dataset.json"])
    with open(os.path.join(task["preprocessed"], "dataset_properties.pkl"), "rb") as f:
        after = pickle.load(f)
    assert after['all_classes'] == before['all_classes'] == [1, 2] and after['all_sizes'] == before['all_sizes']
    for m in range(2):
        for k in ('median', 'mean', 'sd', 'mn', 'mx', 'percentile_99_5', 'percentile_00_5'):
            assert after['intensityproperties'][m][k].tobytes() == before['intensityproperties'][m][k].tobytes()


def test_run_preprocessing_takes_the_cropped_folder_and_its_intensity_properties(task, tmp_path):
    """the chain: a hand-written CT plans dict around the produced dataset_properties; the stage files equal resample_and_normalize
    fed the same numbers"""
    from e2enet_medical_amd.preprocessing import GenericPreprocessor, run_preprocessing
    with open(os.path.join(task["cropped"], "dataset_properties.pkl"), "rb") as f:
        dp = pickle.load(f)
    target = np.array([2.0, 1.25, 1.25])
    schemes, masks = {0: "CT", 1: "nonCT"}, {0: False, 1: True}
    plans = {'plans_per_stage': {0: {'patch_size': [16, 32, 32], 'current_spacing': target}}, 'normalization_schemes': schemes,
             'use_mask_for_norm': masks, 'transpose_forward': [0, 1, 2], 'data_identifier': "nnUNetData_plans_v2.1",
             'dataset_properties': dp}
    out = str(tmp_path / TASK)
    run_preprocessing(plans, task["cropped"], out, 2)
    stage = os.path.join(out, "nnUNetData_plans_v2.1_stage0")
    names = sorted(CASE_NAMES)
    assert sorted(os.listdir(stage)) == sorted(c + e for c in names for e in (".npz", ".pkl"))
    assert sorted(os.listdir(os.path.join(out, "gt_segmentations"))) == [c + ".nii.gz" for c in names]
    pre = GenericPreprocessor(schemes, masks, [0, 1, 2], dp['intensityproperties'])
    ip = dp['intensityproperties'][0]
    for c in names:
        all_data = np.load(os.path.join(stage, c + ".npz"))["data"]
        with open(os.path.join(stage, c + ".pkl"), "rb") as f:
            props = pickle.load(f)
        data, seg, cprops = GenericPreprocessor.load_cropped(task["cropped"], c)
        wd, ws, _ = pre.resample_and_normalize(data, target, cprops, seg)
        assert all_data.tobytes() == np.vstack((wd, ws)).astype(np.float32).tobytes() and all_data.shape[1:] != data.shape[1:]
        assert list(props['class_locations'].keys()) == [1, 2] and all(len(props['class_locations'][k]) for k in (1, 2))
        # the CT channel was clipped to the fingerprint's percentiles and normalised by its mean and sd
        lo, hi = ((np.float64(ip[k]) - np.float64(ip['mean'])) / np.float64(ip['sd']) for k in ('percentile_00_5', 'percentile_99_5'))
        assert all_data[0].min() >= lo - 1e-5 and all_data[0].max() <= hi + 1e-5
