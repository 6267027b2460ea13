"""The host half of the dataset fingerprint: the rank-and-interpolation rule of the seven intensity numbers against numpy, and the
host helpers around the cropped folder (file lists, the layout of dataset_properties.pkl, size reductions, the reader plumbing).
No GPU and no library."""
import json
import os
import pickle

import numpy as np
import pytest

PERCENTILES = (99.5, 0.5)


def half_ulp32(ref):
    """half the spacing of fp32 at |ref|, taken from the binade below when |ref| rounds up into the next one"""
    a = abs(float(ref))
    f = np.float32(a)
    if float(f) > a:
        f = np.nextafter(f, np.float32(0))
    return 0.5 * float(np.spacing(f))


def _same_special(got, ref):
    """a reference that is NaN or infinite must be met exactly"""
    return (np.isnan(got) and np.isnan(ref)) or float(got) == float(ref)


def check_seven(got, v):
    """the bars every implementation of _compute_stats is held to, for an fp32 sample ``v`` (any order) without a NaN:
    median: np.median(list(v)) bit for bit;  min, max: numpy's;  percentiles: within half an fp32 ulp plus 1e-12 relative of
    np.percentile(v.astype(np.float64), q);  mean and sd: no farther from the fp64 value than numpy's fp32 result over list(v) is,
    or within half an fp32 ulp of it."""
    v = np.asarray(v, dtype=np.float32)
    assert len(got) == 7 and all(type(g) is np.float32 for g in got), [type(g) for g in got]
    median, mean, sd, mn, mx, p995, p005 = got
    with np.errstate(all='ignore'):
        assert np.float32(median).tobytes() == np.float32(np.median(list(v))).tobytes(), (median, np.median(list(v)))
        assert mn == v.min() and mx == v.max()
        x = v.astype(np.float64)
        for g, q in zip((p995, p005), PERCENTILES):
            ref = np.percentile(x, q)
            if not np.isfinite(ref):
                assert _same_special(g, ref), (q, g, ref)
            else:
                assert abs(float(g) - ref) <= half_ulp32(ref) + 1e-12 * abs(ref), (q, g, ref)
        for g, ref, theirs in ((mean, x.mean(), np.mean(list(v))), (sd, x.std(), np.std(list(v)))):
            if not np.isfinite(ref):
                assert _same_special(g, ref), (g, ref)
            else:
                assert abs(float(g) - ref) <= max(abs(float(theirs) - ref), half_ulp32(ref)), (g, ref, theirs)


def sample(n, ties, seed):
    rng = np.random.RandomState(seed)
    if ties:
        return rng.randint(-3, 4, size=n).astype(np.float32) * np.float32(0.25)
    return (rng.randn(n) * 300.0 - 150.0).astype(np.float32)


def _host_rule(v):
    """drives the rank rule with order statistics taken from np.sort, and with nothing but the ranks it asked for"""
    from e2enet_medical_amd.experiment_planning.intensity_stats import requested_ranks, stats_from_order_statistics
    v = np.asarray(v, dtype=np.float32)
    s = np.sort(v)
    n = s.size
    ranks = requested_ranks(n)
    assert ranks == sorted(set(ranks)) and 1 <= len(ranks) <= 6 and ranks[0] >= 0 and ranks[-1] < n
    x = v.astype(np.float64)
    with np.errstate(all='ignore'):
        total = x.sum()
        sq_dev = ((x - total / n) ** 2).sum()
    return stats_from_order_statistics(n, int(np.isnan(v).sum()), s[0], s[-1], total, sq_dev, {r: s[r] for r in ranks})


@pytest.mark.parametrize("ties", [False, True], ids=["distinct", "ties"])
@pytest.mark.parametrize("n", [1, 2, 3, 200, 201, 202, 4567, 20000])
def test_rank_rule_against_numpy(n, ties):
    for seed in range(3):
        v = sample(n, ties, 100 * n + seed)
        check_seven(_host_rule(v), v)


def test_rank_rule_edge_cases():
    from e2enet_medical_amd.experiment_planning.intensity_stats import stats_from_order_statistics, stats_of_sorted
    empty = stats_from_order_statistics(0, 0, 0., 0., 0., 0., {})
    assert len(empty) == 7 and all(isinstance(e, float) and np.isnan(e) for e in empty)        # the reference's seven np.nan
    with_nan = _host_rule(np.array([1.0, np.nan, 3.0], dtype=np.float32))
    assert len(with_nan) == 7 and all(type(e) is np.float32 and np.isnan(e) for e in with_nan)
    zeros = np.array([0.0, -0.0, 0.0, -0.0], dtype=np.float32)
    got = _host_rule(zeros)
    check_seven(got, zeros)
    assert all(g == 0 for g in got)                            # -0.0 and 0.0 compare equal
    wide = np.array([-np.inf, -5.0, 0.0, 1.0, 2.0, np.inf], dtype=np.float32)
    check_seven(_host_rule(wide), wide)
    assert stats_of_sorted(np.sort(wide))[3] == -np.inf
    v = sample(777, False, 5)
    assert [a.tobytes() for a in stats_of_sorted(np.sort(v))] == [a.tobytes() for a in _host_rule(v)]


def test_rule_needs_neither_the_library_nor_torch_cuda():
    import subprocess
    import sys
    code = ("import e2enet_medical_amd.experiment_planning.intensity_stats as m; import e2enet_medical_amd._lib as l; "
            "assert l._lib is None and m.requested_ranks(1) == [0]")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, "-c", code], check=True, cwd=root)


# ------------------------------------------------------------------------------------------------------------ host helpers
DATASET_JSON = {"modality": {"0": "CT", "1": "MRI"}, "labels": {"0": "background", "1": "liver", "2": "tumour"},
                "training": [{"image": "./imagesTr/liver_7.nii.gz", "label": "./labelsTr/liver_7.nii.gz"},
                             {"image": "./imagesTr/liver_12.nii.gz", "label": "./labelsTr/liver_12.nii.gz"}]}


def test_create_lists_from_splitted_dataset(tmp_path):
    from e2enet_medical_amd.experiment_planning.utils import create_lists_from_splitted_dataset
    (tmp_path / "dataset.json").write_text(json.dumps(DATASET_JSON))
    lists, modalities = create_lists_from_splitted_dataset(str(tmp_path))
    base = str(tmp_path)
    assert lists == [[os.path.join(base, "imagesTr", "liver_7_0000.nii.gz"), os.path.join(base, "imagesTr", "liver_7_0001.nii.gz"),
                      os.path.join(base, "labelsTr", "liver_7.nii.gz")],
                     [os.path.join(base, "imagesTr", "liver_12_0000.nii.gz"), os.path.join(base, "imagesTr", "liver_12_0001.nii.gz"),
                      os.path.join(base, "labelsTr", "liver_12.nii.gz")]]
    assert modalities == {0: "CT", 1: "MRI"}
    from e2enet_medical_amd.preprocessing.cropping import get_case_identifier
    assert [get_case_identifier(c) for c in lists] == ["liver_7", "liver_12"]


def _cropped_folder(folder, with_intensity=None):
    """pickles and empty .npz names of two cropped cases, dataset.json"""
    os.makedirs(folder, exist_ok=True)
    with open(os.path.join(folder, "dataset.json"), "w") as f:
        json.dump(DATASET_JSON, f)
    props = {"case_b": {"size_after_cropping": (10, 20, 30), "original_size_of_raw_data": np.array([20, 20, 30]),
                        "original_spacing": np.array([2.5, 0.8, 0.8])},
             "case_a": {"size_after_cropping": (8, 16, 16), "original_size_of_raw_data": np.array([8, 16, 16]),
                        "original_spacing": np.array([5.0, 1.0, 1.0])}}
    for name, p in props.items():
        with open(os.path.join(folder, name + ".npz"), "wb") as f:
            f.write(b"")
        with open(os.path.join(folder, name + ".pkl"), "wb") as f:
            pickle.dump(p, f)
    with open(os.path.join(folder, "notes.txt"), "w") as f:
        f.write("not a case")
    if with_intensity is not None:
        with open(os.path.join(folder, "intensityproperties.pkl"), "wb") as f:
            pickle.dump(with_intensity, f)
    return props


def test_analyzer_host_methods_and_the_file_without_intensity_properties(tmp_path):
    from e2enet_medical_amd.experiment_planning import DatasetAnalyzer
    from e2enet_medical_amd.preprocessing.cropping import get_patient_identifiers_from_cropped_files
    folder = str(tmp_path / "cropped")
    props = _cropped_folder(folder)
    assert get_patient_identifiers_from_cropped_files(folder) == ["case_a", "case_b"]
    an = DatasetAnalyzer(folder, overwrite=True, num_processes=64)
    assert an.num_processes == 16 and an.patient_identifiers == ["case_a", "case_b"]
    assert an.get_classes() == DATASET_JSON["labels"] and an.get_modalities() == {0: "CT", 1: "MRI"}
    red = an.get_size_reduction_by_cropping()
    assert list(red.keys()) == ["case_a", "case_b"] and red["case_a"] == 1.0 and red["case_b"] == 0.5
    sizes, spacings = an.get_sizes_and_spacings_after_cropping()
    assert sizes == [(8, 16, 16), (10, 20, 30)] and np.array_equal(spacings, [props["case_a"]["original_spacing"],
                                                                                 props["case_b"]["original_spacing"]])
    got = an.analyze_dataset(collect_intensityproperties=False)
    with open(os.path.join(folder, "dataset_properties.pkl"), "rb") as f:
        saved = pickle.load(f)
    for d in (got, saved):
        assert set(d.keys()) == {'all_sizes', 'all_spacings', 'all_classes', 'modalities', 'intensityproperties', 'size_reductions'}
        assert d['all_classes'] == [1, 2] and d['modalities'] == {0: "CT", 1: "MRI"} and d['intensityproperties'] is None
        assert d['all_sizes'] == sizes and dict(d['size_reductions']) == dict(red)


def test_overwrite_false_reuses_the_intensity_properties_file(tmp_path):
    from e2enet_medical_amd.experiment_planning import DatasetAnalyzer
    folder = str(tmp_path / "cropped")
    kept = {0: {"mean": np.float32(4.0)}, 1: {"mean": np.float32(5.0)}}
    _cropped_folder(folder, with_intensity=kept)
    an = DatasetAnalyzer(folder, overwrite=False)
    assert an.collect_intensity_properties(2) == kept                      # no case is read: the .npz files are empty
    assert an.analyze_dataset(True)['intensityproperties'] == kept


def test_nesting_of_the_intensity_properties():
    from e2enet_medical_amd.experiment_planning.DatasetAnalyzer import dataset_properties_dict, intensity_properties_dict
    names = ['median', 'mean', 'sd', 'mn', 'mx', 'percentile_99_5', 'percentile_00_5']
    cases = ["a", "b"]
    g = [tuple(np.float32(10 * m + i) for i in range(7)) for m in range(2)]
    loc = [[tuple(np.float32(100 * m + 10 * c + i) for i in range(7)) for c in range(2)] for m in range(2)]
    ip = intensity_properties_dict(cases, g, loc)
    assert list(ip.keys()) == [0, 1]
    for m in range(2):
        assert list(ip[m].keys()) == ['local_props'] + names                              # the reference's order of insertion
        assert [ip[m][k] for k in names] == list(g[m])
        assert list(ip[m]['local_props'].keys()) == cases
        for c, case in enumerate(cases):
            assert list(ip[m]['local_props'][case].keys()) == names
            assert [ip[m]['local_props'][case][k] for k in names] == list(loc[m][c])
    d = dataset_properties_dict([(1, 2, 3)], [np.ones(3)], {"0": "bg", "2": "b", "1": "a"}, {0: "CT"}, ip, {"a": 0.5})
    assert list(d.keys()) == ['all_sizes', 'all_spacings', 'all_classes', 'modalities', 'intensityproperties', 'size_reductions']
    assert d['all_classes'] == [2, 1] and d['intensityproperties'] is ip


def test_samples_that_do_not_fit_the_device_raise_with_the_byte_count(monkeypatch):
    import torch
    from e2enet_medical_amd.experiment_planning import DatasetAnalyzer

    def no_room(parts):
        raise torch.cuda.OutOfMemoryError("out of memory")
    parts = [torch.zeros(5), torch.zeros(7)]
    assert DatasetAnalyzer._concatenate(parts).numel() == 12 and DatasetAnalyzer._concatenate(parts[:1]) is parts[0]
    monkeypatch.setattr(torch, "cat", no_room)
    with pytest.raises(MemoryError, match="48 bytes.*no host fallback"):
        DatasetAnalyzer._concatenate(parts)


def _memory_reader(store):
    def read(list_of_files):
        return (np.stack([store[f] for f in list_of_files]),
                {"original_spacing": np.array([2.0, 1.0, 1.0]), "itk_spacing": (1.0, 1.0, 2.0)})
    return read


def test_reader_plumbing_of_a_case_with_a_seg_file():
    from e2enet_medical_amd.preprocessing.cropping import load_case_with_reader, load_seg_with_reader
    rng = np.random.RandomState(0)
    store = {"a_0000": rng.rand(3, 4, 5), "a_0001": rng.rand(3, 4, 5), "a_seg": rng.randint(0, 3, (3, 4, 5)).astype(np.int16)}
    reader = _memory_reader(store)
    data, seg, props = load_case_with_reader(["a_0000", "a_0001"], "a_seg", reader, "test")
    assert data.dtype == np.float32 and data.shape == (2, 3, 4, 5) and np.array_equal(data[1], store["a_0001"].astype(np.float32))
    assert seg.dtype == np.float32 and seg.shape == (1, 3, 4, 5) and np.array_equal(seg[0], store["a_seg"])
    assert props["seg_file"] == "a_seg" and props["list_of_data_files"] == ["a_0000", "a_0001"]
    assert list(props["original_size_of_raw_data"]) == [3, 4, 5]
    assert np.array_equal(load_seg_with_reader("a_seg", reader), seg)
    data, seg, props = load_case_with_reader(["a_0000"], None, reader, "test")
    assert seg is None and props["seg_file"] is None


def test_cropping_a_folder_without_a_reader_refuses(tmp_path, monkeypatch):
    from e2enet_medical_amd.preprocessing import cropping
    monkeypatch.setattr(cropping, "default_reader", lambda: None)
    gt = tmp_path / "raw" / "a.nii.gz"
    gt.parent.mkdir()
    gt.write_bytes(b"gt")
    cropper = cropping.ImageCropper(2, str(tmp_path / "out"))
    with pytest.raises(NotImplementedError, match="no reader"):
        cropper.run_cropping([["a_0000.nii.gz", str(gt)]])
    with pytest.raises(NotImplementedError, match="no reader"):
        cropper.load_crop_save(["a_0000.nii.gz", str(gt)], "a")
    assert cropper.get_patient_identifiers_from_cropped_files() == []
    cropper.save_properties("a", {"x": 1})
    assert cropper.load_properties("a") == {"x": 1}


def test_command_line_arguments():
    from e2enet_medical_amd.crop_and_fingerprint import build_parser
    args = build_parser().parse_args(["-t", "Task555_X"])
    assert args.task_name == "Task555_X" and args.tf == 8 and args.override is False
    args = build_parser().parse_args(["-t", "5", "-tf", "3", "--override"])
    assert args.task_name == "5" and args.tf == 3 and args.override is True
