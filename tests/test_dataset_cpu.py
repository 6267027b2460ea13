"""The host half of preprocessing a training folder: how many class voxels are kept, which ranks are drawn, and what
run_preprocessing refuses.  No GPU and no library."""
import os

import numpy as np
import pytest


@pytest.mark.parametrize("n,want", [(0, 0), (1, 1), (9999, 9999), (10000, 10000), (10001, 10000), (1000000, 10000), (1000001, 10001),
                                    (1000100, 10001)])
def test_target_num_samples(n, want):
    from e2enet_medical_amd.preprocessing.class_sampling import target_num_samples
    assert target_num_samples(n) == want


def _restatement(seg, all_classes):
    """reference preprocessing.py:343-361 in plain numpy"""
    rndst = np.random.RandomState(1234)
    class_locs = {}
    for c in all_classes:
        all_locs = np.argwhere(seg == c)
        if len(all_locs) == 0:
            class_locs[c] = []
            continue
        target_num_samples = min(10000, len(all_locs))
        target_num_samples = max(target_num_samples, int(np.ceil(len(all_locs) * 0.01)))
        class_locs[c] = all_locs[rndst.choice(len(all_locs), target_num_samples, replace=False)]
    return class_locs


def _volume():
    return np.random.RandomState(7).choice(np.array([-1.0, 0.0, 1.0, 3.0], dtype=np.float32), size=(20, 22, 24), p=[0.2, 0.3, 0.3, 0.2])


@pytest.mark.parametrize("all_classes", [[1, 2, 3], [3, 2, 1]], ids=["ascending", "descending"])
def test_rank_draw_against_numpy(all_classes):
    from e2enet_medical_amd.preprocessing.class_sampling import draw_class_ranks, sort_ranks
    seg = _volume()
    assert (seg == 2).sum() == 0 and (seg == 1).sum() > 0 and (seg == 3).sum() > 0
    want = _restatement(seg, all_classes)
    ranks = draw_class_ranks(all_classes, [int((seg == c).sum()) for c in all_classes])
    assert list(ranks.keys()) == all_classes                   # the order given, not sorted
    assert isinstance(ranks[2], list) and ranks[2] == []
    for c in (1, 3):
        assert ranks[c].dtype == np.int64
        assert np.array_equal(np.argwhere(seg == c)[ranks[c]], want[c])
        s, slots = sort_ranks(ranks[c])
        assert (np.diff(s) > 0).all() and np.array_equal(ranks[c][slots], s)


def test_absent_class_consumes_no_random_numbers():
    from e2enet_medical_amd.preprocessing.class_sampling import draw_class_ranks
    seg = _volume()
    n1, n3 = int((seg == 1).sum()), int((seg == 3).sum())
    with_absent = draw_class_ranks([1, 2, 3], [n1, 0, n3])
    without = draw_class_ranks([1, 3], [n1, n3])
    assert np.array_equal(with_absent[3], without[3]) and np.array_equal(with_absent[1], without[1])
    # and the state is shared: class 3 after class 1 is not class 3 alone
    assert not np.array_equal(draw_class_ranks([3], [n3])[3], without[3])


def test_helper_needs_neither_the_library_nor_torch_cuda():
    import subprocess
    import sys
    code = ("import sys; import e2enet_medical_amd.preprocessing.class_sampling as m; import e2enet_medical_amd._lib as l; "
            "assert l._lib is None and m.target_num_samples(5) == 5")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, "-c", code], check=True, cwd=root)


PLANS = {'plans_per_stage': {0: {'patch_size': [16, 32, 32], 'current_spacing': np.array([2.5, 0.5, 0.5])}},
         'normalization_schemes': {0: "nonCT"}, 'use_mask_for_norm': {0: False}, 'transpose_forward': [0, 1, 2],
         'data_identifier': "nnUNetData_plans_v2.1"}


@pytest.mark.parametrize("change", [dict(preprocessor_name="PreprocessorFor2D"), dict(preprocessor_name="Preprocessor3DDifferentResampling"),
                                    dict(plans_per_stage={0: {'patch_size': [64, 64], 'current_spacing': np.array([1.0, 0.5, 0.5])}})],
                         ids=["2d_class", "custom_class", "2d_plans"])
def test_run_preprocessing_refuses_before_touching_a_file(tmp_path, change):
    from e2enet_medical_amd.preprocessing import run_preprocessing
    cropped, out = tmp_path / "cropped", tmp_path / "out"
    (cropped / "gt_segmentations").mkdir(parents=True)
    (cropped / "gt_segmentations" / "a.nii.gz").write_bytes(b"x")
    with pytest.raises(NotImplementedError, match="GenericPreprocessor_linearResampling on 3-D plans"):
        run_preprocessing(dict(PLANS, **change), str(cropped), str(out), 2)
    assert not out.exists()


def test_save_npz_is_savez_compressed_with_reproducible_bytes(tmp_path):
    from e2enet_medical_amd.preprocessing.preprocessing import save_npz
    a = np.random.RandomState(0).rand(3, 4, 5, 6).astype(np.float32)
    save_npz(str(tmp_path / "a.npz"), a)
    save_npz(str(tmp_path / "b.npz"), a.copy())
    got = np.load(str(tmp_path / "a.npz"))
    assert got.files == ["data"] and got["data"].dtype == np.float32 and np.array_equal(got["data"], a)
    assert (tmp_path / "a.npz").read_bytes() == (tmp_path / "b.npz").read_bytes()
