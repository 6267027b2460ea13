"""Preprocessing a training folder on the device: the class-location kernels (csrc/class_select.hip) against numpy, bit for bit, and
GenericPreprocessor.run / run_preprocessing from a cropped folder to a stage folder the trainer trains on."""
import os
import pickle

import numpy as np
import pytest
import torch

from tests.test_dataset_cpu import _restatement

pytestmark = pytest.mark.gpu


def _check(seg, all_classes):
    """class_locations of a device volume == the reference's numpy on the downloaded volume, exactly; returns the dict"""
    from e2enet_medical_amd.preprocessing import class_locations
    dev = torch.from_numpy(np.ascontiguousarray(seg, dtype=np.float32)).cuda()
    got = class_locations(dev, all_classes)
    want = _restatement(dev.cpu().numpy(), all_classes)
    assert list(got.keys()) == list(want.keys())
    for c in all_classes:
        if len(want[c]) == 0:
            assert isinstance(got[c], list) and got[c] == []
        else:
            assert got[c].dtype == np.int64 and got[c].shape == want[c].shape
            assert np.array_equal(got[c], want[c]), "class %r" % (c,)
    return got


def test_small_volume_every_voxel_in_the_permuted_order():
    from e2enet_medical_amd.preprocessing import class_locations
    seg = np.random.RandomState(3).choice(np.array([-1.0, 0.0, 1.0, 2.0], dtype=np.float32), size=(5, 6, 7))
    got = _check(seg, [1, 2, 3])
    assert got[3] == []
    for c in (1, 2):
        assert len(got[c]) == int((seg == c).sum()) > 1
        assert not np.array_equal(got[c], np.argwhere(seg == c))                           # permuted, ...
        assert np.array_equal(got[c][np.lexsort(got[c].T[::-1])], np.argwhere(seg == c))     # ... and every voxel once
        assert (seg[tuple(got[c].T)] == c).all()                                           # -1 and 0 appear nowhere
    # a numpy volume is uploaded and gives the same
    again = class_locations(seg, [1, 2, 3])
    assert all(np.array_equal(again[c], got[c]) for c in (1, 2)) and again[3] == []
    assert class_locations(seg, []) == {}


def _boundary_indices(q):
    """first and last voxel of a wave, first and last voxel of a workgroup's chunk, the tail chunk"""
    return [0, 63, 64, q - 1, q, 2 * q - 1, 2 * q, 2 * q + 2]


@pytest.mark.parametrize("flat", [True, False], ids=["row", "odd_planes"])
def test_chunk_boundaries(flat):
    from e2enet_medical_amd._lib import lib
    q = lib().pp_select_chunk()
    n = 2 * q + 3
    if flat:
        shape = (1, 1, n)
    else:
        h, w = 11, 149                                          # odd; 5 * 11 * 149 = 2 * 4096 + 3
        shape = (-(-n // (h * w)), h, w)
    seg = np.zeros(shape, dtype=np.float32)
    seg.reshape(-1)[:] = np.where(np.arange(seg.size) % 3 == 0, -1.0, 0.0)
    idx = _boundary_indices(q)
    seg.reshape(-1)[idx] = 1.0
    got = _check(seg, [1])[1]
    want = np.stack(np.unravel_index(idx, shape), axis=1)
    assert np.array_equal(got[np.lexsort(got.T[::-1])], want)


def test_a_true_subset_with_the_same_bytes_on_every_run():
    seg = (np.random.RandomState(5).rand(48, 48, 48) < 0.5).astype(np.float32)
    n = int((seg == 1).sum())
    assert n > 10000
    a = _check(seg, [1])[1]
    b = _check(seg, [1])[1]
    assert a.shape == (10000, 3) and a.tobytes() == b.tobytes()


def test_the_one_percent_rule_and_a_scan_longer_than_one_step():
    """104^3 voxels are 275 chunks of 4096: the offset scan, which takes 256 chunks per step, runs two steps"""
    from e2enet_medical_amd._lib import lib
    seg = np.ones((104, 104, 104), dtype=np.float32)
    assert seg.size // lib().pp_select_chunk() > 256
    got = _check(seg, [1])[1]
    assert got.shape == (11249, 3)


def test_one_random_state_serves_the_classes_in_the_order_given():
    seg = np.random.RandomState(6).choice(np.array([0.0, 1.0, 2.0], dtype=np.float32), size=(20, 21, 23))
    swapped = _check(seg, [2, 1])
    ordered = _check(seg, [1, 2])
    assert list(swapped.keys()) == [2, 1]
    assert not np.array_equal(swapped[1], ordered[1])          # class 1 drawn after class 2 is another draw


def test_more_classes_than_one_launch_serves():
    """the host loops over groups of pp_select_max_classes classes; the random state runs through all of them"""
    from e2enet_medical_amd._lib import lib
    kmax = lib().pp_select_max_classes()
    seg = np.random.RandomState(8).randint(-1, kmax + 12, size=(9, 10, 11)).astype(np.float32)
    _check(seg, list(range(kmax + 9, 0, -1)) + [1])            # (a class listed twice is drawn twice, like the reference's loop)


def test_indices_behind_two_to_the_31():
    """2^31 + 2^16 voxels (8 GiB): voxels on both sides of 2^31 come back with their coordinates; the expected rows are closed forms"""
    from e2enet_medical_amd._lib import lib
    from e2enet_medical_amd.preprocessing import class_locations
    q = lib().pp_select_chunk()
    shape = (2, 32768, 32769)
    n = shape[0] * shape[1] * shape[2]
    assert n > 2 ** 31
    idx = np.array([0, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + q + 1, n - 1], dtype=np.int64)
    seg = torch.zeros(shape, dtype=torch.float32, device="cuda")
    seg.view(-1)[torch.from_numpy(idx).cuda()] = 1.0
    got = class_locations(seg, [2, 1])
    del seg
    order = np.random.RandomState(1234).choice(len(idx), len(idx), replace=False)
    assert got[2] == [] and np.array_equal(got[1], np.stack(np.unravel_index(idx[order], shape), axis=1))


# ---------------------------------------------------------------------------------------------------------------- a training folder
SPACINGS = [np.array([5.0, 2.0, 2.0]), np.array([2.5, 0.5, 0.5])]
ALL_CLASSES = [1, 2]
DATA_IDENTIFIER = "nnUNetData_plans_v2.1"
CASES = ("case_a", "case_b")


def _plans():
    from tests.test_gpu_preprocess import MASKS2, SCHEMES2
    from tests.test_gpu_trainer import PLANS
    stages = {i: dict(PLANS['plans_per_stage'][0], current_spacing=SPACINGS[i]) for i in range(2)}
    return dict(PLANS, plans_per_stage=stages, num_modalities=2, normalization_schemes=SCHEMES2, use_mask_for_norm=MASKS2,
                data_identifier=DATA_IDENTIFIER, all_classes=ALL_CLASSES)


def _write_cropped(folder):
    """two cropped cases as the reference's ImageCropper leaves them (<case>.npz with [modalities..., seg], <case>.pkl), the dataset
    properties and a ground-truth folder"""
    from e2enet_medical_amd.preprocessing import ImageCropper
    from tests.test_gpu_preprocess import _raw_case
    os.makedirs(os.path.join(folder, "gt_segmentations"))
    for ci, name in enumerate(CASES):
        x, props = _raw_case(50 + ci, shape=(12, 24, 26 + 2 * ci))
        zz, yy, xx = np.meshgrid(*[np.arange(s) for s in x.shape[1:]], indexing="ij")
        seg = ((((zz // 2 + yy // 4 + xx // 5 + ci) % 4) < 2).astype(np.float32) + ((zz + yy // 3 + xx // 3) % 5 == 0)).astype(np.float32)
        data, seg, props = ImageCropper.crop(x, props, np.minimum(seg, 2.0)[None])
        assert (seg == -1).any() and (seg == 1).any() and (seg == 2).any()
        np.savez_compressed(os.path.join(folder, name + ".npz"), data=np.vstack((data, seg)))
        with open(os.path.join(folder, name + ".pkl"), "wb") as f:
            pickle.dump(props, f)
        with open(os.path.join(folder, "gt_segmentations", name + ".nii.gz"), "wb") as f:
            f.write(b"gt of " + name.encode())
    with open(os.path.join(folder, "dataset_properties.pkl"), "wb") as f:
        pickle.dump({"all_classes": ALL_CLASSES}, f)


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    """(cropped folder, task folder preprocessed with one writer thread)"""
    from e2enet_medical_amd.preprocessing import run_preprocessing
    root = tmp_path_factory.mktemp("dataset")
    cropped, out = str(root / "cropped"), str(root / "Task997")
    _write_cropped(cropped)
    run_preprocessing(_plans(), cropped, out, 1)
    return cropped, out


def test_run_writes_the_reference_layout(folders):
    from e2enet_medical_amd.preprocessing import GenericPreprocessor
    from tests.test_gpu_preprocess import MASKS2, SCHEMES2
    cropped, out = folders
    assert sorted(os.listdir(os.path.join(out, "gt_segmentations"))) == [c + ".nii.gz" for c in CASES]
    pre = GenericPreprocessor(SCHEMES2, MASKS2, [0, 1, 2])
    for i, spacing in enumerate(SPACINGS):
        stage = os.path.join(out, "%s_stage%d" % (DATA_IDENTIFIER, i))
        assert sorted(os.listdir(stage)) == sorted(c + e for c in CASES for e in (".npz", ".pkl"))
        for c in CASES:
            npz = np.load(os.path.join(stage, c + ".npz"))
            assert npz.files == ["data"]
            all_data = npz["data"]
            with open(os.path.join(stage, c + ".pkl"), "rb") as f:
                props = pickle.load(f)
            data, seg, cprops = GenericPreprocessor.load_cropped(cropped, c)
            wd, ws, wprops = pre.resample_and_normalize(data, spacing, cprops, seg)
            assert all_data.dtype == np.float32 and all_data.tobytes() == np.vstack((wd, ws)).astype(np.float32).tobytes()
            assert tuple(props["size_after_resampling"]) == all_data.shape[1:] == tuple(wprops["size_after_resampling"])
            assert np.array_equal(props["spacing_after_resampling"], spacing) and props["crop_bbox"] == cprops["crop_bbox"]
            want = _restatement(all_data[-1], ALL_CLASSES)
            assert list(props["class_locations"].keys()) == ALL_CLASSES
            for k in ALL_CLASSES:
                assert len(want[k]) > 0 and props["class_locations"][k].dtype == np.int64
                assert np.array_equal(props["class_locations"][k], want[k])
    shapes = [np.load(os.path.join(out, "%s_stage%d" % (DATA_IDENTIFIER, i), "case_a.npz"))["data"].shape for i in range(2)]
    assert shapes[0][1:] != shapes[1][1:] and shapes[0][0] == shapes[1][0] == 3


def test_files_do_not_depend_on_the_thread_count_and_unpack_writes_npy(folders, tmp_path):
    from e2enet_medical_amd.preprocessing import GenericPreprocessor_linearResampling, run_preprocessing
    cropped, out = folders
    out4 = str(tmp_path / "Task997")
    run_preprocessing(_plans(), cropped, out4, 4, unpack_npy=True)
    for i in range(2):
        a, b = (os.path.join(o, "%s_stage%d" % (DATA_IDENTIFIER, i)) for o in (out, out4))
        assert sorted(os.listdir(b)) == sorted(c + e for c in CASES for e in (".npz", ".pkl", ".npy"))
        for c in CASES:
            for e in (".npz", ".pkl"):
                with open(os.path.join(a, c + e), "rb") as fa, open(os.path.join(b, c + e), "rb") as fb:
                    assert fa.read() == fb.read(), (i, c, e)
            npy = np.load(os.path.join(b, c + ".npy"), "r")
            assert npy.dtype == np.float32 and np.array_equal(npy, np.load(os.path.join(b, c + ".npz"))["data"])
    # the linear preprocessor inherits run: one stage, by name through the plans
    lin = str(tmp_path / "linear")
    plans = _plans()
    run_preprocessing(dict(plans, preprocessor_name="GenericPreprocessor_linearResampling", plans_per_stage={0: plans['plans_per_stage'][1]}),
                      cropped, lin, [3])
    stage = os.path.join(lin, DATA_IDENTIFIER + "_stage0")
    got = np.load(os.path.join(stage, "case_a.npz"))["data"]
    cubic = np.load(os.path.join(out, DATA_IDENTIFIER + "_stage1", "case_a.npz"))["data"]
    assert GenericPreprocessor_linearResampling.run is not None and got.shape == cubic.shape
    assert np.array_equal(got[-1], cubic[-1]) and not np.array_equal(got[0], cubic[0])


def test_trainer_trains_on_the_produced_stage_folder(folders, tmp_path):
    """load_dataset over the produced folder, DataLoader3D forced onto foreground for every sample, one training iteration"""
    from e2enet_medical_amd.training.network_training.nnUNetTrainer_simple import nnUNetTrainer_simple
    _, out = folders
    tr = nnUNetTrainer_simple(_plans(), "all", output_folder=str(tmp_path / "model"), dataset_directory=out, batch_dice=False, stage=1,
                              Tconv='shiftConvPP', max_num_epochs=1, num_batches_per_epoch=2)
    tr.base_num_features_override = 8
    tr.oversample_foreground_percent = 1.0
    torch.manual_seed(0)
    np.random.seed(0)
    tr.initialize(True)
    assert tr.folder_with_preprocessed_data == os.path.join(out, DATA_IDENTIFIER + "_stage1")
    assert sorted(tr.dataset.keys()) == list(CASES) and all('class_locations' in e['properties'] for e in tr.dataset.values())
    assert tr.dl_tr.oversample_foreground_percent == 1.0
    for _ in range(3):
        batch = tr.dl_tr.generate_train_batch()
        assert batch['data'].shape[:2] == (tr.batch_size, 2)
        for j in range(tr.batch_size):
            assert (batch['seg'][j] > 0).any(), "a forced-foreground patch without a foreground voxel"
    loss = float(tr.run_iteration(tr.tr_gen, True))
    assert np.isfinite(loss)
