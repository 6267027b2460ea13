"""The experiment planner against the reference's recorded plans (tests/golden/planner.json, tools/make_golden_planner.py), the
refusals of the ``nnUNet_plan_and_preprocess`` command, and the host-only checks of ``sanity_checks``.  No GPU."""
import contextlib
import io
import json
import os
import pickle
from collections import OrderedDict

import numpy as np
import pytest

from tests import nifti_oracle as no
from tests import planner_golden as pg

GOLDEN = pg.load()
RUNS = GOLDEN["runs"]


def _planner_class(name):
    from e2enet_medical_amd.experiment_planning.nnUNet_plan_and_preprocess import PLANNERS_3D
    return PLANNERS_3D[name]


def _cropped_folder(root, dataset):
    """a cropped folder as the planner needs it: the fingerprint, empty <case>.npz names, minimal <case>.pkl files"""
    cropped, out = os.path.join(root, "cropped"), os.path.join(root, "preprocessed")
    os.makedirs(cropped)
    os.makedirs(out)
    with open(os.path.join(cropped, "dataset_properties.pkl"), "wb") as f:
        pickle.dump(pg.decode(dataset["fingerprint"]), f)
    for c in dataset["cases"]:
        open(os.path.join(cropped, c + ".npz"), "wb").close()
        with open(os.path.join(cropped, c + ".pkl"), "wb") as f:
            pickle.dump(OrderedDict(case=c), f)
    return cropped, out


def _plan(root, run):
    dataset = GOLDEN["datasets"][run["dataset"]]
    cropped, out = _cropped_folder(root, dataset)
    planner = _planner_class(run["planner"])(cropped, out)
    with contextlib.redirect_stdout(io.StringIO()):
        planner.plan_experiment()
    return planner, dataset, cropped


def test_the_golden_covers_every_branch_of_the_planning():
    facts = [r["facts"] for r in RUNS]
    some = lambda **want: any(all(f[k] == v for k, v in want.items()) for f in facts)
    assert some(stages=1) and some(stages=2) and some(stages=1, lowres_walk=True)
    assert some(aniso=True, aniso_clamped=False) and some(aniso=True, aniso_clamped=True) and some(transposed=True)
    assert some(vram_loop_in_fullres=True) and any(not f["vram_loop_in_fullres"] and f["batch_size"] > 2 for f in facts)
    assert some(cap_binds=True) and some(dummy_2D=True) and some(dummy_2D=False)
    assert sum(f["planner"] == "ExperimentPlanner" for f in facts) >= 2


@pytest.mark.parametrize("run", RUNS, ids=["%s-%s" % (r["dataset"], r["planner"]) for r in RUNS])
def test_plans_equal_the_references(tmp_path, run):
    planner, dataset, cropped = _plan(str(tmp_path), run)
    assert os.path.basename(planner.plans_fname) == run["plans_file"] and os.path.isfile(planner.plans_fname)
    with open(planner.plans_fname, "rb") as f:
        written = pickle.load(f)
    want = pg.decode(run["plans"], str(tmp_path))
    fingerprint = pg.decode(dataset["fingerprint"])
    # the golden stores the fingerprint once; the plans repeat it in three entries
    for key, part in (('dataset_properties', fingerprint), ('original_spacings', fingerprint['all_spacings']),
                      ('original_sizes', fingerprint['all_sizes'])):
        assert pg.difference(written[key], part, key) is None
    order = list(written)
    got = {k: v for k, v in written.items() if k not in ('dataset_properties', 'original_spacings', 'original_sizes')}
    assert pg.difference(got, want) is None, pg.difference(got, want)
    assert order == ['num_stages', 'num_modalities', 'modalities', 'normalization_schemes', 'dataset_properties', 'list_of_npz_files',
                     'original_spacings', 'original_sizes', 'preprocessed_data_folder', 'num_classes', 'all_classes',
                     'base_num_features', 'use_mask_for_norm', 'keep_only_largest_region', 'min_region_size_per_class',
                     'min_size_per_class', 'transpose_forward', 'transpose_backward', 'data_identifier', 'plans_per_stage',
                     'preprocessor_name', 'conv_per_stage']
    assert pg.difference(planner.plans, written, "planner.plans") is None          # the pickled file round-trips
    # every cropped <case>.pkl has gained the mask decision, and kept what it had
    for c in dataset["cases"]:
        with open(os.path.join(cropped, c + ".pkl"), "rb") as f:
            props = pickle.load(f)
        assert props["case"] == c and pg.difference(props['use_nonzero_mask_for_norm'], want['use_mask_for_norm']) is None
    # load_my_plans gives the planner its state back
    again = _planner_class(run["planner"])(cropped, os.path.dirname(planner.plans_fname))
    again.load_my_plans()
    assert pg.difference(again.plans, written) is None and again.transpose_forward == written['transpose_forward']
    assert again.plans_per_stage is again.plans['plans_per_stage']


def test_plans_hold_only_plain_python_and_numpy_objects(tmp_path):
    planner, _, _ = _plan(str(tmp_path), RUNS[2])
    pg.encode(planner.plans)                                      # raises on anything else
    blob = pickle.dumps(planner.plans)
    assert b"e2enet_medical_amd" not in blob                      # nothing that needs this package to load


@pytest.mark.parametrize("name", sorted(GOLDEN["calls"]))
def test_recorded_calls_of_the_layout_and_the_estimate(name):
    from e2enet_medical_amd.experiment_planning import common_utils
    from e2enet_medical_amd.network_architecture.generic_UNet import Generic_UNet
    fn = Generic_UNet.compute_approx_vram_consumption if name == "compute_approx_vram_consumption" else getattr(common_utils, name)
    assert len(GOLDEN["calls"][name]) >= 5
    for call in GOLDEN["calls"][name]:
        call = pg.decode(call)
        got = fn(*call["args"], **call["kwargs"])
        d = pg.difference(got, call["result"], name)
        assert d is None, "%s%r: %s" % (name, tuple(call["args"]), d)


def test_the_small_helpers_of_the_layout():
    from e2enet_medical_amd.experiment_planning.common_utils import (get_network_numpool, get_shape_must_be_divisible_by, pad_shape)
    assert list(get_shape_must_be_divisible_by([3, 5, 5])) == [8, 32, 32]
    assert list(pad_shape([56, 190, 160], [8, 32, 32])) == [56, 192, 160] and list(pad_shape([5, 7], 4)) == [8, 8]
    assert pad_shape([5, 7], 4).dtype == np.int64
    assert get_network_numpool([128, 128, 128]) == [5, 5, 5] and get_network_numpool([20, 320, 7], maxpool_cap=4) == [2, 4, 0]
    with pytest.raises(AssertionError):
        pad_shape([5, 7], [4])


def test_generic_unet_is_the_estimate_only():
    from e2enet_medical_amd.network_architecture.generic_UNet import Generic_UNet
    assert (Generic_UNet.DEFAULT_BATCH_SIZE_3D, Generic_UNet.BASE_NUM_FEATURES_3D, Generic_UNet.MAX_NUM_FILTERS_3D,
            Generic_UNet.use_this_for_batch_size_computation_3D) == (2, 30, 320, 520000000)
    with pytest.raises(NotImplementedError) as e:
        Generic_UNet(1, 30, 3, 5)
    assert "shiftConvPP" in str(e.value) and "'ori'" in str(e.value)
    # 128^3, five isotropic poolings, 30 features, one modality, three classes: by hand
    v = 128 ** 3
    want = 5 * v * 30 + v + 3 * v + sum((5 if s < 4 else 2) * (v >> (3 * (s + 1))) * min(30 * 2 ** (s + 1), 320) for s in range(5))
    got = Generic_UNet.compute_approx_vram_consumption([128, 128, 128], [5, 5, 5], 30, 320, 1, 3, [[2, 2, 2]] * 5)
    assert got == want and isinstance(got, np.int64)


def test_the_trainer_accepts_a_produced_plans_file(tmp_path):
    from e2enet_medical_amd.training.network_training.nnUNetTrainer_simple import nnUNetTrainer_simple
    run = [r for r in RUNS if r["dataset"] == "ct_two_stage" and r["planner"] == "ExperimentPlanner3D_v21"][0]
    planner, _, _ = _plan(str(tmp_path), run)
    tr = nnUNetTrainer_simple(planner.plans_fname, 0, output_folder=None, stage=1, Tconv='shiftConvPP')
    tr.load_plans_file()
    tr.process_plans(tr.plans)
    full = planner.plans['plans_per_stage'][1]
    assert tr.threeD and tr.batch_size == full['batch_size'] and list(tr.patch_size) == list(full['patch_size'])
    assert tr.net_num_pool_op_kernel_sizes == full['pool_op_kernel_sizes'] and tr.num_classes == 3 and tr.num_input_channels == 1
    assert tr.base_num_features == 32 and tr.transpose_forward == planner.plans['transpose_forward']
    assert tr.normalization_schemes == OrderedDict([(0, "CT")]) and tr.do_dummy_2D_aug == full['do_dummy_2D_data_aug']


# ------------------------------------------------------------------------------------------------------------------ the command
def test_the_command_refuses_what_is_not_built_before_any_work(tmp_path, monkeypatch):
    from e2enet_medical_amd.experiment_planning import nnUNet_plan_and_preprocess as cmd
    monkeypatch.setenv("nnUNet_raw_data_base", str(tmp_path / "raw"))
    monkeypatch.setenv("nnUNet_preprocessed", str(tmp_path / "pre"))
    touched = []
    monkeypatch.setattr(cmd, "crop", lambda *a, **k: touched.append("crop"))
    monkeypatch.setattr(cmd, "convert_id_to_task_name", lambda i: touched.append("task") or "Task%03d_x" % i)
    with pytest.raises(RuntimeError) as e:
        cmd.main(["-t", "997", "-pl3d", "ExperimentPlanner3D_v99"])
    assert "Could not find the Planner class ExperimentPlanner3D_v99" in str(e.value)
    with pytest.raises(NotImplementedError) as e:
        cmd.main(["-t", "997", "-pl2d", "ExperimentPlanner2D_v21"])
    assert "2-D" in str(e.value) and "ExperimentPlanner2D_v21" in str(e.value)
    with pytest.raises(NotImplementedError) as e:
        cmd.main(["-t", "997", "-overwrite_plans", "some_plans.pkl", "-overwrite_plans_identifier", "X",
                  "-pl3d", "ExperimentPlanner3D_v21_Pretrained"])
    assert "overwrite_plans" in str(e.value)
    assert touched == [] and not os.path.exists(str(tmp_path / "raw")) and not os.path.exists(str(tmp_path / "pre"))
    # the names that are taken
    args = cmd.build_parser().parse_args(["-t", "1", "2"])
    assert args.task_ids == [1, 2] and args.planner3d == "ExperimentPlanner3D_v21" and args.planner2d is None
    assert (args.tl, args.tf, args.no_pp, args.verify_dataset_integrity, args.native_nifti) == (8, 8, False, False, False)
    assert cmd.select_planners(args).__name__ == "ExperimentPlanner3D_v21"
    assert cmd.select_planners(cmd.build_parser().parse_args(["-t", "1", "-pl3d", "ExperimentPlanner"])).__name__ == "ExperimentPlanner"
    assert cmd.select_planners(cmd.build_parser().parse_args(["-t", "1", "-pl3d", "None", "-pl2d", "None"])) is None


# ---------------------------------------------------------------------------------------------------------------- sanity checks
class _Geometry(object):
    def __init__(self, origin=(0., 0., 0.), spacing=(1., 1., 2.), direction=(1., 0., 0., 0., 1., 0., 0., 0., 1.), shape=(4, 5, 6)):
        self.itk_origin, self.itk_spacing, self.itk_direction, self.shape = origin, spacing, direction, shape


def test_verify_same_geometry_says_what_differs(capsys):
    from e2enet_medical_amd.preprocessing.sanity_checks import verify_same_geometry
    assert verify_same_geometry(_Geometry(), _Geometry()) and capsys.readouterr().out == ""
    assert verify_same_geometry(_Geometry(spacing=(1., 1., 2.)), _Geometry(spacing=(1., 1., 2. + 1e-9)))         # within np.isclose
    capsys.readouterr()
    assert not verify_same_geometry(_Geometry(origin=(0., 1., 0.)), _Geometry())
    assert capsys.readouterr().out == "the origin does not match between the images:\n(0.0, 1.0, 0.0)\n(0.0, 0.0, 0.0)\n"
    assert not verify_same_geometry(_Geometry(spacing=(1., 1., 2.5)), _Geometry(shape=(4, 5, 7)))
    assert capsys.readouterr().out == ("the spacing does not match between the images\n(1.0, 1.0, 2.5)\n(1.0, 1.0, 2.0)\n"
                                       "the size does not match between the images\n(6, 5, 4)\n(7, 5, 4)\n")
    flipped = (-1., 0., 0., 0., 1., 0., 0., 0., 1.)
    assert not verify_same_geometry(_Geometry(direction=flipped), _Geometry())
    assert capsys.readouterr().out.startswith("the direction does not match between the images\n")


def test_verify_same_geometry_of_two_headers(tmp_path):
    from e2enet_medical_amd import nifti
    from e2enet_medical_amd.preprocessing.sanity_checks import verify_same_geometry
    vol = np.zeros((3, 4, 5), dtype=np.int16)
    for name, pixdim in (("a", (1., 0.7, 0.8, 2.5, 0., 0., 0., 0.)), ("b", (1., 0.7, 0.8, 2.5, 0., 0., 0., 0.)),
                         ("c", (1., 0.7, 0.9, 2.5, 0., 0., 0., 0.))):
        hdr = no.build_header(vol.shape, 4, pixdim=pixdim, qform_code=1, qoffset_x=-3.0)
        no.write_file(str(tmp_path / (name + ".nii.gz")), no.file_bytes(hdr, no.voxel_bytes(vol)))
    a, b, c = (nifti.read_raw(str(tmp_path / (n + ".nii.gz"))) for n in "abc")
    assert verify_same_geometry(a, b) and not verify_same_geometry(a, c)


def test_orientation_codes_of_direction_matrices(tmp_path):
    from e2enet_medical_amd.preprocessing.sanity_checks import axcodes_of_direction, verify_all_same_orientation
    assert axcodes_of_direction((1., 0., 0., 0., 1., 0., 0., 0., 1.)) == ("L", "P", "S")          # ITK's identity is LPS
    assert axcodes_of_direction((-1., 0., 0., 0., -1., 0., 0., 0., 1.)) == ("R", "A", "S")
    assert axcodes_of_direction((0., 0., 1., -1., 0., 0., 0., 1., 0.)) == ("A", "S", "L")         # x runs to anterior, y up, z left
    c, s = np.cos(np.radians(20.)), np.sin(np.radians(20.))
    assert axcodes_of_direction((-c, s, 0., -s, -c, 0., 0., 0., -1.)) == ("R", "A", "I")          # 20 degrees off the axes, z down
    # a folder of headers: identity qform (RAS in NIfTI terms) and one flipped along x
    vol = np.zeros((2, 3, 4), dtype=np.uint8)
    same = tmp_path / "same"
    mixed = tmp_path / "mixed"
    for folder, quaterns in ((same, [(0., 0., 0.), (0., 0., 0.)]), (mixed, [(0., 0., 0.), (0., 1., 0.)])):
        os.makedirs(str(folder))
        for i, (qb, qc, qd) in enumerate(quaterns):
            hdr = no.build_header(vol.shape, 2, qform_code=1, quatern_b=qb, quatern_c=qc, quatern_d=qd)
            no.write_file(str(folder / ("v%d.nii.gz" % i)), no.file_bytes(hdr, no.voxel_bytes(vol)))
    ok, codes = verify_all_same_orientation(str(same))
    assert ok and codes.tolist() == [["R", "A", "S"]]
    ok, codes = verify_all_same_orientation(str(mixed))
    assert not ok and sorted(codes.tolist()) == [["L", "A", "I"], ["R", "A", "S"]]                # 180 degrees about y


def _task_folder(root, training=("c_a", "c_b"), labels=("0", "1", "2"), test=(), listed=None, modalities=1):
    folder = os.path.join(str(root), "Task998_Checks")
    for sub in ("imagesTr", "labelsTr", "imagesTs"):
        os.makedirs(os.path.join(folder, sub))
    vol = np.zeros((2, 3, 4), dtype=np.uint8)
    blob = no.file_bytes(no.build_header(vol.shape, 2), no.voxel_bytes(vol))
    for c in training:
        for m in range(modalities):
            no.write_file(os.path.join(folder, "imagesTr", "%s_%04d.nii.gz" % (c, m)), blob)
        no.write_file(os.path.join(folder, "labelsTr", c + ".nii.gz"), blob)
    for c in test:
        for m in range(modalities):
            no.write_file(os.path.join(folder, "imagesTs", "%s_%04d.nii.gz" % (c, m)), blob)
    listed = training if listed is None else listed
    with open(os.path.join(folder, "dataset.json"), "w") as f:
        json.dump({"modality": {str(m): "MRI" for m in range(modalities)}, "labels": {k: "l" + k for k in labels},
                   "training": [{"image": "./imagesTr/%s.nii.gz" % c, "label": "./labelsTr/%s.nii.gz" % c} for c in listed],
                   "test": ["./imagesTs/%s.nii.gz" % c for c in test]}, f)
    return folder


def test_integrity_outcomes_that_need_no_voxels(tmp_path, monkeypatch):
    """the outcomes that are decided before a voxel is looked at (the scan is replaced by one that must not be reached, or by a clean
    result where the check comes after the voxel pass)"""
    from e2enet_medical_amd import nifti
    from e2enet_medical_amd.preprocessing import sanity_checks as sc

    def no_scan(raw):
        raise AssertionError("the scan was reached")
    clean = lambda raw: nifti.NiftiScan(0, -1, 0, -1, np.bincount([0], minlength=256) * int(np.prod(raw.shape)))
    monkeypatch.setattr(nifti, "scan", no_scan)
    with pytest.raises(AssertionError) as e:
        sc.verify_dataset_integrity(str(tmp_path / "nowhere"))
    assert "dataset.json" in str(e.value)
    with pytest.raises(RuntimeError) as e:                        # duplicate identifiers
        sc.verify_dataset_integrity(_task_folder(tmp_path / "dup", listed=("c_a", "c_b", "c_a")))
    assert "duplicate training cases" in str(e.value)
    folder = _task_folder(tmp_path / "missing", training=("c_b",), listed=("c_b", "c_a"))
    monkeypatch.setattr(nifti, "scan", clean)
    with pytest.raises(AssertionError) as e:                      # a listed case without files: after the cases before it
        sc.verify_dataset_integrity(folder, 2)
    assert "could not find label file for case c_a" in str(e.value)
    folder = _task_folder(tmp_path / "missing_image", modalities=2)
    os.remove(os.path.join(folder, "imagesTr", "c_b_0001.nii.gz"))
    with pytest.raises(AssertionError) as e:
        sc.verify_dataset_integrity(folder, 2)
    assert "some image files are missing for case c_b" in str(e.value)
    folder = _task_folder(tmp_path / "straggler", training=("c_a", "c_b"), listed=("c_a",))
    with pytest.raises(AssertionError) as e:
        sc.verify_dataset_integrity(folder, 2)
    assert "not listed in dataset.json" in str(e.value) and "c_b_0000.nii.gz" in str(e.value)
    with pytest.raises(AssertionError) as e:                      # labels 0, 1, 3
        sc.verify_dataset_integrity(_task_folder(tmp_path / "gap", labels=("0", "1", "3")), 2)
    assert "consecutive order" in str(e.value) and "[3]" in str(e.value)
    with pytest.raises(AssertionError) as e:
        sc.verify_dataset_integrity(_task_folder(tmp_path / "no_background", labels=("1", "2")), 2)
    assert "first label must be 0" in str(e.value)
    # and a folder with nothing wrong, test set included, passes with the clean scan
    sc.verify_dataset_integrity(_task_folder(tmp_path / "fine", test=("t_a",), modalities=2), 3)
