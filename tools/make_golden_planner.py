#!/usr/bin/env python
"""Generate tests/golden/planner.json: the reference's experiment planners run on synthetic fingerprints.

    python tools/make_golden_planner.py [REFERENCE_ROOT]

Runs where a checkout of the reference is at hand (default: where tools/make_golden.py looks for it), on the CPU, and is not part of
any test.  Nothing of the
reference is copied: the script imports ``ExperimentPlanner3D_v21`` and ``ExperimentPlanner`` with the third-party modules that are
absent stubbed (batchgenerators' file helpers, SimpleITK, scikit-image) and ``e2enet.training.model_restore`` replaced by an empty
module (it would pull in the trainers), runs ``plan_experiment()`` on synthetic cropped folders -- a ``dataset_properties.pkl``, empty
``<case>.npz`` names, minimal ``<case>.pkl`` files in a temporary folder -- and stores, per dataset, the fingerprint fed in and the plans
dict that came out (tests/planner_golden.py is the file format), plus some of the calls of ``get_pool_and_conv_props*`` and
``compute_approx_vram_consumption`` made on the way, arguments and results.

The datasets are chosen so that the reference takes every branch of its planning; ``check_coverage`` asserts that it did, so a
regeneration cannot quietly lose one."""
import json
import os
import pickle
import sys
import tempfile
import types
from collections import OrderedDict
from copy import deepcopy

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import planner_golden as pg                                          # noqa: E402

MAX_CALLS_PER_FUNCTION = 10


# ------------------------------------------------------------------------------------------------------------------------ stubs
def _file_helpers():
    """what the reference's planner modules take from batchgenerators.utilities.file_and_folder_operations (``import *``)"""
    m = types.ModuleType("batchgenerators.utilities.file_and_folder_operations")

    def subfiles(folder, join=True, prefix=None, suffix=None, sort=True):
        res = [os.path.join(folder, i) if join else i for i in os.listdir(folder)
               if os.path.isfile(os.path.join(folder, i)) and (prefix is None or i.startswith(prefix))
               and (suffix is None or i.endswith(suffix))]
        return sorted(res) if sort else res

    def subdirs(folder, join=True, prefix=None, suffix=None, sort=True):
        res = [os.path.join(folder, i) if join else i for i in os.listdir(folder)
               if os.path.isdir(os.path.join(folder, i)) and (prefix is None or i.startswith(prefix))
               and (suffix is None or i.endswith(suffix))]
        return sorted(res) if sort else res

    def load_pickle(file, mode='rb'):
        with open(file, mode) as f:
            return pickle.load(f)

    def save_pickle(obj, file, mode='wb'):
        with open(file, mode) as f:
            pickle.dump(obj, f)

    def load_json(file):
        with open(file) as f:
            return json.load(f)

    def save_json(obj, file, indent=4, sort_keys=True):
        with open(file, 'w') as f:
            json.dump(obj, f, sort_keys=sort_keys, indent=indent)

    m.__dict__.update(os=os, pickle=pickle, json=json, join=os.path.join, isdir=os.path.isdir, isfile=os.path.isfile,
                      listdir=os.listdir, maybe_mkdir_p=lambda d: os.makedirs(d, exist_ok=True), subfiles=subfiles, subdirs=subdirs,
                      load_pickle=load_pickle, save_pickle=save_pickle, load_json=load_json, save_json=save_json)
    return m


def install_stubs():
    mods = {"batchgenerators": types.ModuleType("batchgenerators"),
            "batchgenerators.utilities": types.ModuleType("batchgenerators.utilities"),
            "batchgenerators.utilities.file_and_folder_operations": _file_helpers(),
            "batchgenerators.augmentations": types.ModuleType("batchgenerators.augmentations"),
            "batchgenerators.augmentations.utils": types.ModuleType("batchgenerators.augmentations.utils"),
            "SimpleITK": types.ModuleType("SimpleITK"),
            "skimage": types.ModuleType("skimage"), "skimage.morphology": types.ModuleType("skimage.morphology"),
            "skimage.transform": types.ModuleType("skimage.transform"),
            "e2enet.training.model_restore": types.ModuleType("e2enet.training.model_restore")}
    mods["batchgenerators.augmentations.utils"].pad_nd_image = None
    mods["skimage.morphology"].label = None
    mods["skimage.transform"].resize = None
    mods["e2enet.training.model_restore"].recursive_find_python_class = None
    sys.modules.update(mods)


# --------------------------------------------------------------------------------------------------------------------- datasets
def _dataset(name, planners, modalities, classes, cases, size_reduction):
    """``cases``: [(spacing, size after cropping)], one per case"""
    ids = ["%s_%03d" % (name, i) for i in range(len(cases))]
    fingerprint = OrderedDict()
    fingerprint['all_sizes'] = [np.array(size) for _, size in cases]
    fingerprint['all_spacings'] = [np.array(spacing, dtype=np.float64) for spacing, _ in cases]
    fingerprint['all_classes'] = list(classes)
    fingerprint['modalities'] = {i: m for i, m in enumerate(modalities)}
    fingerprint['intensityproperties'] = None
    fingerprint['size_reductions'] = OrderedDict((c, size_reduction) for c in ids)
    return {"name": name, "planners": planners, "cases": ids, "fingerprint": fingerprint}


def _jitter(n, spacing, size, dspacing, dsize, seed):
    """n cases around a spacing and a size: spacings that differ from case to case, so that the percentiles interpolate"""
    rng = np.random.RandomState(seed)
    spacing, size = np.array(spacing, dtype=np.float64), np.array(size)
    out = []
    for _ in range(n):
        s = spacing * (1.0 + np.array(dspacing) * rng.uniform(-1, 1, 3))
        out.append((s, size + (np.array(dsize) * rng.uniform(-1, 1, 3)).astype(int)))
    return out


def datasets():
    both = ["ExperimentPlanner3D_v21", "ExperimentPlanner"]
    v21 = ["ExperimentPlanner3D_v21"]
    thick = [((z, 1.25, 1.25), (n, 256, 256 - 8 * (i % 3))) for i, (z, n) in
             enumerate([(5.0, 20), (6.0, 18), (8.0, 14), (10.0, 12), (10.0, 11), (7.5, 15), (10.0, 12), (9.0, 13), (6.5, 17), (10.0, 10)])]
    clamp = [((z, 1.25, 1.3), (n, 240, 240)) for z, n in
             [(0.9, 60), (0.9, 64), (4.0, 22), (4.0, 24), (4.5, 20), (4.0, 21), (5.0, 18), (4.0, 23), (4.0, 22), (4.2, 20), (4.0, 25)]]
    return [
        # 1 mm brain-like MRI, four modalities (one of them noNorm), cropping took 40 % away: one stage, the VRAM loop runs, mask on
        _dataset("iso_mri", both, ["T1", "T2", "FLAIR", "noNorm"], [1, 2, 3],
                 _jitter(20, (1.0, 1.0, 1.0), (138, 170, 138), (0.02, 0.01, 0.03), (6, 8, 6), 1), 0.6),
        # abdominal CT, thick-ish slices: two stages
        _dataset("ct_two_stage", both, ["CT"], [1, 2],
                 _jitter(30, (2.0, 0.78, 0.78), (180, 512, 512), (0.25, 0.1, 0.1), (60, 0, 0), 2), 1.0),
        # thick slices: the anisotropy branch, its 10th percentile stays above the in-plane spacing
        _dataset("thick", v21, ["MRI"], [1], thick, 1.0),
        # a few thin-slice cases among thick ones: the 10th percentile falls below the in-plane spacing and is clamped to it + 1e-5
        _dataset("thick_clamp", v21, ["ct"], [1, 2, 3, 4], clamp, 0.9),
        # the coarse axis is the last one
        _dataset("coarse_last", both, ["MRI", "ADC"], [1, 2],
                 _jitter(16, (0.8, 0.8, 3.0), (320, 320, 40), (0.05, 0.05, 0.1), (16, 16, 6), 3), 0.7),
        # small cases, few of them: the patch is the median case, no VRAM loop, and 5 % of the dataset caps the batch
        _dataset("small_few", both, ["noNorm"], [1],
                 _jitter(10, (1.0, 1.0, 1.0), (40, 56, 40), (0.05, 0.05, 0.05), (3, 4, 3), 4), 1.0),
        # small cases, many of them: the batch grows past 2
        _dataset("small_many", v21, ["T2"], [1, 2],
                 _jitter(60, (1.5, 1.5, 1.5), (48, 64, 48), (0.03, 0.03, 0.03), (4, 4, 4), 5), 0.95),
        # a median case of just over four patches: the lowres walk starts, and what it finds is not small enough to keep
        _dataset("lowres_dropped", v21, ["CT"], [1],
                 _jitter(12, (1.0, 1.0, 1.0), (204, 204, 204), (0.0, 0.0, 0.0), (2, 2, 2), 6), 1.0),
    ]


# ---------------------------------------------------------------------------------------------------------------------- running
class Recorder(object):
    """wraps a function of a module or class: counts the calls and keeps the first few distinct ones, arguments and result"""

    def __init__(self):
        self.calls = {}
        self.counts = {}

    def wrap(self, owner, name, static=False):
        inner = getattr(owner, name)

        def outer(*args, **kwargs):
            before = deepcopy((args, kwargs))
            result = inner(*args, **kwargs)
            self.counts[name] = self.counts.get(name, 0) + 1
            kept = self.calls.setdefault(name, [])
            entry = {"args": list(before[0]), "kwargs": before[1], "result": deepcopy(result)}
            if len(kept) < MAX_CALLS_PER_FUNCTION and not any(pg.difference(entry, k) is None for k in kept):
                kept.append(entry)
            return result
        setattr(owner, name, staticmethod(outer) if static else outer)


def run_one(ds, planner_cls, root):
    cropped, out = os.path.join(root, "cropped"), os.path.join(root, "preprocessed")
    os.makedirs(cropped)
    os.makedirs(out)
    with open(os.path.join(cropped, "dataset_properties.pkl"), "wb") as f:
        pickle.dump(ds["fingerprint"], f)
    for c in ds["cases"]:
        open(os.path.join(cropped, c + ".npz"), "wb").close()
        with open(os.path.join(cropped, c + ".pkl"), "wb") as f:
            pickle.dump(OrderedDict(case=c), f)
    planner = planner_cls(cropped, out)
    stage_calls = []
    inner = planner.get_properties_for_stage
    planner.get_properties_for_stage = lambda *a: stage_calls.append(1) or inner(*a)
    planner.plan_experiment()
    with open(planner.plans_fname, "rb") as f:
        plans = pickle.load(f)
    for c in ds["cases"]:
        with open(os.path.join(cropped, c + ".pkl"), "rb") as f:
            assert pg.difference(pickle.load(f)['use_nonzero_mask_for_norm'], plans['use_mask_for_norm'], c) is None
    return plans, len(stage_calls), os.path.basename(planner.plans_fname)


def facts_of(ds, planner_name, plans, stage_calls, vram_calls, ref_budget):
    """which branches a run took, from its inputs and outputs"""
    fp = ds["fingerprint"]
    spacings = np.vstack(fp['all_spacings'])
    median = np.percentile(spacings, 50, 0)
    full = plans['plans_per_stage'][plans['num_stages'] - 1]
    target = np.array(full['current_spacing'])[plans['transpose_backward']]
    worst = int(np.argmax(median))
    others = [median[i] for i in range(3) if i != worst]
    aniso = bool(target[worst] != median[worst])
    facts = {"stages": plans['num_stages'], "lowres_walk": stage_calls > 1, "aniso": aniso,
             "aniso_clamped": aniso and bool(target[worst] == max(others) + 1e-5),
             "transposed": plans['transpose_forward'] != [0, 1, 2],
             "vram_loop_in_fullres": vram_calls[0] > 1, "dummy_2D": bool(full['do_dummy_2D_data_aug']),
             "batch_size": int(full['batch_size']), "mask": sorted(set(plans['use_mask_for_norm'].values())),
             "schemes": sorted(set(plans['normalization_schemes'].values())),
             "spacings_differ": bool((spacings != spacings[0]).any()), "planner": planner_name}
    cap = max(np.round(0.05 * np.prod(full['median_patient_size_in_voxels']) * len(ds["cases"]) /
                       np.prod(full['patch_size'], dtype=np.int64)).astype(int), 2)
    uncapped = int(np.floor(max(ref_budget / vram_calls[1], 1) * 2))
    facts["cap_binds"] = bool(cap < uncapped and full['batch_size'] == cap)
    return facts


def check_coverage(facts):
    def some(**want):
        hits = [f for f in facts if all(f[k] == v for k, v in want.items())]
        assert hits, "no dataset with %r" % (want,)
    some(stages=1)
    some(stages=2)
    some(stages=1, lowres_walk=True)
    some(aniso=True, aniso_clamped=False)
    some(aniso=True, aniso_clamped=True)
    some(aniso=False)
    some(transposed=True)
    some(vram_loop_in_fullres=True)
    some(vram_loop_in_fullres=False)
    assert any(not f["vram_loop_in_fullres"] and f["batch_size"] > 2 for f in facts), "no clipped patch with a batch above 2"
    some(cap_binds=True)
    some(cap_binds=False)
    some(dummy_2D=True)
    some(dummy_2D=False)
    assert any(True in f["mask"] for f in facts) and any(False in f["mask"] for f in facts)
    assert {"CT", "nonCT", "noNorm"} <= set(s for f in facts for s in f["schemes"])
    some(spacings_differ=True)
    assert sum(f["planner"] == "ExperimentPlanner" for f in facts) >= 2


def main():
    reference = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    sys.path.insert(0, reference)
    install_stubs()
    work = tempfile.mkdtemp()
    os.chdir(work)                                   # (the reference's paths.py creates its relative folders while importing)
    from e2enet.experiment_planning import common_utils, experiment_planner_baseline_3DUNet as base_mod
    from e2enet.experiment_planning import experiment_planner_baseline_3DUNet_v21 as v21_mod
    from e2enet.network_architecture.generic_UNet import Generic_UNet
    classes = {"ExperimentPlanner": base_mod.ExperimentPlanner, "ExperimentPlanner3D_v21": v21_mod.ExperimentPlanner3D_v21}
    rec = Recorder()
    rec.wrap(Generic_UNet, "compute_approx_vram_consumption", static=True)
    rec.wrap(common_utils, "get_pool_and_conv_props")
    rec.wrap(common_utils, "get_pool_and_conv_props_poolLateV2")
    base_mod.get_pool_and_conv_props_poolLateV2 = common_utils.get_pool_and_conv_props_poolLateV2
    v21_mod.get_pool_and_conv_props = common_utils.get_pool_and_conv_props

    runs, facts = [], []
    for ds in datasets():
        for planner_name in ds["planners"]:
            root = os.path.join(work, ds["name"] + "_" + planner_name)
            # the estimate's calls during the fullres stage (the first get_properties_for_stage): how many, and the last result
            seen = {"n": 0, "last": None, "stage": 0}
            inner_vram = Generic_UNet.compute_approx_vram_consumption
            inner_props = classes[planner_name].get_properties_for_stage

            def vram(*a, _inner=inner_vram, **k):
                r = _inner(*a, **k)
                if seen["stage"] == 1:
                    seen["n"], seen["last"] = seen["n"] + 1, r
                return r

            def props(self, *a, _inner=inner_props):
                seen["stage"] += 1
                return _inner(self, *a)
            Generic_UNet.compute_approx_vram_consumption = staticmethod(vram)
            classes[planner_name].get_properties_for_stage = props
            try:
                plans, stage_calls, fname = run_one(ds, classes[planner_name], root)
            finally:
                Generic_UNet.compute_approx_vram_consumption = staticmethod(inner_vram)
                classes[planner_name].get_properties_for_stage = inner_props
            budget = 520000000 * plans['base_num_features'] / 30 if planner_name.endswith("v21") else 520000000
            f = facts_of(ds, planner_name, plans, stage_calls, (seen["n"], seen["last"]), budget)
            facts.append(f)
            print(ds["name"], planner_name, f)
            # the fingerprint is stored once: the plans repeat it in three entries
            for k, v in (('dataset_properties', ds["fingerprint"]), ('original_spacings', ds["fingerprint"]['all_spacings']),
                         ('original_sizes', ds["fingerprint"]['all_sizes'])):
                assert pg.difference(plans.pop(k), v, k) is None
            runs.append({"dataset": ds["name"], "planner": planner_name, "plans_file": fname, "facts": f,
                         "plans": pg.encode(plans, root)})
    check_coverage(facts)
    doc = {"datasets": {ds["name"]: {"cases": ds["cases"], "fingerprint": pg.encode(ds["fingerprint"])} for ds in datasets()},
           "runs": runs,
           "calls": {name: [pg.encode(c) for c in calls] for name, calls in rec.calls.items()}}
    os.makedirs(os.path.dirname(pg.GOLDEN), exist_ok=True)
    with open(pg.GOLDEN, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print("wrote %s (%d bytes, %d runs, calls kept: %s)" % (pg.GOLDEN, os.path.getsize(pg.GOLDEN), len(runs),
                                                            {k: len(v) for k, v in rec.calls.items()}))


if __name__ == "__main__":
    main()
