"""Region targets without a device: the fixture against a float64 restatement of the loss formulas, region words, the array-level
region evaluation, and the region trainer's configuration / lookup by name."""
import numpy as np
import pytest
import torch

from tests.helpers import golden, seeded_input

SHAPES = [(2, 3, 8, 12, 10), (2, 3, 4, 6, 5), (2, 3, 2, 3, 5), (2, 3, 1, 3, 5)]
CONFIGS = (("sample", False, 0.), ("batch", True, 1e-5))

PLANS = {'plans_per_stage': {0: {'batch_size': 2, 'patch_size': [16, 32, 32], 'num_pool_per_axis': [3, 5, 5],
                                 'pool_op_kernel_sizes': [[2, 2, 2]] * 3 + [[1, 2, 2]] * 2,
                                 'conv_kernel_sizes': [[3, 3, 3]] * 6, 'do_dummy_2D_data_aug': False}},
         'base_num_features': 32, 'num_modalities': 1, 'num_classes': 3, 'all_classes': [1, 2, 3],
         'transpose_forward': [0, 1, 2], 'transpose_backward': [0, 1, 2], 'conv_per_stage': 2}


def region_loss_fp64(logits, y, batch_dice, smooth):
    """(loss, dloss/dlogits) of one scale in float64, from the closed forms: BCE in its stable form, soft Dice over every
    region, and the gradient  (p - y)/(B R S) + p (1 - p) g,  g = -(2 Dn - N)/(Dn^2 M) where y = 1, N/(Dn^2 M) where y = 0."""
    l, y = logits.double(), y.double()
    b, r = l.shape[:2]
    s = l[0, 0].numel()
    p = torch.sigmoid(l)
    bce = (l.clamp(min=0) - l * y + torch.log1p(torch.exp(-l.abs()))).sum() / (b * r * s)
    axes = tuple(range(2, l.dim()))
    tp, fp, fn = (p * y).sum(axes), (p * (1 - y)).sum(axes), ((1 - p) * y).sum(axes)          # [B, R]
    if batch_dice:
        tp, fp, fn = tp.sum(0, keepdim=True), fp.sum(0, keepdim=True), fn.sum(0, keepdim=True)
    n, dn = 2 * tp + smooth, 2 * tp + fp + fn + smooth + 1e-8
    m = tp.numel()
    loss = bce - (n / dn).mean()
    shape = dn.shape + (1,) * len(axes)
    g_hit, g_miss = (-(2 * dn - n) / (dn * dn * m)).reshape(shape), (n / (dn * dn * m)).reshape(shape)
    grad = (p - y) / (b * r * s) + p * (1 - p) * torch.where(y > 0.5, g_hit, g_miss)
    return loss, grad


def multihot_np(labels, regions):
    """numpy restatement of the reference's conversion loop: region r is 1 where the label equals one of its labels"""
    sets = list(regions.values()) if isinstance(regions, dict) else list(regions)
    out = np.zeros((labels.shape[0], len(sets)) + labels.shape[2:], dtype=np.float32)
    for b in range(labels.shape[0]):
        for r, s in enumerate(sets):
            for l in s:
                out[b, r][labels[b, 0] == l] = 1
    return out


def test_golden_is_reproduced_by_the_float64_formulas():
    """The golden is the reference's own fp32 run; its distance from fp64 is fp32 rounding (value ~1e-7, gradients ~1e-10)."""
    g = golden("regions_loss.npz")
    from e2enet_medical_amd.evaluation.region_based_evaluation import get_brats_regions
    regions = get_brats_regions()
    assert [tuple(int(v) for v in row if v >= 0) for row in g["region_labels"]] == [tuple(v) for v in regions.values()]
    logits = [seeded_input(s, seed=50 + i).mul(2.0) for i, s in enumerate(SHAPES)]
    for i in range(4):
        labels = g["labels%d" % i]
        assert labels.min() == 0 and labels.max() == 3 and not (labels[0] == 3).any()        # label 3 absent from sample 0
        assert np.array_equal(g["multihot%d" % i], multihot_np(labels, regions))
    w = g["ds_weights"]
    for tag, bd, smooth in CONFIGS:
        total = 0.0
        for i in range(4):
            loss, grad = region_loss_fp64(logits[i], torch.from_numpy(g["multihot%d" % i].astype(np.float32)), bd, smooth)
            # the closed-form gradient is the autograd gradient of the closed-form value
            leaf = logits[i].double().requires_grad_(True)
            y = torch.from_numpy(g["multihot%d" % i].astype(np.float64))
            p = torch.sigmoid(leaf)
            axes = (0, 2, 3, 4) if bd else (2, 3, 4)
            tp, fp, fn = (p * y).sum(axes), (p * (1 - y)).sum(axes), ((1 - p) * y).sum(axes)
            auto = torch.nn.functional.binary_cross_entropy_with_logits(leaf, y) - \
                ((2 * tp + smooth) / (2 * tp + fp + fn + smooth + 1e-8)).mean()
            auto.backward()
            assert abs(auto.item() - loss.item()) < 1e-12
            assert float((leaf.grad - grad).abs().max()) < 1e-15
            total += w[i] * loss.item()
            np.testing.assert_allclose(w[i] * grad.numpy(), g[tag + "_g%d" % i], rtol=0, atol=2e-7)
            assert np.isfinite(grad.numpy()).all()
        assert abs(total - float(g[tag + "_loss"])) < 1e-6
        assert abs(total - float(g[tag + "_loss_fp64"])) < 1e-12
    # hard counts of the full-resolution scale
    assert float(logits[0].abs().min()) >= 1e-6
    pos = (logits[0] > 0).numpy()
    y = g["multihot0"].astype(bool)
    want = np.stack([(pos & y).sum((0, 2, 3, 4)), (pos & ~y).sum((0, 2, 3, 4)), (~pos & y).sum((0, 2, 3, 4))], 1)
    assert np.array_equal(g["hard_tp_fp_fn"], want)


def test_region_words_from_region_dicts():
    from e2enet_medical_amd.evaluation.region_based_evaluation import get_brats_regions, get_KiTS_regions
    from e2enet_medical_amd.training.data_augmentation.custom_transforms import region_words
    assert region_words(get_brats_regions()) == (0b1110, 0b1100, 0b1000)
    assert region_words(get_KiTS_regions()) == (0b110, 0b100)
    assert region_words({"with background": (0, 2), "top": (31,)}) == (0b101, 1 << 31)
    assert region_words([(1, 2), (2,)]) == (0b110, 0b100)
    with pytest.raises(ValueError):
        region_words({"too large": (1, 32)})
    with pytest.raises(ValueError):
        region_words({"negative": (-1,)})
    with pytest.raises(ValueError):
        region_words({})
    with pytest.raises(ValueError):
        region_words([(1,)] * 33)


def test_evaluate_case_against_numpy():
    from e2enet_medical_amd.evaluation.region_based_evaluation import (evaluate_case, get_brats_regions, get_KiTS_regions,
                                                                        create_region_from_mask)
    rng = np.random.RandomState(0)
    pred, gt = rng.randint(0, 4, (9, 11, 7)), rng.randint(0, 4, (9, 11, 7))
    pred[pred == 3] = 0
    gt[gt == 3] = 0                                     # 'enhancing tumor' empty in both
    regions = get_brats_regions()
    got = evaluate_case(pred, gt, regions)
    assert len(got) == 3
    for d, labels in zip(got[:2], list(regions.values())[:2]):
        a, b = np.isin(pred, labels), np.isin(gt, labels)
        assert abs(d - 2.0 * (a & b).sum() / (a.sum() + b.sum())) < 1e-15
    assert np.isnan(got[2])
    assert evaluate_case(pred, gt, list(regions.values()))[:2] == got[:2]
    gt2 = gt.copy()
    gt2[0, 0, 0] = 3                                    # present in the ground truth only: Dice 0, not nan
    assert evaluate_case(pred, gt2, regions)[2] == 0.0
    m = create_region_from_mask(gt, (1, 2))
    assert m.dtype == np.uint8 and np.array_equal(m.astype(bool), np.isin(gt, (1, 2)))
    assert list(get_KiTS_regions().keys()) == ["kidney incl tumor", "tumor"]
    with pytest.raises(ValueError):
        evaluate_case(pred, gt[:-1], regions)


def test_region_trainer_configuration_and_lookup(tmp_path):
    from e2enet_medical_amd.training.network_training.competitions_with_custom_Trainers.BraTS2020.nnUNetTrainerV2BraTSRegions \
        import nnUNetTrainerV2BraTSRegions
    from e2enet_medical_amd.training.network_training.nnUNetTrainer_simple import nnUNetTrainer_simple
    from e2enet_medical_amd.training.loss_functions.dice_loss import DC_and_BCE_loss
    from e2enet_medical_amd.evaluation.region_based_evaluation import get_brats_regions
    from e2enet_medical_amd.training import model_restore
    from e2enet_medical_amd import simple_main
    tr = nnUNetTrainerV2BraTSRegions(PLANS, 0, output_folder=str(tmp_path), batch_dice=True, Tconv='shiftConvPP')
    assert isinstance(tr, nnUNetTrainer_simple)
    assert tr.regions == get_brats_regions() and tr.regions_class_order == (1, 2, 3)
    assert isinstance(tr.loss, DC_and_BCE_loss) and tr.loss.batch_dice is False and tr.loss.smooth == 0.0
    assert tr.batch_dice is False
    tr.process_plans(PLANS)
    assert tr.num_classes == 3 and tr._num_labels() == 4
    kw = tr._engine_loss_kwargs()
    assert kw == {'smooth': 0.0, 'regions': (14, 12, 8)}
    assert nnUNetTrainer_simple(PLANS, 0, Tconv='shiftConvPP')._engine_loss_kwargs() == {}
    # what the loss module refuses
    with pytest.raises(NotImplementedError):
        DC_and_BCE_loss({'pos_weight': torch.ones(3)}, {'batch_dice': False, 'do_bg': True, 'smooth': 0})
    with pytest.raises(NotImplementedError):
        DC_and_BCE_loss({}, {'batch_dice': False, 'do_bg': False, 'smooth': 0})
    with pytest.raises(NotImplementedError):
        DC_and_BCE_loss({}, {'batch_dice': False, 'do_bg': True, 'smooth': 0}, aggregate="mean")
    with pytest.raises(RuntimeError):                    # no CPU fallback
        DC_and_BCE_loss({}, {})(torch.zeros(1, 2, 4, 4, 4), torch.zeros(1, 2, 4, 4, 4))
    # lookup by the reference's name
    assert model_restore.recursive_find_python_class("nnUNetTrainerV2BraTSRegions") is nnUNetTrainerV2BraTSRegions
    assert model_restore.recursive_find_python_class("nnUNetTrainer_simple") is nnUNetTrainer_simple
    assert model_restore.recursive_find_python_class("nnUNetTrainerV2BraTSRegions_BN") is None
    assert simple_main.select_trainer_class("nnUNetTrainerV2BraTSRegions") is nnUNetTrainerV2BraTSRegions
    for other in ("nnUNetTrainerV2", "nnUNetTrainer_simple", "anything"):
        assert simple_main.select_trainer_class(other) is nnUNetTrainer_simple
    args = simple_main.build_parser().parse_args(["--network_trainer", "nnUNetTrainerV2BraTSRegions"])
    assert simple_main.select_trainer_class(args.network_trainer) is nnUNetTrainerV2BraTSRegions
    assert simple_main.select_trainer_class(simple_main.build_parser().parse_args([]).network_trainer) is nnUNetTrainer_simple


def test_restore_model_builds_the_trainer_named_in_the_pickle(tmp_path):
    import pickle
    from collections import OrderedDict
    from e2enet_medical_amd.training.model_restore import restore_model
    for name in ("nnUNetTrainerV2BraTSRegions", "nnUNetTrainer_simple"):
        pkl = str(tmp_path / (name + ".pkl"))
        with open(pkl, "wb") as f:
            pickle.dump(OrderedDict(init=(PLANS, 0, str(tmp_path), None, True, None, True, True, False), name=name, plans=PLANS), f)
        tr = restore_model(pkl)
        assert type(tr).__name__ == name
        assert tr.num_classes == (3 if name == "nnUNetTrainerV2BraTSRegions" else 4)
    with open(str(tmp_path / "x.pkl"), "wb") as f:
        pickle.dump(OrderedDict(init=(), name="nnUNetTrainerV2", plans=PLANS), f)
    with pytest.raises(RuntimeError, match="Could not find the model trainer"):
        restore_model(str(tmp_path / "x.pkl"))


def test_get_moredA_augmentation_still_refuses_soft_ds():
    from e2enet_medical_amd.training.data_augmentation.data_augmentation_moreDA import get_moreDA_augmentation
    with pytest.raises(NotImplementedError):
        get_moreDA_augmentation([], [], (16, 32, 32), {'do_mirror': True}, soft_ds=True)
