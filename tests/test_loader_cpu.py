"""Host half of the resident training loader (training/dataloading/resident_loading.py) without a GPU: the draw plan it shares with
DataLoader3D, the budget bookkeeping of DeviceCaseCache, and the refusals."""
import numpy as np
import pytest
import torch

from e2enet_medical_amd.training.dataloading import dataset_loading
from e2enet_medical_amd.training.dataloading.dataset_loading import DataLoader3D
from e2enet_medical_amd.training.dataloading.resident_loading import DeviceCaseCache, ResidentDataLoader3D
from tests.helpers import synthetic_cases


class _FakeCache:
    """every case 'resident' as its host array"""
    device = "cpu"

    def fetch(self, entry, memmap_mode="r"):
        return dataset_loading._load_case(entry, memmap_mode), True


def _numpy_crop(log):
    """e2e_loader_crop restated with np.pad; notes the (shape, offset) of every sample it is asked for"""
    def crop(sources, offsets, num_channels, patch_size, data_mode, data_fill, seg_fill, device):
        data = np.empty((len(sources), num_channels) + tuple(patch_size), np.float32)
        seg = np.empty((len(sources), 1) + tuple(patch_size), np.float32)
        for j, (src, off) in enumerate(zip(sources, offsets)):
            log.append((tuple(src.shape), tuple(off)))
            shape = src.shape[1:]
            lo = [max(0, off[d]) for d in range(3)]
            hi = [min(shape[d], off[d] + patch_size[d]) for d in range(3)]
            box = np.asarray(src[:, lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]])
            pad = ((0, 0),) + tuple((lo[d] - off[d], off[d] + patch_size[d] - hi[d]) for d in range(3))
            if data_mode == 1:
                data[j] = np.pad(box[:-1], pad, "edge")
            else:
                data[j] = np.pad(box[:-1], pad, "constant", constant_values=data_fill)
            seg[j] = np.pad(box[-1:], pad, "constant", constant_values=seg_fill)
        return torch.from_numpy(data), torch.from_numpy(seg)
    return crop


@pytest.mark.parametrize("mode,kw", [("edge", None), ("constant", {'constant_values': 0})])
def test_both_loaders_draw_the_same_plan_and_leave_the_stream_at_the_same_position(tmp_path, mode, kw):
    ds = synthetic_cases(str(tmp_path))
    args = (ds, (16, 18, 20), (12, 14, 16), 4, False)
    kwargs = dict(oversample_foreground_percent=0.33, pad_mode=mode, pad_kwargs_data=kw)

    np.random.seed(1234)
    host = DataLoader3D(*args, **kwargs)
    plans = [host.draw_batch(lambda e: dataset_loading._load_case(e, "r")) for _ in range(3)]
    after = np.random.randint(0, 2 ** 31 - 1, 4)

    np.random.seed(1234)
    host = DataLoader3D(*args, **kwargs)
    batches = [{k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in next(host).items()} for _ in range(3)]
    assert np.array_equal(np.random.randint(0, 2 ** 31 - 1, 4), after)

    np.random.seed(1234)
    log = []
    res = ResidentDataLoader3D(*args, cache=_FakeCache(), crop=_numpy_crop(log), **kwargs)
    assert res.data_shape == host.data_shape and res.seg_shape == host.seg_shape
    for it in range(3):
        b = next(res)
        keys, plan = plans[it]
        assert [str(k) for k in b['keys']] == [str(k) for k in keys] == [str(k) for k in batches[it]['keys']]
        assert [o for _, o in log[4 * it:4 * it + 4]] == [tuple(int(v) for v in bb) for _, _, _, bb in plan]
        assert [s for s, _ in log[4 * it:4 * it + 4]] == [tuple(case.shape) for _, case, _, _ in plan]
        assert [p['name'] for p in b['properties']] == [str(k) for k in keys]
        assert "data_pinned" not in b and "seg_pinned" not in b
        assert np.array_equal(b['data'].numpy(), batches[it]['data']) and np.array_equal(b['seg'].numpy(), batches[it]['seg'])
    assert np.array_equal(np.random.randint(0, 2 ** 31 - 1, 4), after)
    assert res.batches == 3 and res.staged_samples == 0


def _entries(tmp_path, sizes):
    """cases of sizes[i] fp32 words each, as [2, 1, 1, n / 2]"""
    out = []
    for i, n in enumerate(sizes):
        path = str(tmp_path / ("c%d" % i))
        np.save(path + ".npy", np.arange(n, dtype=np.float32).reshape(2, 1, 1, n // 2))
        out.append({'data_file': path + ".npz"})
    return out


def test_budget_bookkeeping(tmp_path):
    uploads = []

    def upload(a):
        uploads.append(a.shape)
        return np.array(a)
    e = _entries(tmp_path, [8, 16, 4, 2, 2])                                       # 32, 64, 16, 8, 8 bytes

    everything = DeviceCaseCache(None, "cpu", upload)
    assert all(everything.fetch(x)[1] for x in e) and len(everything) == 5 and everything.resident_bytes == 128

    nothing = DeviceCaseCache(0, "cpu", upload)
    got = [nothing.fetch(x) for x in e]
    assert not any(r for _, r in got) and len(nothing) == 0 and nothing.resident_bytes == 0
    assert isinstance(got[0][0], np.ndarray) and got[0][0].shape == (2, 1, 1, 4)      # the host array, as _load_case returns it

    del uploads[:]
    c = DeviceCaseCache(56, "cpu", upload)
    assert c.fetch(e[0])[1] and c.resident_bytes == 32                                # 32 of 56
    assert not c.fetch(e[1])[1] and c.resident_bytes == 32                            # 64 do not fit; nothing is evicted for it
    assert c.fetch(e[2])[1] and c.resident_bytes == 48                                # 16 fit
    assert c.fetch(e[3])[1] and c.resident_bytes == 56                                # exactly what is left
    assert not c.fetch(e[4])[1] and c.resident_bytes == 56                            # full
    assert c.fetch(e[0])[1] and not c.fetch(e[1])[1]                                  # and it stays that way
    assert len(c) == 3 and e[0]['data_file'] in c and e[1]['data_file'] not in c
    assert len(uploads) == 3                                                          # one upload per resident case

    one_byte_short = DeviceCaseCache(31, "cpu", upload)
    assert not one_byte_short.fetch(e[0])[1] and one_byte_short.fetch(e[2])[1]
    with pytest.raises(ValueError):
        DeviceCaseCache(-1, "cpu", upload)


def test_a_resident_case_is_not_loaded_again(tmp_path, monkeypatch):
    e = _entries(tmp_path, [8, 16])
    calls = []
    real = dataset_loading._load_case
    monkeypatch.setattr(dataset_loading, "_load_case", lambda *a, **k: calls.append(a[0]['data_file']) or real(*a, **k))
    c = DeviceCaseCache(32, "cpu", lambda a: np.array(a))
    for _ in range(3):
        c.fetch(e[0])
        c.fetch(e[1])
    assert calls.count(e[0]['data_file']) == 1 and calls.count(e[1]['data_file']) == 3


def test_error_paths(tmp_path, monkeypatch):
    ds = synthetic_cases(str(tmp_path))
    args = (ds, (16, 18, 20), (12, 14, 16), 4)
    fake = dict(cache=_FakeCache(), crop=_numpy_crop([]))
    with pytest.raises(NotImplementedError, match="previous-stage"):
        ResidentDataLoader3D(*args, True, **fake)
    with pytest.raises(NotImplementedError, match="reflect"):
        ResidentDataLoader3D(*args, False, pad_mode="reflect", **fake)
    with pytest.raises(NotImplementedError, match="pad_kwargs_data"):
        ResidentDataLoader3D(*args, False, pad_mode="constant", pad_kwargs_data={'stat_length': 2}, **fake)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no GPU is visible"):
        ResidentDataLoader3D(*args, False, cache=DeviceCaseCache(None))
    with pytest.raises(NotImplementedError):                    # the cascade is refused whether or not a GPU is there
        ResidentDataLoader3D(*args, True, cache=DeviceCaseCache(None))


def test_trainer_switch_is_off_by_default_and_the_parser_takes_it():
    from e2enet_medical_amd.simple_main import build_parser
    from e2enet_medical_amd.training.network_training.nnUNetTrainer_simple import nnUNetTrainer_simple
    assert build_parser().parse_args([]).resident_data is None
    assert build_parser().parse_args(["--resident_data", "1.5"]).resident_data == 1.5
    assert build_parser().parse_args(["--resident_data", "-1"]).resident_data == -1.0
    plans = {'plans_per_stage': {0: {'batch_size': 2, 'patch_size': [16, 32, 32], 'num_pool_per_axis': [3, 5, 5],
                                     'pool_op_kernel_sizes': [[2, 2, 2]] * 3 + [[1, 2, 2]] * 2,
                                     'conv_kernel_sizes': [[3, 3, 3]] * 6, 'do_dummy_2D_data_aug': False}},
             'base_num_features': 32, 'num_modalities': 1, 'num_classes': 2, 'all_classes': [1, 2],
             'transpose_forward': [0, 1, 2], 'transpose_backward': [0, 1, 2], 'conv_per_stage': 2}
    assert nnUNetTrainer_simple(plans, 0, Tconv='shiftConvPP').resident_data_gib is None
