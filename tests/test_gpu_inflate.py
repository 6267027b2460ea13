"""The device inflater (csrc/inflate.hip; ``deflate.inflate`` / ``load_npz``) on the device encoder's own streams: round trips for
both codes, the scan records against ``tests/inflate_oracle.py`` field for field, false candidates and corrupt records that leave
the output untouched, ``savez`` -> ``load_npz``, the ensemble and the resident loader with ``device_inflate`` against their default
routes, the refusals.  Every comparison is for exact bytes."""
import os
import zipfile
import zlib
from collections import OrderedDict

import numpy as np
import pytest
import torch

from tests import inflate_oracle as oracle
from tests.test_gpu_deflate import CHUNK, SIZES
from tests.test_inflate_cpu import _mixed, _zero_minus_one, named_inputs

pytestmark = pytest.mark.gpu

CODES = ["fixed", "dynamic"]


def _deflate():
    from e2enet_medical_amd import deflate
    assert deflate.chunk_bytes() == CHUNK == deflate.CHUNK
    return deflate


def _round_trip(host, elem, codes):
    """deflate on the device, inflate on the device: the bytes, and the CRC kernels on their own; returns (body, stats)"""
    d = _deflate()
    host = np.ascontiguousarray(host).view(np.uint8).reshape(-1)
    dev = torch.from_numpy(host.copy()).cuda()
    stream, crc, nbytes = d.raw_deflate(dev, elem, codes)
    stats = {}
    out = d.inflate(stream[:-2], nbytes, stats=stats)
    assert out is not None and out.is_cuda and out.dtype == torch.uint8 and out.numel() == host.size
    assert out.cpu().numpy().tobytes() == host.tobytes()
    assert stats["records"] == -(-host.size // CHUNK) and stats["records"] <= stats["candidates"] <= d.candidate_cap(host.size)
    assert d.device_crc32(out) == crc == zlib.crc32(host.tobytes())
    return stream[:-2], stats


@pytest.mark.parametrize("codes", CODES)
@pytest.mark.parametrize("elem", [1, 2, 4, 8])
def test_round_trip_at_every_size(elem, codes):
    value = bytes([0x00, 0x3C, 0x81, 0x7F, 0x01, 0x02, 0x90, 0xFF][:elem])
    for size in SIZES:
        n = size // elem * elem
        _round_trip(np.frombuffer(value * (n // elem), dtype=np.uint8), elem, codes)
        _round_trip(_mixed(n, 300 + size), elem, codes)
        _round_trip(np.random.default_rng(size).integers(0, 256, n, dtype=np.uint8), elem, codes)


def _device_scan(body, starts):
    from e2enet_medical_amd._lib import lib
    comp = torch.from_numpy(np.frombuffer(body, dtype=np.uint8).copy()).cuda()
    starts_d = torch.tensor([int(s) for s in starts], dtype=torch.int64, device="cuda")
    records = torch.full((len(starts), 8), -1, dtype=torch.int32, device="cuda")
    lib().inflate_scan(comp.data_ptr(), comp.numel(), starts_d.data_ptr(), len(starts), records.data_ptr(),
                       torch.cuda.current_stream().cuda_stream)
    return records.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("codes", CODES)
@pytest.mark.parametrize("case", ["a_constant", "b_run_across", "c_abcx", "d_stored_then_constant", "e_high_bytes_distance_8",
                                  "f_fibonacci"])
def test_scan_records_equal_the_oracle(case, codes):
    """the named cases through the real kernels; every candidate's record, the false ones included, word for word"""
    d = _deflate()
    data, elem = named_inputs()[case]
    body, _ = _round_trip(data, elem, codes)
    starts = d.candidate_starts(body, data.size)
    extra = [1, 2, 3, len(body) - 1, len(body), len(body) + 7, -1]              # no record starts here; two lie outside the stream
    got = _device_scan(body, list(starts) + extra)
    want = oracle.scan(body, starts)
    assert np.array_equal(got[:len(starts)], want)
    kinds = {int(w[1]) & 0xFF for w in want if w[0] == 0}
    if case == "d_stored_then_constant":
        assert d.STORED in kinds and len(kinds) >= 2
    if case == "f_fibonacci" and codes == "dynamic":
        assert kinds == {d.DYNAMIC}
    for s, words in zip(extra, got[len(starts):]):
        assert list(words) == oracle.record_words(body, s) if 0 <= s < len(body) else list(words) == [1, 0, 0, 0, 0, 0, 0, 0]


def _chunks(body, starts, tails, nbytes, slack=4096):
    """``e2e_inflate_chunks`` into the middle of a buffer of 0xA5: (the buffer, the status word)"""
    from e2enet_medical_amd._lib import lib
    comp = torch.from_numpy(np.frombuffer(body, dtype=np.uint8).copy()).cuda()
    buf = torch.full((slack + nbytes + slack,), 0xA5, dtype=torch.uint8, device="cuda")
    status = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    starts_d, tails_d = torch.from_numpy(np.ascontiguousarray(starts)).cuda(), torch.from_numpy(np.ascontiguousarray(tails)).cuda()
    lib().inflate_chunks(comp.data_ptr(), comp.numel(), starts_d.data_ptr(), tails_d.data_ptr(), len(starts),
                         buf[slack:].data_ptr(), nbytes, status.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return buf.cpu().numpy(), int(status.item())


@pytest.mark.parametrize("codes", CODES)
def test_false_candidates_and_corrupt_records_leave_the_output_untouched(codes):
    """the writing pass trusts nothing: a record that is invalid, starts at a false candidate or gives another length than its place
    in the output takes, is counted and writes nothing; the records beside it are written, and nothing outside [0, nbytes)"""
    d = _deflate()
    data = np.concatenate([_mixed(2 * CHUNK, 5), np.random.default_rng(1).integers(0, 256, CHUNK, dtype=np.uint8), _mixed(1000, 6)])
    dev = torch.from_numpy(data.copy()).cuda()
    body = d.raw_deflate(dev, 1, codes)[0][:-2]
    starts, tails, _ = d.inflate_plan(body, data.size, oracle.scan)
    slack = 4096
    buf, status = _chunks(body, starts, tails, data.size, slack)
    assert status == 0 and buf[slack:slack + data.size].tobytes() == data.tobytes()
    assert (buf[:slack] == 0xA5).all() and (buf[slack + data.size:] == 0xA5).all()
    inside = int(starts[2]) + 5 + 1000                      # a false candidate inside the stored record
    for k, bad in ((1, int(starts[1]) + 1), (2, inside), (0, int(starts[3])), (3, int(starts[0])), (1, len(body) + 5), (2, -8)):
        moved = starts.copy()
        moved[k] = bad
        buf, status = _chunks(body, moved, tails, data.size, slack)
        assert status == 1, (k, bad)
        lo, hi = slack + k * CHUNK, slack + min((k + 1) * CHUNK, data.size)
        assert (buf[lo:hi] == 0xA5).all() and (buf[:slack] == 0xA5).all() and (buf[slack + data.size:] == 0xA5).all()
        assert buf[slack:lo].tobytes() == data[:k * CHUNK].tobytes() and buf[hi:slack + data.size].tobytes() == data[(k + 1) * CHUNK:].tobytes()
    damaged = bytearray(body)
    assert damaged[int(starts[1])] & 7 in (2, 4)
    damaged[int(starts[1])] |= 1                             # BFINAL inside the chain
    buf, status = _chunks(bytes(damaged), starts, tails, data.size, slack)
    assert status == 1 and (buf[slack + CHUNK:slack + 2 * CHUNK] == 0xA5).all()
    with pytest.raises(ValueError, match="1 of 4 records are corrupt"):      # through the package, after a scan that saw other bytes
        d.inflate(bytes(damaged), data.size, scan=lambda _, c: oracle.scan(body, c))
    assert d.inflate(bytes(damaged), data.size) is None                      # the device's own scan breaks the chain there


def test_markers_in_stored_chunks_go_to_the_host_and_dynamic_ones_do_not():
    """cases g and g'"""
    d = _deflate()
    data = _zero_minus_one()
    dev = torch.from_numpy(data.copy()).cuda()
    stream = d.raw_deflate(dev, 2, "fixed")[0]
    assert d.inflate(stream[:-2], data.size) is None and zlib.decompress(stream, -15) == data.tobytes()
    _, stats = _round_trip(data, 2, "dynamic")
    assert stats["candidates"] <= 8


def test_foreign_streams_are_none():
    d = _deflate()
    data = _mixed(2 * CHUNK + 100, 8).tobytes()
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    s = c.compress(data) + c.flush()
    assert d.inflate(s, len(data)) is None and d.inflate(s[:-2], len(data)) is None
    ours = d.raw_deflate(torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda(), 1, "dynamic")[0]
    assert d.inflate(ours, len(data)) is None                           # (with the closing 03 00: not the device part)
    assert d.inflate(ours[:-3], len(data)) is None and d.inflate(ours[:-2], len(data) + 1) is None


# ----------------------------------------------------------------------------------------------------------------------- npz
@pytest.mark.parametrize("codes", CODES)
def test_savez_then_load_npz(tmp_path, codes):
    d = _deflate()
    rng = np.random.default_rng(12)
    arrays = OrderedDict(softmax=np.round(rng.random((3, 7, 33, 65)), 2).astype(np.float16),
                         values=np.round(rng.normal(0, 1, (3, 20000)), 1).astype(np.float32),
                         labels=np.repeat(rng.integers(0, 3, 900, dtype=np.uint8), 41).reshape(9, 41, 100),
                         empty=np.zeros((0, 5), dtype=np.float16))
    path = str(tmp_path / "four.npz")
    d.savez(path, codes=codes, **{k: torch.from_numpy(v).cuda() for k, v in arrays.items()})
    stats = {}
    got = d.load_npz(path, stats=stats)
    assert list(got) == list(arrays)
    with np.load(path) as want:
        for key, a in arrays.items():
            t = got[key]
            assert t.is_cuda and t.shape == a.shape and t.cpu().numpy().dtype == a.dtype
            assert t.cpu().numpy().tobytes() == a.tobytes() == want[key].tobytes(), key
            assert stats[key]["route"] == "device" and stats[key]["records"] == -(-a.nbytes // CHUNK)
    np.savez_compressed(str(tmp_path / "host.npz"), **arrays)             # zlib's own members: np.load and an upload
    stats = {}
    got = d.load_npz(str(tmp_path / "host.npz"), keys=("labels", "softmax"), stats=stats)
    assert list(got) == ["labels", "softmax"] and all(v["route"] == "host" for v in stats.values())
    assert got["softmax"].is_cuda and got["softmax"].cpu().numpy().tobytes() == arrays["softmax"].tobytes()
    blob = bytearray(open(path, "rb").read())                              # a damaged payload is refused by name
    raw = d.read_npz_raw(path)
    m = raw.members["values"]
    at = int(m.body.__array_interface__["data"][0] - raw.data.__array_interface__["data"][0]) + len(m.body) // 2
    blob[at] ^= 0x01
    open(str(tmp_path / "bad.npz"), "wb").write(bytes(blob))
    # refused either way: by name where the chain still stands (a stored record: the CRC), by np.load where it broke
    with pytest.raises((ValueError, zlib.error, zipfile.BadZipFile)) as e:
        d.load_npz(str(tmp_path / "bad.npz"), keys=("values",))
    if e.type is ValueError:
        assert "bad.npz: member values" in str(e.value)


def test_ensemble_merge_with_device_inflate_writes_the_same_files(tmp_path):
    from e2enet_medical_amd import nifti
    from e2enet_medical_amd.inference.ensemble_predictions import merge, merge_files
    from e2enet_medical_amd.inference.predict import save_softmax_npz
    rng = np.random.default_rng(9)
    shape = (3, 12, 40, 40)
    props = {"itk_spacing": (1., 1., 2.), "itk_origin": (0., 0., 0.), "itk_direction": (1., 0., 0., 0., 1., 0., 0., 0., 1.),
             "size_after_cropping": shape[1:], "original_size_of_raw_data": np.array(shape[1:]),
             "crop_bbox": [[0, shape[1]], [0, shape[2]], [0, shape[3]]]}
    folders = [str(tmp_path / "f0"), str(tmp_path / "f1")]
    for fi, folder in enumerate(folders):
        os.makedirs(folder)
        for case in ("case0", "case1"):
            logits = rng.normal(0, 3, shape).astype(np.float32)
            logits[:, :, :15] = 0
            soft = torch.softmax(torch.from_numpy(logits), 0).to(torch.float16).cuda().contiguous()
            # one folder by the device encoder (a code per folder), one case of the other by host zlib: both routes in one merge
            save_softmax_npz(soft, os.path.join(folder, case + ".npz"), dict(props, name=case),
                             device_deflate=(False if (fi, case) == (1, "case1") else ("dynamic" if fi else True)))
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    merge(folders, a, 2, writer=nifti.writer, store_npz=True)
    merge(folders, b, 2, writer=nifti.writer, store_npz=True, device_inflate=True)
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and "case0.nii.gz" in names and "case1.npz" in names
    for name in names:
        if name.endswith(".npz"):                   # (np.savez_compressed stamps the time of day into the archive)
            assert np.load(os.path.join(a, name))["softmax"].tobytes() == np.load(os.path.join(b, name))["softmax"].tobytes()
        else:
            assert open(os.path.join(a, name), "rb").read() == open(os.path.join(b, name), "rb").read(), name
    one = str(tmp_path / "one.nii.gz")
    merge_files([os.path.join(f, "case0.npz") for f in folders], [os.path.join(f, "case0.pkl") for f in folders], one, True, False,
                writer=nifti.writer, device_inflate=True)
    assert open(one, "rb").read() == open(os.path.join(a, "case0.nii.gz"), "rb").read()


def test_resident_loader_with_device_inflate_equals_the_host_loader(tmp_path):
    from e2enet_medical_amd.training.dataloading.dataset_loading import DataLoader3D
    from e2enet_medical_amd.training.dataloading.resident_loading import DeviceCaseCache, ResidentDataLoader3D
    d = _deflate()
    ds = OrderedDict()
    for ci, name in enumerate(("case_a", "case_b")):
        shp = (24, 40, 40)
        j = np.arange(int(np.prod(shp)), dtype=np.float64).reshape(shp)
        zz, yy, xx = np.meshgrid(*[np.arange(s) for s in shp], indexing="ij")
        seg = np.minimum(((zz * 3 + yy * 5 + xx * 7 + ci) % 11 < 2).astype(np.float32) + ((zz + yy + xx) % 13 == 0) * 2.0, 2.0)
        arr = np.stack([np.sin(0.37 * j + ci).astype(np.float32) * (zz > 4), seg]).astype(np.float32)
        path = os.path.join(str(tmp_path), name + ".npz")
        d.savez(path, codes="dynamic" if ci else "fixed", data=torch.from_numpy(arr).cuda())      # packed only: no .npy
        locs = OrderedDict((c, np.argwhere(seg == c)) for c in (1, 2))
        ds[name] = OrderedDict(data_file=path, properties=OrderedDict(class_locations=locs, name=name))
    args = (ds, (16, 18, 20), (12, 14, 16), 4, False)
    kw = dict(oversample_foreground_percent=0.33, pad_mode="constant", pad_kwargs_data={'constant_values': 0})
    np.random.seed(77)
    host = DataLoader3D(*args, **kw)
    want = [next(host) for _ in range(2)]
    want = [{k: (np.array(b[k]) if k in ("data", "seg") else b[k]) for k in b} for b in want]
    cache = DeviceCaseCache(None, "cuda", device_inflate=True)
    np.random.seed(77)
    loader = ResidentDataLoader3D(*args, cache=cache, **kw)
    for w in want:
        b = next(loader)
        assert [str(k) for k in b['keys']] == [str(k) for k in w['keys']]
        assert np.array_equal(b['data'].cpu().numpy(), w['data']) and np.array_equal(b['seg'].cpu().numpy(), w['seg'].astype(np.float32))
    assert cache.inflated_cases == len(cache) == 2 and loader.staged_samples == 0
    for name in ds:
        assert cache.fetch(ds[name])[0].cpu().numpy().tobytes() == np.load(ds[name]['data_file'])['data'].tobytes()


# -------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(tmp_path, capsys):
    from e2enet_medical_amd._lib import lib, E2EError
    from e2enet_medical_amd import simple_main
    from e2enet_medical_amd.training.network_training.nnUNetTrainer_simple import nnUNetTrainer_simple
    d = _deflate()
    L, st = lib(), torch.cuda.current_stream().cuda_stream
    x = torch.zeros(64, dtype=torch.uint8, device="cuda")
    w = torch.zeros(16, dtype=torch.int64, device="cuda")
    with pytest.raises(E2EError, match="null"):
        L.inflate_scan(x.data_ptr(), 64, None, 1, w.data_ptr(), st)
    with pytest.raises(E2EError, match="candidates"):
        L.inflate_scan(x.data_ptr(), 64, w.data_ptr(), -1, w.data_ptr(), st)
    with pytest.raises(E2EError, match="records for"):
        L.inflate_chunks(x.data_ptr(), 64, w.data_ptr(), x.data_ptr(), 2, x.data_ptr(), 10, w.data_ptr(), st)
    with pytest.raises(E2EError, match="null"):
        L.inflate_chunks(x.data_ptr(), 64, w.data_ptr(), x.data_ptr(), 1, None, 10, w.data_ptr(), st)
    with pytest.raises(E2EError, match="null"):
        L.inflate_chunks(x.data_ptr(), 64, w.data_ptr(), x.data_ptr(), 1, x.data_ptr(), 10, None, st)
    with pytest.raises(E2EError, match="aligned to 16"):
        L.inflate_chunks(x.data_ptr(), 64, w.data_ptr(), x.data_ptr(), 1, x.data_ptr() + 8, 10, w.data_ptr(), st)
    with pytest.raises(E2EError, match="null"):
        L.crc32(x.data_ptr(), 64, None, w.data_ptr(), st)
    with pytest.raises(E2EError, match="bytes"):
        L.crc32(x.data_ptr(), -1, w.data_ptr(), w.data_ptr(), st)
    assert d.device_crc32(x[:0]) == 0 and d.device_crc32(x) == zlib.crc32(bytes(64))
    with pytest.raises(ValueError, match="device tensor"):
        d.device_crc32(x.cpu())
    with pytest.raises(ValueError, match="uint8"):
        d.inflate(np.zeros(4, dtype=np.int32), 16)
    assert d.inflate(b"", 0).numel() == 0 and d.inflate(b"", 5) is None and d.inflate(b"\x00", 0) is None
    with pytest.raises(SystemExit):
        simple_main.main(["--device_inflate"])
    assert "--device_inflate needs --resident_data" in capsys.readouterr().err
    tr = nnUNetTrainer_simple.__new__(nnUNetTrainer_simple)
    tr.device_inflate, tr.resident_data_gib, tr.load_dataset, tr.do_split = True, None, lambda: None, lambda: None
    with pytest.raises(ValueError, match="--device_inflate"):
        tr.get_basic_generators()
