"""The device inflater for any DEFLATE stream (csrc/inflate_any.hip; ``deflate.inflate_any``) on zlib's own streams: the five
kernels against tests/inflate_any_oracle.py word for word, round trips against ``zlib.decompress``, corrupt streams, the refusals of
the C ABI, and the containers (``load_npz(foreign="device")``, ``nifti.read_raw(inflate="device")``, the ensemble merge and the
resident loader with ``device_inflate="any"``) against their default routes.  Every comparison is for exact bytes.  The inputs are
those of tests/test_inflate_any_cpu.py, which shows on the CPU that they hold no false block start."""
import gzip
import os
import zlib

import numpy as np
import pytest
import torch

from tests import inflate_any_oracle as oracle
from collections import OrderedDict

from tests.test_inflate_any_cpu import CASES, NONE_INPUTS, ct_like, inputs, label_runs, nii_gz_bytes, nii_volume, stages

pytestmark = pytest.mark.gpu

W = oracle.W


def _lib():
    from e2enet_medical_amd._lib import lib
    return lib()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _comp(stream):
    return torch.from_numpy(np.frombuffer(bytes(stream) or b"\x00", dtype=np.uint8).copy()).cuda()[:len(stream)]


def device_find(stream, S):
    comp = _comp(stream)
    nseg = -(-len(stream) // S)
    starts = torch.full((max(nseg, 1),), -7, dtype=torch.int64, device="cuda")
    _lib().inflate_find(comp.data_ptr(), len(stream), S, nseg, starts.data_ptr(), _st())
    return starts.cpu().numpy()


def device_count(stream, starts, cap):
    comp = _comp(stream)
    starts_d = torch.from_numpy(np.ascontiguousarray(starts, dtype=np.int64)).cuda()
    records = torch.full((len(starts), 8), -1, dtype=torch.int32, device="cuda")
    _lib().inflate_spans_count(comp.data_ptr(), len(stream), starts_d.data_ptr(), len(starts), cap, records.data_ptr(), _st())
    return records.cpu().numpy().view(np.uint32)


def device_write(stream, starts, offs, cap, slack=64):
    """``e2e_inflate_spans_write`` into the middle of a buffer of 0xFFFF: (the buffer, the status word)"""
    comp = _comp(stream)
    total = int(offs[-1])
    starts_d = torch.from_numpy(np.ascontiguousarray(starts, dtype=np.int64)).cuda()
    offs_d = torch.from_numpy(np.ascontiguousarray(offs, dtype=np.int64)).cuda()
    buf = torch.full((slack + total + slack,), -1, dtype=torch.int16, device="cuda")
    status = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    _lib().inflate_spans_write(comp.data_ptr(), len(stream), starts_d.data_ptr(), offs_d.data_ptr(), len(starts), cap,
                               buf[slack:].data_ptr(), total, status.data_ptr(), _st())
    return buf.cpu().numpy().view(np.uint16), int(status.item())


def device_windows(sym, offs):
    m, total = len(offs) - 1, int(offs[-1])
    sym_d = torch.from_numpy(np.ascontiguousarray(sym).view(np.int16)).cuda()
    offs_d = torch.from_numpy(np.ascontiguousarray(offs, dtype=np.int64)).cuda()
    wins = torch.zeros((m, W), dtype=torch.uint8, device="cuda")
    status = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    _lib().inflate_windows(sym_d.data_ptr(), offs_d.data_ptr(), m, total, wins.data_ptr(), status.data_ptr(), _st())
    return wins.cpu().numpy(), int(status.item())


def device_resolve(sym, offs, wins, slack=64):
    m, total = len(offs) - 1, int(offs[-1])
    sym_d = torch.from_numpy(np.ascontiguousarray(sym).view(np.int16)).cuda()
    offs_d = torch.from_numpy(np.ascontiguousarray(offs, dtype=np.int64)).cuda()
    wins_d = torch.from_numpy(np.ascontiguousarray(wins)).cuda()
    buf = torch.full((slack + total + slack,), 0xA5, dtype=torch.uint8, device="cuda")
    status = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    _lib().inflate_resolve(sym_d.data_ptr(), offs_d.data_ptr(), m, wins_d.data_ptr(), buf[slack:].data_ptr(), total, status.data_ptr(), _st())
    return buf.cpu().numpy(), int(status.item())


@pytest.mark.parametrize("name,S", CASES)
def test_find_equals_the_oracle_and_the_true_block_starts(name, S):
    """word for word; tests/test_inflate_any_cpu.py shows the oracle's starts to be the true ones, first per segment"""
    raw, stream, _ = inputs()[name]
    got = device_find(stream, S)
    assert got[0] == -7                                 # entry 0 is the host's
    got[0] = 0
    assert np.array_equal(got, oracle.find(stream, S))


@pytest.mark.parametrize("name,S", CASES)
def test_every_kernel_and_the_round_trip(name, S):
    """count, write, windows and resolve against the oracle, stage by stage on the oracle's input of the stage, then the whole of
    ``inflate_any`` against zlib, with its CRC-32"""
    from e2enet_medical_amd import deflate
    raw, stream, _ = inputs()[name]
    want = stages(name, S)
    stats = {}
    out = deflate.inflate_any(stream, len(raw), segment_bytes=S, stats=stats)
    if name in NONE_INPUTS:
        assert want is None and out is None and "gap" in stats["refused"]
        return
    assert out is not None and out.is_cuda and out.dtype == torch.uint8
    assert out.cpu().numpy().tobytes() == raw == zlib.decompress(stream, -15)
    assert deflate.device_crc32(out) == zlib.crc32(raw)
    assert stats["spans"] == len(want["starts"]) and stats["refused"] is None
    assert stats["largest_gap"] == oracle.largest_gap(want["starts"], len(stream))
    starts, offs = want["starts"], want["offs"]
    assert np.array_equal(device_count(stream, starts, 8 * S), want["records"])
    slack = 64
    sym, status = device_write(stream, starts, offs, 8 * S, slack)
    assert status == 0 and np.array_equal(sym[slack:slack + len(raw)], want["sym"])
    assert (sym[:slack] == 0xFFFF).all() and (sym[slack + len(raw):] == 0xFFFF).all()
    wins, status = device_windows(want["sym"], offs)
    assert status == 0 and np.array_equal(wins[1:], want["wins"][1:])
    buf, status = device_resolve(want["sym"], offs, want["wins"], slack)
    assert status == 0 and buf[slack:slack + len(raw)].tobytes() == raw
    assert (buf[:slack] == 0xA5).all() and (buf[slack + len(raw):] == 0xA5).all()


def test_a_device_stream_is_used_as_it_is():
    from e2enet_medical_amd import deflate
    raw, stream, _ = inputs()["a_ct_15000_level6"]
    padded = _comp(b"\x00\x00\x00" + stream)           # an odd address
    out = deflate.inflate_any(padded[3:], len(raw), segment_bytes=256)
    assert out.cpu().numpy().tobytes() == raw


def test_false_starts_give_statuses_and_no_output():
    """starts injected at positions that are no block start: the count records equal the oracle's field for field, the span in
    front of a false start overshoots, ``inflate_any`` says None, and the writing pass keeps a bad span inside its own range of the symbols"""
    from e2enet_medical_amd import deflate
    raw, stream, _ = inputs()["a_ct_15000_level6"]
    S = 256
    want = stages("a_ct_15000_level6", S)
    starts = want["starts"]
    seen = set()
    for k, shift in ((3, 5), (7, -9), (10, 1), (20, 64), (len(starts) - 1, 3)):
        moved = starts.copy()
        moved[k] += shift
        got, ref = device_count(stream, moved, 8 * S), oracle.count(stream, moved, 8 * S)
        assert np.array_equal(got, ref)
        assert ref[k - 1, 0] == oracle.OVERSHOOT or shift < 0
        assert ref[k, 0] != 0 and not ref[k, 1:].any()
        seen |= set(ref[:, 0].tolist())
        stats = {}
        hook = lambda data, seg, moved=moved: moved.copy()      # (inflate_any only compacts what find returns)
        assert deflate.inflate_any(stream, len(raw), segment_bytes=S, stats=stats, find=hook) is None and "span" in stats["refused"]
        # the same starts in the writing pass: the spans around the false start are counted and store nothing outside their own
        # ranges, the rest is written, nothing outside the buffer
        slack = 64
        sym, status = device_write(stream, moved, want["offs"], 8 * S, slack)
        bad = [j for j in range(len(starts)) if ref[j, 0] != 0]
        assert status == len(bad)
        good = np.ones(len(raw), dtype=bool)           # (a bad span may have stored symbols before it failed, inside its own range)
        for j in bad:
            good[int(want["offs"][j]):int(want["offs"][j + 1])] = False
        assert np.array_equal(sym[slack:slack + len(raw)][good], want["sym"][good])
        assert (sym[:slack] == 0xFFFF).all() and (sym[slack + len(raw):] == 0xFFFF).all()
    assert oracle.OVERSHOOT in seen and len(seen) >= 3
    # starts outside the stream, a cap that is too small, offsets that lie
    odd = np.asarray([0, 8 * len(stream), 8 * len(stream) + 77, -5], dtype=np.int64)
    assert np.array_equal(device_count(stream, odd, 8 * S), oracle.count(stream, odd, 8 * S))
    assert np.array_equal(device_count(stream, starts, 16), oracle.count(stream, starts, 16))
    lying = want["offs"].copy()
    lying[5] += 1
    sym, status = device_write(stream, starts, lying, 8 * S)
    assert status == 2
    wild = want["offs"].copy()
    wild[3] = -40
    wild[9] = int(wild[-1]) + 1000
    sym, status = device_write(stream, starts, wild, 8 * S)
    assert status >= 2 and (sym[:64] == 0xFFFF).all() and (sym[64 + len(raw):] == 0xFFFF).all()


def test_markers_in_span_zero_are_a_status():
    offs = np.asarray([0, 40000, 80000], dtype=np.int64)
    sym = np.zeros(80000, dtype=np.uint16)
    sym[39990] = 0x8000 | 5
    wins, status = device_windows(sym, offs)
    assert status >= 1
    buf, status = device_resolve(sym, offs, np.zeros((2, W), dtype=np.uint8))
    assert status >= 1


def test_a_flipped_bit_never_returns_wrong_bytes(tmp_path):
    from e2enet_medical_amd import deflate
    raw, stream, _ = inputs()["a_ct_15000_level6"]
    for at, bit in ((len(stream) // 2, 0), (len(stream) // 2, 5), (len(stream) // 2 + 1, 7), (len(stream) // 3, 2)):
        bad = bytearray(stream)
        bad[at] ^= 1 << bit
        try:
            got = deflate.inflate_any(bytes(bad), len(raw), segment_bytes=256)
        except ValueError:
            continue
        if got is not None:
            assert got.cpu().numpy().tobytes() == zlib.decompress(bytes(bad), -15)
    # the same in a container: load_npz raises, or takes the host route and gives the host route's own error
    path = str(tmp_path / "case.npz")
    np.savez_compressed(path, data=np.frombuffer(ct_like(60000, 50), dtype=np.int16))
    blob = bytearray(open(path, "rb").read())
    blob[len(blob) // 2] ^= 0x10
    open(path, "wb").write(bytes(blob))
    try:
        host = np.load(path)["data"]
    except Exception as e:
        host = type(e)
    try:
        got = deflate.load_npz(path, foreign="device")["data"].cpu().numpy()
        assert not isinstance(host, type) and np.array_equal(got, host)
    except Exception as e:
        assert isinstance(e, ValueError) or isinstance(e, host)


def test_savez_compressed_members_take_the_new_route(tmp_path):
    from e2enet_medical_amd import deflate
    rng = np.random.default_rng(0)
    arrays = {"data": np.frombuffer(ct_like(3 * 40 * 50 * 60, 41), dtype=np.int16).reshape(3, 40, 50, 60).copy(),
              "softmax": rng.random((4, 20, 30, 30)).astype(np.float16),
              "labels": np.frombuffer(label_runs(50000, 3), dtype=np.uint8).reshape(50, 1000).copy(),
              "odd": np.arange(7, dtype=np.float64), "empty": np.zeros((0, 3), dtype=np.float32),
              "fortran": np.asfortranarray(np.arange(24, dtype=np.float32).reshape(4, 6))}
    path = str(tmp_path / "case.npz")
    np.savez_compressed(path, **arrays)
    stats = {}
    got = deflate.load_npz(path, stats=stats, foreign="device")
    ref = np.load(path)
    for key in ref.files:
        assert got[key].is_cuda and tuple(got[key].shape) == ref[key].shape
        assert got[key].cpu().numpy().dtype == ref[key].dtype and np.array_equal(got[key].cpu().numpy(), ref[key]), key
    for key in ("data", "labels", "odd", "empty"):
        assert stats[key]["route"] == "any" and stats[key]["any"]["refused"] is None, (key, stats[key])
    assert stats["fortran"]["route"] == "host"
    default = deflate.load_npz(path, stats=stats)
    assert all(stats[k]["route"] == "host" for k in ref.files) and all(torch.equal(default[k], got[k]) for k in ref.files)


def test_the_abi_refuses_before_any_launch():
    from e2enet_medical_amd._lib import E2EError
    L, st = _lib(), _st()
    comp = _comp(inputs()["a_ct_15000_level6"][1])
    n = comp.numel()
    i64 = torch.zeros(64, dtype=torch.int64, device="cuda")
    i32 = torch.zeros(64, dtype=torch.int32, device="cuda")
    i16 = torch.zeros(64, dtype=torch.int16, device="cuda")
    u8 = torch.zeros(W * 2 + 64, dtype=torch.uint8, device="cuda")
    calls = [
        lambda: L.inflate_find(comp.data_ptr(), n, 8, -(-n // 8), i64.data_ptr(), st),                  # S < 16
        lambda: L.inflate_find(comp.data_ptr(), n, 4096, 2, i64.data_ptr(), st),                        # not ceil(n / S) segments
        lambda: L.inflate_find(None, n, 4096, -(-n // 4096), i64.data_ptr(), st),
        lambda: L.inflate_find(comp.data_ptr(), n, 4096, -(-n // 4096), None, st),
        lambda: L.inflate_find(comp.data_ptr(), (1 << 38) + 1, 1 << 24, -(-((1 << 38) + 1) // (1 << 24)), i64.data_ptr(), st),
        lambda: L.inflate_spans_count(comp.data_ptr(), n, None, 2, 4096, i32.data_ptr(), st),
        lambda: L.inflate_spans_count(comp.data_ptr(), n, i64.data_ptr(), (1 << 26) + 1, 4096, i32.data_ptr(), st),
        lambda: L.inflate_spans_count(comp.data_ptr(), n, i64.data_ptr(), 2, 0, i32.data_ptr(), st),
        lambda: L.inflate_spans_write(comp.data_ptr(), n, i64.data_ptr(), i64.data_ptr(), 2, 4096, i16.data_ptr() + 2, 8, i32.data_ptr(), st),
        lambda: L.inflate_spans_write(comp.data_ptr(), n, i64.data_ptr(), None, 2, 4096, i16.data_ptr(), 8, i32.data_ptr(), st),
        lambda: L.inflate_spans_write(comp.data_ptr(), n, i64.data_ptr(), i64.data_ptr(), 2, 4096, i16.data_ptr(), 8, None, st),
        lambda: L.inflate_windows(i16.data_ptr(), i64.data_ptr(), 2, 8, None, i32.data_ptr(), st),
        lambda: L.inflate_windows(i16.data_ptr(), i64.data_ptr(), (1 << 26) + 1, 8, u8.data_ptr(), i32.data_ptr(), st),
        lambda: L.inflate_resolve(i16.data_ptr(), i64.data_ptr(), 2, u8.data_ptr(), u8.data_ptr() + 1, 8, i32.data_ptr(), st),
        lambda: L.inflate_resolve(i16.data_ptr() + 2, i64.data_ptr(), 2, u8.data_ptr(), u8.data_ptr(), 8, i32.data_ptr(), st),
        lambda: L.inflate_resolve(i16.data_ptr(), i64.data_ptr(), 2, None, u8.data_ptr(), 8, i32.data_ptr(), st),
        lambda: L.inflate_resolve(i16.data_ptr(), i64.data_ptr(), 2, u8.data_ptr(), u8.data_ptr(), (1 << 37) + 1, i32.data_ptr(), st),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(E2EError):
            call()
            pytest.fail("call %d was not refused" % i)
    torch.cuda.synchronize()
    assert not i64.any() and not i32.any() and not i16.any() and not u8.any()


# --------------------------------------------------------------------------------------------------------------------- .nii.gz
@pytest.mark.parametrize("extras", [False, True])
def test_nii_gz_through_the_device_equals_the_host_route(tmp_path, extras):
    """24 x 40 x 48: an int16 image and a uint8 label file, plain gzip and a member header with FEXTRA / FNAME / FCOMMENT / FHCRC;
    decode_f32, decode_u8 and scan bit for bit"""
    from e2enet_medical_amd import nifti
    for kind in ("image", "labels"):
        vol, datatype = nii_volume(kind)
        path = str(tmp_path / ("%s.nii.gz" % kind))
        fields = dict(scl_slope=0.5, scl_inter=-7.0) if kind == "image" else {}
        open(path, "wb").write(nii_gz_bytes(vol, datatype, extras, **fields))
        host, dev = nifti.read_raw(path), nifti.read_raw(path, inflate="device")
        assert isinstance(dev.payload, nifti.DeferredPayload)
        assert nifti.resolve_payload(dev).cpu().numpy().tobytes() == vol.tobytes()
        assert torch.equal(nifti.decode_f32(dev), nifti.decode_f32(host))
        a, b = nifti.scan(dev), nifti.scan(host)
        assert a[:4] == b[:4] and np.array_equal(a.histogram, b.histogram)
        if kind == "labels":
            assert torch.equal(nifti.decode_u8(dev), nifti.decode_u8(host))
            cb = nifti.callbacks("device")
            assert np.array_equal(cb.gt_reader(path), nifti.gt_reader(path))
        else:
            data, props = nifti.callbacks("device").reader([path, path])
            want, wprops = nifti.reader([path, path])
            assert torch.equal(data, want) and list(props) == list(wprops)
    # a damaged payload: a ValueError that names the file (the CRC on the device, a corrupt span), or whatever the host route makes of
    # the file -- which reads no further than the voxels and so may not notice
    blob = bytearray(open(path, "rb").read())
    blob[len(blob) // 2] ^= 0x04
    bad = str(tmp_path / "bad.nii.gz")
    open(bad, "wb").write(bytes(blob))
    try:
        host = nifti.decode_u8(nifti.read_raw(bad)).cpu().numpy()
    except Exception as ex:
        host = type(ex)
    try:
        got = nifti.decode_u8(nifti.read_raw(bad, inflate="device")).cpu().numpy()
    except Exception as ex:
        assert (isinstance(ex, ValueError) and "bad.nii.gz" in str(ex)) or (isinstance(host, type) and isinstance(ex, host)), repr(ex)
    else:
        assert not isinstance(host, type) and np.array_equal(got, host)


def test_nii_gz_the_device_route_does_not_serve(tmp_path):
    from e2enet_medical_amd import nifti
    vol, datatype = nii_volume("labels")
    blob = nii_gz_bytes(vol, datatype)
    two = str(tmp_path / "two.nii.gz")
    open(two, "wb").write(blob + gzip.compress(b"behind", mtime=0))
    assert torch.equal(nifti.decode_u8(nifti.read_raw(two, inflate="device")), nifti.decode_u8(nifti.read_raw(two)))
    cut = str(tmp_path / "cut.nii.gz")
    open(cut, "wb").write(blob[:349])
    with pytest.raises(Exception) as h:
        nifti.read_raw(cut)
    with pytest.raises(h.type):
        nifti.read_raw(cut, inflate="device")


# ------------------------------------------------------------------------------------------------------ ensemble, resident data
def test_ensemble_merge_of_zlib_written_folders(tmp_path):
    from e2enet_medical_amd import deflate, nifti
    from e2enet_medical_amd.inference.ensemble_predictions import merge, merge_files
    from e2enet_medical_amd.inference.predict import save_softmax_npz
    rng = np.random.default_rng(9)
    shape = (3, 12, 40, 40)
    props = {"itk_spacing": (1., 1., 2.), "itk_origin": (0., 0., 0.), "itk_direction": (1., 0., 0., 0., 1., 0., 0., 0., 1.),
             "size_after_cropping": shape[1:], "original_size_of_raw_data": np.array(shape[1:]),
             "crop_bbox": [[0, shape[1]], [0, shape[2]], [0, shape[3]]]}
    folders = [str(tmp_path / "f0"), str(tmp_path / "f1")]
    for folder in folders:
        os.makedirs(folder)
        for case in ("case0", "case1"):
            logits = rng.normal(0, 3, shape).astype(np.float32)
            logits[:, :, :15] = 0
            soft = torch.softmax(torch.from_numpy(logits), 0).to(torch.float16).cuda().contiguous()
            save_softmax_npz(soft, os.path.join(folder, case + ".npz"), dict(props, name=case))       # np.savez_compressed
    stats = {}
    deflate.load_npz(os.path.join(folders[0], "case0.npz"), stats=stats, foreign="device")
    assert stats["softmax"]["route"] == "any"
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    merge(folders, a, 2, writer=nifti.writer)
    merge(folders, b, 2, writer=nifti.writer, device_inflate="any")
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and "case0.nii.gz" in names
    for name in names:
        assert open(os.path.join(a, name), "rb").read() == open(os.path.join(b, name), "rb").read(), name
    one = str(tmp_path / "one.nii.gz")
    merge_files([os.path.join(f, "case0.npz") for f in folders], [os.path.join(f, "case0.pkl") for f in folders], one, True, False,
                writer=nifti.writer, device_inflate="any")
    assert open(one, "rb").read() == open(os.path.join(a, "case0.nii.gz"), "rb").read()
    with pytest.raises(ValueError):
        merge(folders, str(tmp_path / "c"), 2, writer=nifti.writer, device_inflate="all")


def test_resident_loader_on_a_zlib_written_stage_case(tmp_path):
    from e2enet_medical_amd.training.dataloading.dataset_loading import DataLoader3D
    from e2enet_medical_amd.training.dataloading.resident_loading import DeviceCaseCache, ResidentDataLoader3D
    ds = OrderedDict()
    for ci, name in enumerate(("case_a", "case_b")):
        shp = (24, 40, 40)
        j = np.arange(int(np.prod(shp)), dtype=np.float64).reshape(shp)
        zz, yy, xx = np.meshgrid(*[np.arange(s) for s in shp], indexing="ij")
        seg = np.minimum(((zz * 3 + yy * 5 + xx * 7 + ci) % 11 < 2).astype(np.float32) + ((zz + yy + xx) % 13 == 0) * 2.0, 2.0)
        arr = np.stack([np.round(np.sin(0.37 * j + ci), 2).astype(np.float32) * (zz > 4), seg]).astype(np.float32)
        path = os.path.join(str(tmp_path), name + ".npz")
        np.savez_compressed(path, data=arr)                                    # packed only: no .npy
        locs = OrderedDict((c, np.argwhere(seg == c)) for c in (1, 2))
        ds[name] = OrderedDict(data_file=path, properties=OrderedDict(class_locations=locs, name=name))
    args = (ds, (16, 18, 20), (12, 14, 16), 4, False)
    kw = dict(oversample_foreground_percent=0.33, pad_mode="constant", pad_kwargs_data={'constant_values': 0})
    np.random.seed(77)
    host = DataLoader3D(*args, **kw)
    want = [next(host) for _ in range(2)]
    want = [{k: (np.array(b[k]) if k in ("data", "seg") else b[k]) for k in b} for b in want]
    seen = []
    cache = DeviceCaseCache(None, "cuda", device_inflate="any")
    inner = cache._loader

    def loader(raw):
        from e2enet_medical_amd import deflate
        stats = {}
        deflate.load_npz(raw, keys=("data",), stats=stats, foreign=cache.foreign)
        seen.append(stats["data"]["route"])
        return inner(raw)
    cache._loader = loader
    np.random.seed(77)
    resident = ResidentDataLoader3D(*args, cache=cache, **kw)
    for w in want:
        b = next(resident)
        assert [str(k) for k in b['keys']] == [str(k) for k in w['keys']]
        assert np.array_equal(b['data'].cpu().numpy(), w['data']) and np.array_equal(b['seg'].cpu().numpy(), w['seg'].astype(np.float32))
    assert cache.inflated_cases == len(cache) == 2 and resident.staged_samples == 0 and seen == ["any", "any"]
    for name in ds:
        assert cache.fetch(ds[name])[0].cpu().numpy().tobytes() == np.load(ds[name]['data_file'])['data'].tobytes()
