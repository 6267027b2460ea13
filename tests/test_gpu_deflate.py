"""The device DEFLATE encoder (csrc/deflate.hip, e2enet_medical_amd/deflate.py) against host zlib: every stream inflates to its input
with ``eof`` set and nothing left over, the CRC-32 is zlib's, two calls give the same bytes; the size bounds that follow from the
format; the exact bytes of three small inputs; ``save_softmax_npz`` and ``nifti.write`` with ``device_deflate=True`` against their
default routes; the refusals.

``reference_stream`` below restates the format in Python (it is slow: small inputs only).  It is the oracle of the exact bytes, and
the two size bounds are checked on it without a device (``test_bounds_hold_on_the_restatement``)."""
import gzip
import os
import pickle
import zlib

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

CHUNK = 32768                     # asserted against e2e_deflate_chunk_bytes() by the GPU tests


# --------------------------------------------------------------------------------------------- the format, restated in Python
class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, nbits):
        """nbits of value, least significant first"""
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def huff(self, code, nbits):
        """a Huffman code: most significant bit first"""
        self.put(int(format(code, "0%db" % nbits)[::-1], 2), nbits)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)


_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DIST = {1: (0, 0, 0), 2: (1, 0, 0), 4: (3, 0, 0), 8: (5, 1, 1)}          # distance -> (code, extra bits, extra value)


def _literal(b, v):
    if v < 144:
        b.huff(0x30 + v, 8)
    else:
        b.huff(0x190 + v - 144, 9)


def _match(b, length, elem):
    i = max(k for k in range(29) if _LEN_BASE[k] <= length) if length < 258 else 28
    sym = 257 + i
    if sym < 280:
        b.huff(sym - 256, 7)
    else:
        b.huff(0xC0 + sym - 280, 8)
    b.put(length - _LEN_BASE[i], _LEN_EXTRA[i])
    code, eb, ev = _DIST[elem]
    b.huff(code, 5)
    b.put(ev, eb)


def reference_chunk(data, start, stop, elem):
    """bytes of the chunk data[start:stop]: a fixed-Huffman block closed by an empty stored block, or one stored block"""
    n = stop - start
    b = _Bits()
    b.put(0, 1)                                     # BFINAL
    b.put(1, 2)                                     # BTYPE 01
    i = start
    while i < stop:
        j = i
        while j < stop and j >= elem and data[j] == data[j - elem]:
            j += 1
        if j == i:
            _literal(b, data[i])
            i += 1
            continue
        run = j - i                                 # a maximal run of "the same element again" inside the chunk
        while run >= 258:
            _match(b, 258, elem)
            run -= 258
        if run >= 3:
            _match(b, run, elem)
        else:
            for k in range(j - run, j):
                _literal(b, data[k])
        i = j
    b.huff(0, 7)                                    # end of block
    b.put(0, 3)                                     # BFINAL 0, BTYPE 00
    b.align()
    fixed = bytes(b.out) + b"\x00\x00\xff\xff"
    if len(fixed) > 5 + n:
        return bytes([0, n & 0xFF, n >> 8, ~n & 0xFF, (~n >> 8) & 0xFF]) + bytes(data[start:stop])
    return fixed


def reference_stream(data, elem, chunk=CHUNK):
    data = bytes(data)
    return b"".join(reference_chunk(data, c, min(c + chunk, len(data)), elem) for c in range(0, len(data), chunk)) + b"\x03\x00"


def _ceil(a, b):
    return -(-a // b)


def random_bound(n, chunk=CHUNK):
    return n + 5 * _ceil(n, chunk) + 2


def constant_bound(n, chunk=CHUNK):
    return _ceil(n, chunk) * (_ceil(11 + 13 * _ceil(chunk, 258) + 17, 8) + 5) + 2


def _inflate(stream):
    d = zlib.decompressobj(-15)
    out = d.decompress(stream)
    return out, d.eof, d.unused_data


def _rand(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


@pytest.mark.parametrize("elem", [1, 2, 4, 8])
def test_bounds_hold_on_the_restatement(elem):
    """no device: the restatement inflates to its input, and the two bounds of the GPU tests hold on it.  The constant bound
    counts, per chunk, 3 bits of header, one 8-bit literal, ceil(C / 258) matches of 13 bits (8 for the length 258, 5 for the
    distance), 7 + 3 bits of end-of-block and stored header, 7 of padding, then 00 00 FF FF and one byte to spare.  The first chunk
    really starts with ``elem`` literals and every chunk ends with a shorter match of up to 18 bits: at C = 32768 = 127 * 258 + 2 the
    spare byte covers that for elements whose bytes are below 144 (8-bit literals), which is what the constants here and in the GPU
    tests are.  Distance 8 has an extra bit per match (14 bits), which the formula does not count: elem 8 is not held to it."""
    for n in (0, elem, 3 * elem, 258 * elem, CHUNK - elem, CHUNK, CHUNK + elem, 2 * CHUNK + 8):
        const = bytes([0x3C, 0x00, 0x11, 0x22, 0x33, 0x44, 0x55, 0x66][:elem]) * (n // elem)
        s = reference_stream(const, elem)
        assert _inflate(s) == (const, True, b"")
        if n >= CHUNK and elem < 8:
            assert len(s) <= constant_bound(n), (n, len(s), constant_bound(n))
        rnd = _rand(n, n).tobytes()
        s = reference_stream(rnd, elem)
        assert _inflate(s) == (rnd, True, b"")
        assert len(s) <= random_bound(n)


# ------------------------------------------------------------------------------------------------------------------- the device
def _deflate():
    from e2enet_medical_amd import deflate
    assert deflate.chunk_bytes() == CHUNK
    return deflate


def _check(host, elem):
    """round trip, CRC, determinism; returns the stream"""
    d = _deflate()
    host = np.ascontiguousarray(host).view(np.uint8).reshape(-1).copy()
    dev = torch.from_numpy(host).cuda()
    stream, crc, nbytes = d.raw_deflate(dev, elem)
    out, eof, unused = _inflate(stream)
    assert nbytes == host.size
    assert eof and unused == b""
    assert out == host.tobytes()
    assert crc == zlib.crc32(host.tobytes())
    again = d.raw_deflate(dev, elem)
    assert again[0] == stream and again[1] == crc
    return stream


SIZES = [0, 1, 2, 3, 4, 257, 258, 259, 260, 261, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3, 5 * CHUNK + 17]


def _round(n, elem):
    return n // elem * elem


@gpu
@pytest.mark.parametrize("elem", [1, 2, 4])
def test_constant_and_random_buffers_of_every_size(elem):
    """sizes around the match lengths and the chunk size (rounded down to whole elements, and once more in bytes with elem 1 at the
    odd sizes), constant and random: round trip, CRC, determinism and the two size bounds (the constant's bytes are below 144, see
    ``test_bounds_hold_on_the_restatement``)"""
    value = bytes([0x00, 0x3C, 0x81, 0x7F][:elem])
    for size in SIZES:
        for n, e in {(_round(size, elem), elem), (size, 1)}:
            const = np.frombuffer(value * (n // len(value)) + value[:n % len(value)], dtype=np.uint8)
            s = _check(const, e)
            if e == elem and n % len(value) == 0:
                assert len(s) <= constant_bound(n) if n else s == b"\x03\x00", (n, e, len(s))
            s = _check(_rand(n, 100 + n), e)
            assert len(s) <= random_bound(n), (n, e, len(s))


@gpu
@pytest.mark.parametrize("elem", [1, 2, 4])
def test_runs_between_distinct_values(elem):
    """runs of exactly 2, 3, 258, 259, 260, 261, 516 and 517 elements (and the same counts in bytes) between distinct values"""
    dt = {1: np.uint8, 2: np.uint16, 4: np.uint32}[elem]
    runs = [2, 3, 258, 259, 260, 261, 516, 517]
    parts, v = [], 1
    for rep in range(3):
        for r in runs + [-(-k // elem) for k in runs] + [(k + 1) // elem + 1 for k in runs]:
            parts.append(np.full(r, v * 2654435761 % 2 ** (8 * elem), dtype=np.uint64).astype(dt))
            v += 1
            parts.append(np.array([v * 40503 % 251, (v + 1) * 40503 % 241], dtype=dt)[:1 + rep % 2])   # one or two distinct values
            v += 2
    host = np.concatenate(parts)
    s = _check(host, elem)
    assert s == reference_stream(host.tobytes(), elem)
    assert len(s) < host.nbytes // 8


@gpu
@pytest.mark.parametrize("elem", [1, 2, 4])
def test_run_across_a_chunk_boundary(elem):
    """a run that begins elem bytes before a chunk boundary and ends behind it: the second chunk's first token is a match that
    reaches back in front of the chunk"""
    host = _rand(2 * CHUNK + 64, 7)
    host[CHUNK - 2 * elem:CHUNK + 700] = np.tile(np.arange(1, elem + 1, dtype=np.uint8), (700 + 2 * elem) // elem + 1)[:700 + 2 * elem]
    s = _check(host, elem)
    assert s[:len(s)] == reference_stream(host.tobytes(), elem)


@gpu
@pytest.mark.parametrize("elem", [1, 2, 4])
def test_fp16_constant_with_islands(elem):
    """fp16 1.0 repeated, with random 37-byte islands"""
    rng = np.random.default_rng(11)
    host = np.full(3 * CHUNK // 2 + 50, 1.0, dtype=np.float16).view(np.uint8).copy()
    for at in rng.integers(0, host.size - 37, 40):
        host[at:at + 37] = rng.integers(0, 256, 37, dtype=np.uint8)
    host = host[:_round(host.size, elem)]
    s = _check(host, elem)
    if elem == 2:
        assert len(s) < host.size // 4


@gpu
@pytest.mark.parametrize("elem", [1, 2, 4])
def test_random_chunk_then_constant_chunk(elem):
    """the first chunk is random (stored), the second constant (fixed Huffman, its first match reaching into the stored chunk)"""
    host = np.concatenate([_rand(CHUNK, 3), np.full(CHUNK, 0x5A, dtype=np.uint8)])
    s = _check(host, elem)
    assert len(s) <= random_bound(CHUNK) - 2 + constant_bound(CHUNK)
    assert s[:5] == bytes([0, CHUNK & 0xFF, CHUNK >> 8, ~CHUNK & 0xFF, (~CHUNK >> 8) & 0xFF])


@gpu
@pytest.mark.parametrize("case", ["three_bytes", "short_runs", "two_chunks"])
def test_exact_bytes_of_small_cases(case):
    """the restatement is the oracle of the bytes"""
    if case == "three_bytes":
        host, elem = np.array([7, 7, 7], dtype=np.uint8), 1
    elif case == "short_runs":
        host, elem = np.array([1, 1, 2, 2, 2, 3, 3, 3, 3, 200, 200, 200, 200, 200, 9] * 5, dtype=np.uint16), 2
    else:
        host = np.zeros(CHUNK + 600, dtype=np.uint8)
        host[100:140] = np.arange(40)
        host[CHUNK + 300] = 1
        elem = 4
    s = _check(host, elem)
    assert s == reference_stream(host.tobytes(), elem)


@gpu
def test_elem_8_round_trip_and_bytes():
    """the one distance with an extra bit: fp64 runs, a run over a chunk boundary, random bytes"""
    rng = np.random.default_rng(8)
    vals = np.repeat(rng.normal(0, 1, 40), rng.integers(1, 300, 40)).astype(np.float64)
    host = np.concatenate([vals, np.zeros(CHUNK // 8 + 50), rng.normal(0, 1, 30)])        # (the zeros cross a chunk boundary)
    s = _check(host, 8)
    assert s == reference_stream(host.tobytes(), 8)
    assert len(_check(_rand(CHUNK + 8, 9), 8)) <= random_bound(CHUNK + 8)


# ----------------------------------------------------------------------------------------------------------------- end to end
@gpu
def test_save_softmax_npz_device_route_equals_default(tmp_path):
    from e2enet_medical_amd.inference.predict import save_softmax_npz
    rng = np.random.default_rng(5)
    logits = rng.normal(0, 4, (5, 7, 33, 65)).astype(np.float32)
    logits[:, :, :20] = 0
    logits[0, :, :20] = 30
    soft = torch.softmax(torch.from_numpy(logits), 0).to(torch.float16).cuda().contiguous()
    props = {"itk_spacing": (1., 1., 2.), "size_after_cropping": (7, 33, 65), "name": "case"}
    a, b = str(tmp_path / "a.npz"), str(tmp_path / "b.npz")
    save_softmax_npz(soft, a, props, [2, 1])
    save_softmax_npz(soft, b, props, [2, 1], device_deflate=True)
    got, want = np.load(b)["softmax"], np.load(a)["softmax"]
    assert got.dtype == np.float16 and got.shape == want.shape
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
    assert open(a[:-4] + ".pkl", "rb").read() == open(b[:-4] + ".pkl", "rb").read()
    assert pickle.load(open(b[:-4] + ".pkl", "rb"))["regions_class_order"] == [2, 1]
    import zipfile
    assert zipfile.ZipFile(b).testzip() is None


@gpu
def test_savez_takes_host_arrays_and_several_members(tmp_path):
    """three members of three dtypes, one of them a host array (uploaded), one empty: np.load gives them back, testzip passes"""
    import zipfile
    from e2enet_medical_amd import deflate
    rng = np.random.default_rng(12)
    u1 = np.repeat(rng.integers(0, 3, 900, dtype=np.uint8), 41).reshape(9, 41, 100)
    f4 = np.round(rng.normal(0, 1, (3, 70000)), 1).astype(np.float32)
    f2 = np.zeros((0, 5), dtype=np.float16)
    path = str(tmp_path / "three.npz")
    deflate.savez(path, labels=u1, values=torch.from_numpy(f4).cuda(), empty=torch.from_numpy(f2).cuda())
    assert zipfile.ZipFile(path).testzip() is None
    with np.load(path) as got:
        assert sorted(got.files) == ["empty", "labels", "values"]
        for key, want in (("labels", u1), ("values", f4), ("empty", f2)):
            assert got[key].dtype == want.dtype and got[key].shape == want.shape and got[key].tobytes() == want.tobytes()


@gpu
def test_nifti_write_device_route_equals_default(tmp_path):
    from e2enet_medical_amd import nifti
    rng = np.random.default_rng(6)
    seg = np.zeros((5, 33, 65), dtype=np.uint8)
    seg[1:4, 5:25, 10:50] = rng.integers(0, 4, (3, 20, 40), dtype=np.uint8)
    props = {"itk_spacing": (0.5, 0.75, 2.0), "itk_origin": (1., -2., 3.), "itk_direction": (1., 0., 0., 0., 1., 0., 0., 0., 1.)}
    a, b = str(tmp_path / "a.nii.gz"), str(tmp_path / "b.nii.gz")
    nifti.write(seg, a, props)
    nifti.write(torch.from_numpy(seg).cuda(), b, props, device_deflate=True)
    assert gzip.decompress(open(b, "rb").read()) == gzip.decompress(open(a, "rb").read())
    raw = nifti.read_raw(b)
    assert raw.shape == seg.shape and raw.itk_spacing == nifti.read_raw(a).itk_spacing
    assert np.array_equal(nifti.decode_u8(raw).cpu().numpy(), seg)
    assert getattr(nifti.writer, "accepts_device", False) is True


@gpu
def test_predict_cases_device_route_equals_default(tmp_path):
    """predict_cases(save_npz=True) twice on the tiny network: with the flag nifti.writer is handed the device label volume, and
    both files inflate to what the default route writes; a writer without ``accepts_device`` still gets the host array"""
    from e2enet_medical_amd import nifti
    from e2enet_medical_amd.inference.predict import predict_cases
    from e2enet_medical_amd.training.network_training.nnUNetTrainer_simple import nnUNetTrainer_simple
    from tests.helpers import seeded_input
    from tests.test_gpu_net import TINY, load_closed_form
    plans = {'plans_per_stage': {0: {'batch_size': 2, 'patch_size': list(TINY["patch"]), 'num_pool_per_axis': [3, 5, 5],
                                     'pool_op_kernel_sizes': [list(p) for p in TINY["pools"]],
                                     'conv_kernel_sizes': [[3, 3, 3]] * 6, 'do_dummy_2D_data_aug': False}},
             'base_num_features': 32, 'num_modalities': TINY["cin"], 'num_classes': TINY["k"] - 1, 'all_classes': [1, 2],
             'transpose_forward': [0, 1, 2], 'transpose_backward': [0, 1, 2], 'conv_per_stage': 2}
    tr = nnUNetTrainer_simple(plans, 0, output_folder=None, Tconv='shiftConvPP', max_num_epochs=1, num_batches_per_epoch=1)
    tr.base_num_features_override = TINY["base"]
    tr.synthetic_data = True
    torch.manual_seed(0)
    net, _ = tr.initialize(True)
    load_closed_form(net)
    params = [{'epoch': 0, 'state_dict': {k: v.detach().cpu().clone() for k, v in net.state_dict().items()},
               'optimizer_state_dict': None, 'plot_stuff': ([], [], [], []), 'best_stuff': (None, None, None)}]
    vol = seeded_input((TINY["cin"], 16, 34, 37), seed=11).numpy()
    props = {'size_after_cropping': np.array([16, 34, 37]), 'original_size_of_raw_data': np.array([18, 35, 41]),
             'crop_bbox': [[1, 17], [0, 34], [3, 40]], 'itk_spacing': (0.7, 0.8, 2.5), 'itk_origin': (-90.5, 126.0, -72.25),
             'itk_direction': (1., 0., 0., 0., 1., 0., 0., 0., 1.)}
    os.makedirs(str(tmp_path / "a"))
    os.makedirs(str(tmp_path / "b"))
    a, b = str(tmp_path / "a" / "case0.nii.gz"), str(tmp_path / "b" / "case0.nii.gz")
    handed = []

    def spy(seg, path, properties, device_deflate=False):
        handed.append((type(seg), device_deflate))
        nifti.writer(seg, path, properties, device_deflate=device_deflate)
    spy.accepts_device = True
    assert predict_cases(tr, params, [(a, (vol, props))], nifti.writer, do_tta=False, save_npz=True) == [a]
    assert predict_cases(tr, params, [(b, (vol, props))], spy, do_tta=False, save_npz=True, device_deflate=True) == [b]
    assert handed == [(torch.Tensor, True)]
    assert gzip.decompress(open(b, "rb").read()) == gzip.decompress(open(a, "rb").read())
    want, got = np.load(a[:-7] + ".npz")["softmax"], np.load(b[:-7] + ".npz")["softmax"]
    assert got.dtype == np.float16 and np.array_equal(got.view(np.uint16), want.view(np.uint16))
    assert open(a[:-7] + ".pkl", "rb").read() == open(b[:-7] + ".pkl", "rb").read()
    plain = []
    predict_cases(tr, params, [(b, (vol, props))], lambda seg, path, properties: plain.append(seg), do_tta=False, device_deflate=True)
    assert isinstance(plain[0], np.ndarray) and plain[0].tobytes() == gzip.decompress(open(a, "rb").read())[352:]


@gpu
def test_validate_device_route_stores_the_same_probabilities(tmp_path):
    """validate(save_softmax=True) with and without the flag on a synthetic task: every case's ``softmax`` loads bit for bit equal
    (the device route rounds and permutes with softmax_to_f16, the default on the host), and summary.json holds the same scores"""
    import json
    from tests.helpers import write_synthetic_task
    from tests.test_gpu_trainer import PLANS
    from e2enet_medical_amd.training.network_training.nnUNetTrainer_simple import nnUNetTrainer_simple
    ddir, plans = write_synthetic_task(str(tmp_path / "pre"), plans=dict(PLANS), n_cases=5)
    tr = nnUNetTrainer_simple(plans, 0, output_folder=str(tmp_path / "out"), dataset_directory=ddir, batch_dice=False,
                              Tconv='shiftConvPP', max_num_epochs=1, num_batches_per_epoch=2)
    tr.base_num_features_override = 8
    torch.manual_seed(0)
    np.random.seed(0)
    tr.initialize(True)
    kw = dict(do_mirroring=False, save_softmax=True, writer=lambda seg, path, props: None)
    tr.validate(validation_folder_name="host", **kw)
    tr.validate(validation_folder_name="device", device_deflate=True, **kw)
    assert len(tr.dataset_val) >= 1
    for k in tr.dataset_val.keys():
        want = np.load(os.path.join(tr.output_folder, "host", k + ".npz"))["softmax"]
        got = np.load(os.path.join(tr.output_folder, "device", k + ".npz"))["softmax"]
        assert got.dtype == want.dtype == np.float16 and got.shape == want.shape
        assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
    mean = [json.load(open(os.path.join(tr.output_folder, f, "summary.json")))["results"]["mean"] for f in ("host", "device")]
    assert mean[0] == mean[1]


# -------------------------------------------------------------------------------------------------------------------- refusals
@gpu
def test_refusals(tmp_path):
    from e2enet_medical_amd import nifti
    from e2enet_medical_amd.inference.predict import save_softmax_npz
    d = _deflate()
    x = torch.arange(64 * 6, dtype=torch.uint8, device="cuda").reshape(64, 6)
    with pytest.raises(ValueError, match="contiguous"):
        d.raw_deflate(x.t())
    with pytest.raises(ValueError, match="device tensor"):
        d.raw_deflate(x.cpu())
    with pytest.raises(ValueError, match="does not divide"):
        d.raw_deflate(x.reshape(-1)[:6], 4)
    with pytest.raises(ValueError, match="elem"):
        d.raw_deflate(x, 3)
    seg = torch.zeros((4, 6, 8), dtype=torch.uint8)
    with pytest.raises(ValueError, match="device tensor"):
        nifti.write(seg, str(tmp_path / "c.nii.gz"), None, device_deflate=True)
    with pytest.raises(ValueError, match="contiguous"):
        nifti.write(seg.cuda().permute(2, 1, 0), str(tmp_path / "c.nii.gz"), None, device_deflate=True)
    with pytest.raises(ValueError, match="three axes"):
        nifti.write(seg.cuda()[0], str(tmp_path / "c.nii.gz"), None, device_deflate=True)
    with pytest.raises(ValueError, match="no labels"):
        nifti.write(torch.full((2, 3, 4), 300, dtype=torch.int32, device="cuda"), str(tmp_path / "c.nii.gz"), None, device_deflate=True)
    assert not os.path.exists(str(tmp_path / "c.nii.gz"))
    with pytest.raises(ValueError, match="device tensor"):
        save_softmax_npz(torch.zeros((2, 3, 4, 5), dtype=torch.float16), str(tmp_path / "c.npz"), {}, device_deflate=True)
    from e2enet_medical_amd._lib import lib, E2EError
    with pytest.raises(E2EError, match="elem"):
        lib().deflate_encode(x.data_ptr(), 6, 4, None, None, None, x.data_ptr(), torch.cuda.current_stream().cuda_stream)
