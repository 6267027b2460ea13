"""``deflate.inflate_any`` without a device: tests/inflate_any_oracle.py pinned to zlib stage by stage (find against a block walker,
count / write / windows / resolve against ``zlib.decompress``), the None rules, and -- through the hooks -- ``inflate_any``,
``load_npz(foreign="device")`` and ``nifti.read_raw(inflate="device")`` against the host route; the command-line refusals.  The
inputs of tests/test_gpu_inflate_any.py are built here and are checked here to be free of false block starts."""
import functools
import gzip
import struct
import zlib

import numpy as np
import pytest

from tests import inflate_any_oracle as oracle

W = oracle.W


# ------------------------------------------------------------------------------------------------------------------------ inputs
def ct_like(nvox, seed=0):
    """an int16 random walk around -1000 with steps of at most 3: the low byte wanders, the high byte is nearly constant"""
    r = np.random.default_rng(seed)
    return (np.cumsum(r.integers(-3, 4, nvox)) - 1000).astype(np.int16).tobytes()


def label_runs(nbytes, seed=1):
    """uint8 labels 0..3 in runs of 50-75"""
    r = np.random.default_rng(seed)
    runs = []
    while sum(map(len, runs)) < nbytes:
        runs.append(bytes([int(r.integers(0, 4))]) * int(r.integers(50, 76)))
    return b"".join(runs)[:nbytes]


def raw_deflate(data, level=6, mem=1, strategy=zlib.Z_DEFAULT_STRATEGY, flush=zlib.Z_FINISH):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
    return c.compress(data) + c.flush(flush)


def joined_pieces():
    """(e): pieces of every block type in one stream -- Z_FIXED, Z_RLE, Z_HUFFMAN_ONLY and level 0 pieces between pieces compressed
    normally, every piece but the last closed by a sync or a full flush (an empty stored block, a byte-aligned restart).  A piece is
    a stream of its own that is not final, so no match reaches over a joint."""
    normal = [ct_like(3000, 10 + i) for i in range(5)]
    odd = [(ct_like(150, 20), 6, zlib.Z_FIXED), (label_runs(400, 21), 6, zlib.Z_RLE), (ct_like(200, 22), 6, zlib.Z_HUFFMAN_ONLY),
           (ct_like(100, 23), 0, zlib.Z_DEFAULT_STRATEGY)]
    raw, stream = b"", b""
    for i, piece in enumerate(normal):
        last = i == len(normal) - 1
        stream += raw_deflate(piece, 6, 1, flush=zlib.Z_FINISH if last else (zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH)[i & 1])
        raw += piece
        if not last:
            data, level, strategy = odd[i]
            stream += raw_deflate(data, level, 1, strategy, zlib.Z_SYNC_FLUSH if i & 1 else zlib.Z_FULL_FLUSH)
            raw += data
    return raw, stream


class BitWriter:
    def __init__(self):
        self.acc, self.n = 0, 0

    def bits(self, value, count):                      # least significant bit first (header fields, extra bits)
        self.acc |= (value & ((1 << count) - 1)) << self.n
        self.n += count

    def code(self, value, count):                      # a Huffman code: most significant bit first
        for i in range(count - 1, -1, -1):
            self.bits((value >> i) & 1, 1)

    def bytes(self):
        assert self.n % 8 == 0
        return self.acc.to_bytes(self.n // 8, "little")


def fixed_match_block(length_symbol, length_extra, dist_code, dist_extra):
    """one non-final fixed-Huffman block that holds a single match, closed by an empty stored block: byte-aligned at both ends"""
    w = BitWriter()
    w.bits(0, 1), w.bits(1, 2)
    assert 280 <= length_symbol <= 285 or 257 <= length_symbol <= 279
    if length_symbol >= 280:
        w.code(0xC0 + length_symbol - 280, 8)
    else:
        w.code(length_symbol - 256, 7)
    w.bits(*length_extra)
    w.code(dist_code, 5)
    w.bits(*dist_extra)
    w.code(0, 7)                                       # end of block
    w.bits(0, 3)                                       # BFINAL 0, BTYPE 00
    w.bits(0, -w.n % 8)
    w.bits(0x0000, 16), w.bits(0xFFFF, 16)
    return w.bytes()


def distance_w_stream():
    """zlib never looks further back than 32506 bytes, so a match at the full distance is written by hand: 40 000 bytes through
    zlib (full flush), then twice "258 bytes from 32768 back" in a fixed block each, then more zlib output and the end"""
    head, tail = ct_like(20000, 30), ct_like(3000, 31)
    stream = raw_deflate(head, 6, 1, flush=zlib.Z_FULL_FLUSH)
    block = fixed_match_block(285, (0, 0), 29, (W - 24577, 13))
    stream += block + block + raw_deflate(tail, 6, 1)
    raw = bytearray(head)
    for _ in range(2):
        raw += raw[len(raw) - W:len(raw) - W + 258]
    return bytes(raw + tail), stream


@functools.lru_cache(maxsize=None)
def inputs():
    """name -> (raw bytes, raw DEFLATE stream, the segment sizes S it is served at).  With the default cap of 8 S every gap between
    block starts passes at the listed S (asserted below), except for ``c``, ``d`` and ``h``: random bytes do not compress, zlib
    stores them, there is no dynamic block and the answer is None."""
    rnd = np.random.default_rng(5).integers(0, 256, W, dtype=np.uint8).tobytes()
    period = ct_like(15000, 3)
    out = {}
    for nvox in (15000, 100000):
        for level in (1, 6, 9):
            out["a_ct_%d_level%d" % (nvox, level)] = (ct_like(nvox), level, 1, (64, 256, 4096))
    out["b_labels"] = (label_runs(60000), 6, 1, (64, 256, 4096))
    out["c_random_period_w"] = (rnd * 3 + rnd[:100], 9, 9, (8192,))
    out["d_random_period_w_mem1"] = (rnd * 3 + rnd[:100], 9, 1, (64,))
    # what c and d are after -- far matches, windows handed down hundreds of short spans -- on data zlib does find matches in:
    out["c_ct_period_30000"] = (period * 3 + period[:100], 9, 9, (4096,))
    out["d_ct_period_30000_mem1"] = (period * 3 + period[:100], 9, 1, (64,))
    for size in (0, 1, W - 1, W, W + 1):
        out["f_size_%d" % size] = (ct_like(W)[:size], 6, 1, (64,))
    out["g_ct_200k_default"] = (ct_like(100000, 7), 6, 8, (16384,))
    out["h_random_stored"] = (rnd[:20000], 6, 1, (64, 256))                   # (20 KB: over both caps)
    built = {name: (raw, raw_deflate(raw, level, mem), sizes) for name, (raw, level, mem, sizes) in out.items()}
    raw, stream = joined_pieces()
    built["e_joined_pieces"] = (raw, stream, (64, 256))
    raw, stream = distance_w_stream()
    built["x_distance_w_by_hand"] = (raw, stream, (64, 4096))
    return built


NONE_INPUTS = ("c_random_period_w", "d_random_period_w_mem1", "h_random_stored")
NAMES = sorted(inputs())
CASES = [(name, S) for name in NAMES for S in inputs()[name][2]]


@functools.lru_cache(maxsize=None)
def headers(name):
    return tuple(oracle.valid_headers(inputs()[name][1]))


@functools.lru_cache(maxsize=None)
def stages(name, S):
    """every stage of the oracle for one input: dict(starts, records, offs, sym, wins, out), or None by the gap rule"""
    raw, stream, _ = inputs()[name]
    starts = oracle.compact(oracle.find(stream, S, headers(name)))
    if not oracle.gaps_ok(starts, len(stream), 8 * S):
        return None
    records = oracle.count(stream, starts, 8 * S)
    status, final, end, lengths = oracle.unpack_records(records)
    assert not status.any() and final[-1] == 1 and not final[:-1].any(), (name, S, status)
    offs = oracle.offsets(lengths)
    sym, bad = oracle.write(stream, starts, offs, 8 * S)
    assert bad == 0
    wins, bad = oracle.windows(sym, offs)
    assert bad == 0
    return dict(starts=starts, records=records, offs=offs, sym=sym, wins=wins, out=oracle.resolve(sym, offs, wins).tobytes())


# ------------------------------------------------------------------------------------------------------------ the block walker
def walk_blocks(stream):
    """[(bit position, BFINAL, BTYPE)] of every block of a stream, in order, and the inflated length: a serial walk from bit 0"""
    bits, blocks, total = oracle.Bits(stream, 0), [], 0
    while True:
        at = bits.pos
        final, btype = bits.take(1), bits.take(2)
        blocks.append((at, final, btype))
        assert btype != 3
        if btype == 0:
            bits.pos = (bits.pos + 7) & ~7
            length, nlength = bits.take(16), bits.take(16)
            assert length == ~nlength & 0xFFFF
            bits.pos += 8 * length
            total += length
        else:
            ll, d = (oracle.FIXED_LL, oracle.FIXED_D) if btype == 1 else oracle.dynamic_tables(bits)
            ll_table, d_table = oracle.canonical(ll), oracle.canonical(d)
            while True:
                s = oracle.decode(bits, ll_table)
                if s < 256:
                    total += 1
                    continue
                if s == 256:
                    break
                total += 258 if s == 285 else s - 254 if s < 265 else 3 + ((4 + ((s - 261) & 3)) << ((s - 261) >> 2)) + bits.take((s - 261) >> 2)
                dc = oracle.decode(bits, d_table)
                bits.take((dc >> 1) - 1 if dc >= 4 else 0)
        if final:
            assert (bits.pos + 7) // 8 == len(stream)
            return blocks, total


@pytest.mark.parametrize("name", NAMES)
def test_the_inputs_inflate_and_their_headers_are_exactly_the_block_starts(name):
    """no false positive and no miss of the header check at any bit offset of any input; find = first true start per segment"""
    raw, stream, sizes = inputs()[name]
    assert zlib.decompress(stream, -15) == raw
    blocks, total = walk_blocks(stream)
    assert total == len(raw)
    true_starts = [at for at, final, btype in blocks if btype == 2 and not final]
    assert list(headers(name)) == true_starts
    if name in NONE_INPUTS:
        assert true_starts == []
    for S in sizes:
        found = oracle.find(stream, S, headers(name))
        assert found[0] == 0 and len(found) == max(1, -(-len(stream) // S))
        for s in range(1, len(found)):
            inside = [p for p in true_starts if 8 * s * S <= p < 8 * (s + 1) * S]
            assert found[s] == (inside[0] if inside else -1)


@pytest.mark.parametrize("name,S", CASES)
def test_every_stage_against_zlib(name, S):
    raw, stream, _ = inputs()[name]
    got = stages(name, S)
    if name in NONE_INPUTS:
        assert got is None and oracle.inflate(stream, S) is None
        return
    assert got is not None, "the gap rule refuses %s at S = %d" % (name, S)
    assert got["out"] == raw == oracle.inflate(stream, S)
    status, final, end, lengths = oracle.unpack_records(got["records"])
    assert list(end[:-1]) == list(got["starts"][1:]) and (end[-1] + 7) // 8 == len(stream)
    # the windows are the true bytes in front of every span
    padded = np.frombuffer(bytes(W) + raw, dtype=np.uint8)
    for k in range(1, len(got["starts"])):
        assert got["wins"][k].tobytes() == padded[int(got["offs"][k]):int(got["offs"][k]) + W].tobytes()


def test_what_the_inputs_exercise():
    """the properties the cases were chosen for hold (so a change of zlib's that loses one is noticed here, not on the device)"""
    lengths = lambda name, S: np.diff(stages(name, S)["offs"])
    d = stages("d_ct_period_30000_mem1", 64)
    short = np.diff(d["offs"]) < W
    assert len(d["starts"]) > 50 and short[:-1].all()                      # many short spans in a row: windows carried over
    assert int((d["sym"] >= 0x8000).sum()) > 10000                           # markers, copied by later matches
    assert len(stages("a_ct_100000_level6", 64)["starts"]) > 300 and len(stages("a_ct_15000_level6", 4096)["starts"]) <= 5
    assert len(stages("g_ct_200k_default", 16384)["starts"]) <= 8
    assert all(len(stages("f_size_%d" % n, 64)["out"]) == n for n in (0, 1, W - 1, W, W + 1))
    kinds = {btype for _, _, btype in walk_blocks(inputs()["e_joined_pieces"][1])[0]}
    assert kinds == {0, 1, 2}
    x = stages("x_distance_w_by_hand", 64)
    assert (x["sym"] >= 0x8000).any() and lengths("x_distance_w_by_hand", 64).min() < W
    assert stages("x_distance_w_by_hand", 4096) is not None
    assert min(lengths("b_labels", 64)) > 0


# ------------------------------------------------------------------------------------------------------------------- the hooks
def hooks():
    def write(data, starts, offs, cap, nbytes):
        sym, bad = oracle.write(data.tobytes(), starts, offs, cap)
        if bad:
            raise ValueError("inflate_any: %d corrupt spans" % bad)
        wins, bad = oracle.windows(sym, offs)
        assert not bad and len(sym) == nbytes
        return oracle.resolve(sym, offs, wins)
    return dict(find=lambda data, S: oracle.find(data.tobytes(), S), count=lambda data, starts, cap: oracle.count(data.tobytes(), starts, cap),
                write=write)


@pytest.mark.parametrize("name", ["a_ct_15000_level6", "e_joined_pieces", "f_size_0", "f_size_1", "x_distance_w_by_hand", "h_random_stored"])
def test_inflate_any_through_the_hooks(name):
    from e2enet_medical_amd import deflate
    raw, stream, sizes = inputs()[name]
    stats = {}
    got = deflate.inflate_any(stream, len(raw), segment_bytes=sizes[0], stats=stats, **hooks())
    if name in NONE_INPUTS:
        assert got is None and "gap" in stats["refused"] and stats["starts"] == 0 and stats["spans"] == 1
        return
    want = stages(name, sizes[0])
    assert got.tobytes() == raw and stats["refused"] is None
    assert stats["spans"] == len(want["starts"]) == stats["starts"] + 1 and stats["sym_bytes"] == 2 * len(raw)
    assert stats["largest_gap"] == oracle.largest_gap(want["starts"], len(stream))
    assert stats["window_bytes"] == (W * stats["spans"] if stats["spans"] > 1 else 0)


def test_the_none_rules():
    from e2enet_medical_amd import deflate
    raw, stream, _ = inputs()["a_ct_15000_level6"]
    h = hooks()
    run = lambda s, n, **kw: deflate.inflate_any(s, n, **{**dict(segment_bytes=256), **h, **kw})
    stats = {}
    assert run(stream, len(raw) + 1, stats=stats) is None and "not %d" % (len(raw) + 1) in stats["refused"]      # the length
    assert run(stream, len(raw), max_span_bytes=100, stats=stats) is None and "gap" in stats["refused"]          # the cap
    assert run(b"", 0, stats=stats) is None and stats["refused"] == "an empty stream"
    assert run(stream[:-40], len(raw), stats=stats) is None and "span" in stats["refused"]                       # no final block
    assert run(stream + b"\x00", len(raw), stats=stats) is None and "BFINAL" in stats["refused"]                 # ends too early
    # a start that is no block start: the span in front of it runs over it
    starts = stages("a_ct_15000_level6", 256)["starts"]

    def false_start(data, S):
        found = oracle.find(data.tobytes(), S)
        k = int(np.flatnonzero(found > 0)[3])
        found[k] += 5
        return found
    assert run(stream, len(raw), find=false_start, stats=stats) is None and "overshoot" in stats["refused"]
    assert stats["spans"] == len(starts)
    with pytest.raises(ValueError):
        run(stream, len(raw), segment_bytes=8)
    # the writing pass trusts nothing: a count that lies about a length is a ValueError, not wrong bytes
    def lying_count(data, st, cap):
        r = oracle.count(data.tobytes(), st, cap)
        r[2, 4] += 1
        r[3, 4] -= 1
        return r
    with pytest.raises(ValueError):
        run(stream, len(raw), count=lying_count)


def test_a_flipped_bit_never_gives_wrong_bytes():
    from e2enet_medical_amd import deflate
    raw, stream, _ = inputs()["a_ct_15000_level6"]
    for at in (len(stream) // 2, len(stream) // 3, 100):
        for bit in (0, 3, 7):
            bad = bytearray(stream)
            bad[at] ^= 1 << bit
            try:
                got = deflate.inflate_any(bytes(bad), len(raw), segment_bytes=256, **hooks())
            except ValueError:
                continue
            if got is not None:                        # a flip that gives another valid stream of the same length: zlib agrees
                assert got.tobytes() == zlib.decompress(bytes(bad), -15)


def test_the_gzip_header_parser():
    raw = ct_like(500)
    plain = gzip.compress(raw, 6, mtime=0)
    at, crc, isize = oracle.gzip_member(plain)
    assert at == 10 and crc == zlib.crc32(raw) and isize == len(raw) and zlib.decompress(plain[at:-8], -15) == raw
    body = plain[10:]
    extra = b"AB\x03\x00xyz"
    full = b"\x1f\x8b\x08" + bytes([2 | 4 | 8 | 16]) + plain[4:10] + struct.pack("<H", len(extra)) + extra + b"name.nii\x00" + b"note\x00"
    full += struct.pack("<H", zlib.crc32(full) & 0xFFFF) + body
    at, crc, isize = oracle.gzip_member(full)
    assert zlib.decompress(full[at:-8], -15) == raw and gzip.decompress(full) == raw
    for bad in (b"\x1f\x8c" + plain[2:], plain[:2] + b"\x07" + plain[3:], plain[:3] + b"\x20" + plain[4:], plain[:12]):
        with pytest.raises(ValueError):
            oracle.gzip_member(bad)


# ---------------------------------------------------------------------------------------------------------------- containers
def _npz_inflater(calls):
    from e2enet_medical_amd import deflate

    def inflater(stream, nbytes, st):
        calls.append(nbytes)
        got = deflate.inflate_any(stream, nbytes, segment_bytes=4096, stats=st.setdefault("any", {}), **hooks())
        return got, (zlib.crc32(got.tobytes()) if got is not None else 0)
    return inflater


def test_load_npz_foreign_through_the_hooks(tmp_path):
    import torch
    from e2enet_medical_amd import deflate
    rng = np.random.default_rng(0)
    arrays = {"data": np.frombuffer(ct_like(6000, 40), dtype=np.int16).reshape(10, 20, 30).copy(),
              "noise": rng.integers(0, 256, 40000, dtype=np.uint8),                       # stored blocks: None, the host route
              "fortran": np.asfortranarray(np.arange(24, dtype=np.float32).reshape(4, 6)),
              "empty": np.zeros((0, 3), dtype=np.float32)}
    path = str(tmp_path / "case.npz")
    np.savez_compressed(path, **arrays)
    calls, stats = [], {}
    got = deflate.load_npz(path, device="cpu", stats=stats, inflater=_npz_inflater(calls), foreign="device")
    ref = np.load(path)
    for key in ref.files:
        assert isinstance(got[key], torch.Tensor) and got[key].dtype == torch.from_numpy(np.ascontiguousarray(ref[key])).dtype
        assert tuple(got[key].shape) == ref[key].shape and np.array_equal(got[key].numpy(), ref[key]), key
    assert stats["data"]["route"] == "any" and stats["data"]["any"]["refused"] is None
    assert stats["noise"]["route"] == "host" and "gap" in stats["noise"]["any"]["refused"]
    assert stats["fortran"]["route"] == "host" and "any" not in stats["fortran"]
    # the default leaves foreign members alone
    calls.clear()
    got = deflate.load_npz(path, device="cpu", stats=stats, inflater=_npz_inflater(calls))
    assert calls == [] and all(stats[k]["route"] == "host" for k in ref.files) and np.array_equal(got["data"].numpy(), ref["data"])
    with pytest.raises(ValueError):
        deflate.load_npz(path, device="cpu", foreign="gpu")
    # a CRC that does not match names the file and the member
    def wrong_crc(stream, nbytes, st):
        got, crc = _npz_inflater([])(stream, nbytes, st)
        return got, crc ^ 1
    with pytest.raises(ValueError, match="case.npz.*data"):
        deflate.load_npz(path, keys=["data"], device="cpu", inflater=wrong_crc, foreign="device")


# --------------------------------------------------------------------------------------------------------------------- .nii.gz
def nii_gz_bytes(array, datatype, extras=False, level=6, **fields):
    """a single-file NIfTI-1 of ``array`` as one gzip member; ``extras``: the member header carries FEXTRA, FNAME, FCOMMENT and FHCRC"""
    from tests import nifti_oracle
    body = nifti_oracle.build_header(array.shape, datatype, **fields) + b"\0\0\0\0" + np.ascontiguousarray(array).tobytes()
    plain = gzip.compress(body, level, mtime=0)
    if not extras:
        return plain
    extra = b"AB\x03\x00xyz"
    head = b"\x1f\x8b\x08" + bytes([2 | 4 | 8 | 16]) + plain[4:10] + struct.pack("<H", len(extra)) + extra + b"case.nii\x00" + b"note\x00"
    return head + struct.pack("<H", zlib.crc32(head) & 0xFFFF) + plain[10:]


def nii_volume(kind):
    """24 x 40 x 48: an int16 image (CT-like) or a uint8 label file (runs)"""
    if kind == "image":
        return np.frombuffer(ct_like(24 * 40 * 48, 60), dtype=np.int16).reshape(24, 40, 48), 4
    return np.frombuffer(label_runs(24 * 40 * 48, 61), dtype=np.uint8).reshape(24, 40, 48), 2


def _nifti_inflater(stream, total):
    from e2enet_medical_amd import deflate
    got = deflate.inflate_any(stream, total, **hooks())                 # (the default segment and cap)
    assert got is not None
    return got, zlib.crc32(got.tobytes())


@pytest.mark.parametrize("extras", [False, True])
def test_read_raw_device_route_through_the_hooks(tmp_path, extras):
    from e2enet_medical_amd import nifti
    for kind in ("image", "labels"):
        vol, datatype = nii_volume(kind)
        path = str(tmp_path / ("%s.nii.gz" % kind))
        open(path, "wb").write(nii_gz_bytes(vol, datatype, extras, scl_slope=2.0, scl_inter=-3.0))
        host, dev = nifti.read_raw(path), nifti.read_raw(path, inflate="device")
        assert isinstance(dev.payload, nifti.DeferredPayload) and dev.payload.size == host.payload.size == vol.nbytes
        assert dev.payload.offset == 352 and dev.payload.total == 352 + vol.nbytes
        assert dev._replace(payload=None) == host._replace(payload=None)
        got = nifti.resolve_payload(dev, inflater=_nifti_inflater)
        assert got.numpy().tobytes() == host.payload.tobytes() == vol.tobytes()
        with pytest.raises(ValueError, match="%s.nii.gz.*CRC" % kind):
            nifti.resolve_payload(dev, inflater=lambda s, t: (_nifti_inflater(s, t)[0], 1))
        # where inflate_any says None the host route reads the file
        assert nifti.resolve_payload(dev, inflater=lambda s, t: (None, 0)).numpy().tobytes() == vol.tobytes()
    assert nifti.callbacks("host").reader is nifti.reader and nifti.callbacks("device").reader.keywords == {"inflate": "device"}
    with pytest.raises(ValueError):
        nifti.read_raw(path, inflate="gpu")


def test_read_raw_device_route_leaves_to_the_host_what_it_does_not_serve(tmp_path):
    """a second member, a truncated file, a plain .nii, a header the host refuses: the default route's result or refusal"""
    from e2enet_medical_amd import nifti
    vol, datatype = nii_volume("image")
    blob = nii_gz_bytes(vol, datatype)

    def both(name, data):
        path = str(tmp_path / name)
        open(path, "wb").write(data)
        out = []
        for inflate in ("host", "device"):
            try:
                raw = nifti.read_raw(path, inflate=inflate)
                out.append(("ok", raw._replace(payload=None), raw.payload.tobytes() if isinstance(raw.payload, np.ndarray) else None))
            except Exception as e:
                out.append((type(e), str(e)))
        return out
    two = both("two.nii.gz", blob + gzip.compress(b"behind", mtime=0))
    assert two[0] == two[1] and two[0][0] == "ok" and two[0][2] == vol.tobytes()
    cut = both("cut.nii.gz", blob[:349])
    assert cut[0] == cut[1] and cut[0][0] != "ok"
    half = both("half.nii.gz", blob[:len(blob) // 2])
    assert half[0] == half[1] and half[0][0] != "ok"
    plain = both("plain.nii", gzip.decompress(blob))
    assert plain[0] == plain[1] and plain[0][0] == "ok"
    short = both("short.nii.gz", nii_gz_bytes(vol[:20], datatype, dim=(3, 48, 40, 24, 1, 1, 1, 1)))
    assert short[0] == short[1] and short[0][0] is ValueError and "truncated" in short[0][1]
    bad = both("bad.nii.gz", nii_gz_bytes(vol, datatype, bitpix=8))
    assert bad[0] == bad[1] and bad[0][0] is ValueError and "bitpix" in bad[0][1]
    reserved = bytearray(blob)
    reserved[3] |= 0x20
    res = both("reserved.nii.gz", bytes(reserved))
    assert res[0] == res[1]


# ------------------------------------------------------------------------------------------------------------------- the flags
def test_the_command_lines_refuse_inflate_any_where_it_does_nothing():
    from e2enet_medical_amd import crop_and_fingerprint, evaluator, nifti, simple_main, simple_predict
    from e2enet_medical_amd.inference import ensemble_predictions
    from e2enet_medical_amd.postprocessing import consolidate_postprocessing
    from e2enet_medical_amd.experiment_planning import nnUNet_plan_and_preprocess
    need = ["-ref", "a", "-pred", "b", "-l", "1", "2"]
    with pytest.raises(ValueError, match="--inflate_any.*--native_nifti"):
        evaluator.select_reader(evaluator.build_parser().parse_args(need + ["--inflate_any"]))
    on = evaluator.select_reader(evaluator.build_parser().parse_args(need + ["--inflate_any", "--native_nifti"]))
    assert on.func is nifti.evaluator_reader and on.keywords == {"inflate": "device"}
    assert evaluator.select_reader(evaluator.build_parser().parse_args(need + ["--native_nifti"])) is nifti.evaluator_reader

    with pytest.raises(ValueError, match="--inflate_any"):
        simple_predict.select_callbacks(simple_predict.build_parser().parse_args(["--inflate_any"]))
    reader, writer = simple_predict.select_callbacks(simple_predict.build_parser().parse_args(["--inflate_any", "--native_nifti"]))
    assert reader.func is nifti.reader and reader.keywords == {"inflate": "device"} and writer is nifti.writer

    with pytest.raises(ValueError, match="--inflate_any"):
        crop_and_fingerprint.select_reader(crop_and_fingerprint.build_parser().parse_args(["-t", "1", "--inflate_any"]))
    got = crop_and_fingerprint.select_reader(crop_and_fingerprint.build_parser().parse_args(["-t", "1", "--inflate_any", "--native_nifti"]))
    assert got.func is nifti.reader

    with pytest.raises(ValueError, match="--inflate_any"):
        consolidate_postprocessing.select_callbacks(consolidate_postprocessing.build_parser().parse_args(["-f", "x", "--inflate_any"]))
    kw = consolidate_postprocessing.select_callbacks(consolidate_postprocessing.build_parser().parse_args(["-f", "x", "--inflate_any", "--native_nifti"]))
    assert kw["reader"].keywords == {"inflate": "device"}

    with pytest.raises(ValueError, match="--inflate_any"):
        nnUNet_plan_and_preprocess.main(["-t", "999", "--inflate_any"])

    # the training: --resident_data gives the flag a meaning of its own; without either switch it is refused before any work
    with pytest.raises(SystemExit):
        simple_main.main(["--inflate_any"])
    args = simple_main.build_parser().parse_args(["--inflate_any", "--resident_data", "1"])
    assert simple_main.select_validation_callbacks(args) == (None, None)
    args = simple_main.build_parser().parse_args(["--inflate_any", "--native_nifti"])
    writer, gt = simple_main.select_validation_callbacks(args)
    assert writer is nifti.writer and gt.func is nifti.gt_reader and gt.keywords == {"inflate": "device"}

    # the ensembling: the flag implies --device_inflate and needs nothing else
    args = ensemble_predictions.build_parser().parse_args(["-f", "a", "b", "-o", "c", "--inflate_any"])
    assert args.inflate_any is True and args.device_inflate is False


def test_device_inflate_any_is_accepted_where_true_is():
    from e2enet_medical_amd import deflate
    from e2enet_medical_amd.training.dataloading.resident_loading import DeviceCaseCache
    assert deflate.foreign_of(False) is None and deflate.foreign_of(True) == "host" and deflate.foreign_of("any") == "device"
    with pytest.raises(ValueError):
        deflate.foreign_of("all")
    assert DeviceCaseCache(device_inflate="any").foreign == "device" and DeviceCaseCache(device_inflate="any").device_inflate is True
    assert DeviceCaseCache(device_inflate=True).foreign == "host" and DeviceCaseCache().device_inflate is False
    with pytest.raises(ValueError):
        DeviceCaseCache(device_inflate="every")
