"""Raw DEFLATE of device buffers (csrc/deflate.hip) and the two containers the package writes with it: a gzip member (``.nii.gz``)
and a ``.npz``.  Opt-in (``device_deflate=True`` / ``--device_deflate``, ``device_deflate="dynamic"`` / ``--dynamic_huffman``): the
default routes keep compressing on the host with zlib, byte for byte as before.

What the device writes is a valid but plain stream: chunks of ``chunk_bytes()`` bytes, each one Huffman block whose only matches
say "the same element again" (distance = the element size), or one stored block where that is shorter (include/e2e_hip.h states
the format; tests/test_gpu_deflate.py and tests/deflate_dynamic_oracle.py restate it in Python).  No search for other distances.
With ``codes="fixed"`` (``device_deflate=True``) the block uses the fixed code: a constant background shrinks about 150-fold, noisy
values do not shrink at all.  With ``codes="dynamic"`` every chunk gets a Huffman code built from its own tokens and is written in
the shortest of the three forms: values whose bytes are unevenly distributed (floating point, labels) shrink about as far as zlib's
Huffman coding takes them.  What either saves is the download of the uncompressed volume and the host's single-threaded pass
over it; only compressed bytes cross the link.

A container member is ``host prefix + device buffer``: the prefix (a NIfTI header, a ``.npy`` header) goes through host zlib as a raw
stream ended with a sync flush, which leaves it byte-aligned and not final; the device's chunks follow, every one byte-aligned and not
final; ``03 00`` -- an empty final fixed-Huffman block -- closes the stream.  The CRC-32 of the member is combined from the prefix's
and the device's with the GF(2) shift operator (``crc32_combine``; Python's zlib module does not export zlib's).

The way back is here too (csrc/inflate.hip; opt-in, ``device_inflate=True`` / ``--device_inflate``): ``inflate`` turns the device
part of a member into a device tensor, one wave per chunk, and ``load_npz`` is ``np.load`` for the ``.npz`` files written above,
with every other member read by ``np.load`` itself."""
import argparse
import io
import re
import struct
import zlib

import numpy as np

STREAM_END = b"\x03\x00"                 # BFINAL 1, BTYPE 01, end of block
GZIP_HEADER = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff"       # deflate, no flags, mtime 0, XFL 0, OS unknown: what nifti.write stores
PREFIX_LEVEL = 6
ZIP_DATE_TIME = (1980, 1, 1, 0, 0, 0)    # the fixed stamp of every archive member (preprocessing.save_npz uses the same)
_POLY = 0xEDB88320


# ------------------------------------------------------------------------------------------------------------------------ CRC-32
def _mulmod(a, b):
    """a(x) b(x) mod the CRC-32 polynomial, reflected (bit 31 is x^0): zlib's multmodp"""
    p = 0
    for i in range(32):
        if a & (0x80000000 >> i):
            p ^= b
        b = (b >> 1) ^ _POLY if b & 1 else b >> 1
    return p


def _xpow(nbits):
    """x^nbits mod the polynomial"""
    p, sq = 0x80000000, 0x40000000
    while nbits:
        if nbits & 1:
            p = _mulmod(sq, p)
        sq = _mulmod(sq, sq)
        nbits >>= 1
    return p


def crc32_combine(crc_a, crc_b, len_b):
    """``zlib.crc32(a + b)`` from ``zlib.crc32(a)``, ``zlib.crc32(b)`` and ``len(b)``: the first CRC shifted by the length of the
    second part (multiplied by x^(8 len_b)), plus the second."""
    if len_b < 0:
        raise ValueError("crc32_combine: a length of %d" % len_b)
    return (_mulmod(_xpow(8 * int(len_b)), crc_a & 0xFFFFFFFF) ^ crc_b) & 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------------------------- device half
def chunk_bytes():
    """bytes per chunk of the device encoder (``e2e_deflate_chunk_bytes``)"""
    from ._lib import lib
    return int(lib().deflate_chunk_bytes())


def _as_device_bytes(tensor, elem, who):
    import torch
    if not isinstance(tensor, torch.Tensor) or not tensor.is_cuda:
        raise ValueError("%s: the buffer must be a device tensor (got %s)"
                         % (who, "a CPU tensor" if isinstance(tensor, torch.Tensor) else type(tensor).__name__))
    if not tensor.is_contiguous():
        raise ValueError("%s: the tensor is not contiguous (shape %s, strides %s)" % (who, tuple(tensor.shape), tuple(tensor.stride())))
    nbytes = tensor.numel() * tensor.element_size()
    elem = tensor.element_size() if elem is None else int(elem)
    if elem not in (1, 2, 4, 8):
        raise ValueError("%s: elem %r is not 1, 2, 4 or 8" % (who, elem))
    if nbytes % elem:
        raise ValueError("%s: elem %d does not divide the %d bytes of the buffer" % (who, elem, nbytes))
    return nbytes, elem


CODES = ("fixed", "dynamic")
STORED, FIXED, DYNAMIC = 0, 1, 2         # what ``chunk_kinds`` reports per chunk


def check_codes(codes, who="deflate"):
    if codes not in CODES:
        raise ValueError("%s: codes %r is neither 'fixed' nor 'dynamic'" % (who, codes))
    return codes


def codes_of(device_deflate, who="device_deflate"):
    """The ``device_deflate`` argument of the writers as ``codes``: ``True`` is the fixed code, ``"dynamic"`` the per-chunk code
    (``"fixed"`` is accepted too); a false value is None, the host route."""
    if not device_deflate:
        return None
    if device_deflate is True:
        return "fixed"
    if device_deflate in CODES:
        return device_deflate
    raise ValueError("%s=%r: True, 'fixed', 'dynamic' or False" % (who, device_deflate))


def raw_deflate(tensor, elem=None, codes="fixed"):
    """``(stream, crc32, nbytes)`` of a contiguous device tensor: its bytes as a raw DEFLATE stream that is complete (ends with the
    final block), ``zlib.crc32`` of the bytes, and their number.  ``elem``: the distance of the matches, 1, 2, 4 or 8 bytes and a
    divisor of the byte count; default the tensor's element size.  ``codes``: ``"fixed"`` or ``"dynamic"`` (a Huffman code per
    chunk).  The stream depends on the bytes, ``elem`` and ``codes`` only.  Only the compressed bytes and one CRC word are
    downloaded."""
    body, crc, nbytes = _raw_body(tensor, elem, "raw_deflate", codes)
    return body + STREAM_END, crc, nbytes


def chunk_kinds(tensor, elem=None, codes="dynamic"):
    """The form of every chunk of ``raw_deflate(tensor, elem, codes)`` as a uint8 array: 0 stored, 1 fixed, 2 dynamic.  For the
    fixed codes the form is read off the chunk's first byte (a stored block begins with a zero byte)."""
    return _raw_body(tensor, elem, "chunk_kinds", codes, want_kinds=True)[3]


def _raw_body(tensor, elem, who, codes="fixed", want_kinds=False):
    """the chunks without the closing block"""
    import torch
    from ._lib import lib
    check_codes(codes, who)
    nbytes, elem = _as_device_bytes(tensor, elem, who)
    L = lib()
    st = torch.cuda.current_stream(tensor.device).cuda_stream
    with torch.cuda.device(tensor.device):
        chunk, slot = int(L.deflate_chunk_bytes()), int(L.deflate_slot_bytes())
        nchunks = -(-nbytes // chunk)
        crc = torch.empty(1, dtype=torch.int32, device=tensor.device)
        if nchunks == 0:
            L.deflate_encode(None, 0, elem, None, None, None, crc.data_ptr(), st)
            return (b"", int(crc.item()) & 0xFFFFFFFF, 0) + ((np.zeros(0, dtype=np.uint8),) if want_kinds else ())
        slots = torch.empty(nchunks * slot, dtype=torch.uint8, device=tensor.device)
        counts = torch.empty(nchunks, dtype=torch.int32, device=tensor.device)
        chunk_crcs = torch.empty(nchunks, dtype=torch.int32, device=tensor.device)
        kinds = None
        if codes == "dynamic":
            kinds = torch.empty(nchunks, dtype=torch.uint8, device=tensor.device)
            L.deflate_encode_dynamic(tensor.data_ptr(), nbytes, elem, slots.data_ptr(), counts.data_ptr(), kinds.data_ptr(),
                                     chunk_crcs.data_ptr(), crc.data_ptr(), st)
        else:
            L.deflate_encode(tensor.data_ptr(), nbytes, elem, slots.data_ptr(), counts.data_ptr(), chunk_crcs.data_ptr(),
                             crc.data_ptr(), st)
        ends = torch.cumsum(counts, 0, dtype=torch.int64)                 # 64-bit offsets: 4 GiB and more by construction
        offsets = (ends - counts).contiguous()
        total = int(ends[-1].item())
        out = torch.empty(total, dtype=torch.uint8, device=tensor.device)
        L.deflate_gather(slots.data_ptr(), counts.data_ptr(), offsets.data_ptr(), nchunks, out.data_ptr(), total, st)
        body = out.cpu().numpy().tobytes()
        if not want_kinds:
            return body, int(crc.item()) & 0xFFFFFFFF, nbytes
        if kinds is None:
            kinds = (out[offsets] != 0).to(torch.uint8)
        return body, int(crc.item()) & 0xFFFFFFFF, nbytes, kinds.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------- members
def deflate_prefix(prefix):
    """The host part of a member as a raw stream that is byte-aligned and not final (a sync flush)"""
    if not prefix:
        return b""
    c = zlib.compressobj(PREFIX_LEVEL, zlib.DEFLATED, -15)
    return c.compress(bytes(prefix)) + c.flush(zlib.Z_SYNC_FLUSH)


def member_stream(prefix, body, body_crc, body_len):
    """``(raw stream, crc32, length)`` of ``prefix + buffer``, where ``body`` holds the buffer as byte-aligned non-final blocks (the
    device's chunks) and ``body_crc`` / ``body_len`` are the buffer's CRC-32 and length"""
    prefix = bytes(prefix)
    crc = crc32_combine(zlib.crc32(prefix), body_crc, body_len)
    return deflate_prefix(prefix) + body + STREAM_END, crc, len(prefix) + int(body_len)


def gzip_bytes(stream, crc, length):
    """one gzip member around a complete raw stream"""
    return GZIP_HEADER + stream + struct.pack("<II", crc & 0xFFFFFFFF, length & 0xFFFFFFFF)


def gzip_member(host_prefix, tensor, codes="fixed"):
    """The bytes of a ``.gz`` file that inflates to ``host_prefix`` followed by the bytes of the device tensor: the header
    ``nifti.write`` stores (mtime 0, no name), the prefix through host zlib, the device's stream (``codes`` as in ``raw_deflate``),
    CRC-32 and length (mod 2^32) of the whole."""
    body, crc, nbytes = _raw_body(tensor, None, "gzip_member", codes)
    return gzip_bytes(*member_stream(host_prefix, body, crc, nbytes))


# -------------------------------------------------------------------------------------------------------------------------- npz
_TORCH_TO_NUMPY = {"torch.uint8": "u1", "torch.int8": "i1", "torch.int16": "i2", "torch.int32": "i4", "torch.int64": "i8",
                   "torch.float16": "f2", "torch.float32": "f4", "torch.float64": "f8", "torch.bool": "?"}


def npy_header(dtype, shape):
    """the ``.npy`` header (version 1.0) of a C-contiguous array"""
    f = io.BytesIO()
    np.lib.format.write_array_header_1_0(f, {"descr": np.lib.format.dtype_to_descr(np.dtype(dtype)), "fortran_order": False,
                                             "shape": tuple(int(v) for v in shape)})
    return f.getvalue()


def _dos_stamp(date_time=ZIP_DATE_TIME):
    y, mo, d, h, mi, s = date_time
    return (h << 11) | (mi << 5) | (s // 2), ((y - 1980) << 9) | (mo << 5) | d


def zip_bytes_parts(members):
    """The pieces of a zip archive of deflated members ``(name, raw stream, crc32, uncompressed length)``, to be written one after
    the other.  Laid out as numpy's ``savez`` leaves an archive (``ZipFile.open(..., force_zip64=True)``): version 4.5, sizes in a
    zip64 extra field of every local header and every directory entry, no data descriptors; a zip64 end record when the directory
    lies behind 4 GiB.  The date is fixed: an archive depends on its members alone."""
    dostime, dosdate = _dos_stamp()
    parts, directory, offset = [], [], 0
    for name, stream, crc, length in members:
        fname = name.encode("utf-8")
        flags = 0x800 if any(b > 127 for b in fname) else 0
        extra = struct.pack("<HHQQ", 1, 16, length, len(stream))
        local = struct.pack("<IHHHHHIIIHH", 0x04034B50, 45, flags, 8, dostime, dosdate, crc & 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF,
                            len(fname), len(extra)) + fname + extra
        cextra = struct.pack("<HHQQQ", 1, 24, length, len(stream), offset)
        directory.append(struct.pack("<IHHHHHHIIIHHHHHII", 0x02014B50, 45 | (3 << 8), 45, flags, 8, dostime, dosdate,
                                     crc & 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, len(fname), len(cextra), 0, 0, 0, 0o600 << 16,
                                     0xFFFFFFFF) + fname + cextra)
        parts += [local, stream]
        offset += len(local) + len(stream)
    cd = b"".join(directory)
    parts.append(cd)
    n = len(directory)
    if offset >= 0xFFFFFFFF or len(cd) >= 0xFFFFFFFF or n >= 0xFFFF:
        parts.append(struct.pack("<IQHHIIQQQQ", 0x06064B50, 44, 45, 45, 0, 0, n, n, len(cd), offset))
        parts.append(struct.pack("<IIQI", 0x07064B50, 0, offset + len(cd), 1))
    parts.append(struct.pack("<IHHHHIIH", 0x06054B50, 0, 0, min(n, 0xFFFF), min(n, 0xFFFF), min(len(cd), 0xFFFFFFFF),
                             min(offset, 0xFFFFFFFF), 0))
    return parts


def _npz_path(path):
    path = str(path)
    return path if path.endswith(".npz") else path + ".npz"          # (np.savez's rule)


def _member_parts(members):
    return zip_bytes_parts([(key + ".npy", stream, crc, length) for key, stream, crc, length in members])


def write_npz(path, members):
    """``members``: ``(key, raw stream, crc32, length)`` of ``<key>.npy`` each"""
    write_parts(path, _member_parts(members))


def write_parts(path, parts):
    """what ``npz_parts`` returned, written to ``path`` (``.npz`` appended where it is missing): the half of ``savez`` that needs no
    device, for a writer thread"""
    with open(_npz_path(path), "wb") as f:
        for part in parts:
            f.write(part)


def savez(path, codes="fixed", **arrays):
    """``np.savez_compressed(path, **arrays)`` with the arrays deflated on the device: a ``.npz`` that ``np.load`` reads.  A member
    is the ``.npy`` header (host prefix) and the array's bytes (device stream, ``codes`` as in ``raw_deflate``; an array cannot be
    called ``codes``).  Device tensors never reach the host uncompressed; host arrays are uploaded first.  Every array is
    C-contiguous (a non-contiguous device tensor is a ValueError)."""
    write_parts(path, npz_parts(codes=codes, **arrays))


def npz_parts(codes="fixed", **arrays):
    """The byte strings ``savez`` writes one after the other, without writing them: the thread that owns the GPU compresses, and any
    other thread can write (``write_parts``).  The bytes depend on the arrays, their order and ``codes`` alone."""
    import torch
    check_codes(codes, "deflate.savez")
    members = []
    for key, a in arrays.items():
        if not isinstance(a, torch.Tensor):
            a = torch.from_numpy(np.asarray(a, order="C"))
        if not a.is_cuda:
            if not torch.cuda.is_available():
                raise RuntimeError("deflate.savez: arrays are deflated on the GPU (csrc/deflate.hip); there is no host fallback")
            a = a.contiguous().to("cuda")
        if str(a.dtype) not in _TORCH_TO_NUMPY:
            raise ValueError("deflate.savez: %s: dtype %s has no .npy descr" % (key, a.dtype))
        body, crc, nbytes = _raw_body(a, None, "deflate.savez(%s)" % key, codes)
        members.append((key,) + member_stream(npy_header(_TORCH_TO_NUMPY[str(a.dtype)], a.shape), body, crc, nbytes))
    return _member_parts(members)


# ---------------------------------------------------------------------------------------------------------------------- inflate
# The way back (csrc/inflate.hip): what the device wrote is a sequence of byte-aligned chunk records that need nothing from each
# other but the 8 bytes in front of them, so the device inflates them one wave each.  The stream carries no index of where records
# start.  The host therefore proposes candidate offsets, ``e2e_inflate_scan`` parses one record at each, and the chain of valid
# records is walked from offset 0 on the downloaded table.  A stream that is not this encoder's fails one of the checks before
# anything is written, and ``inflate`` returns None: the caller inflates on the host, with the same result.
CHUNK = 32768                            # e2e_deflate_chunk_bytes(), asserted where the library is loaded
TAIL = 8                                 # bytes in front of a record that its matches may read (distances 1, 2, 4, 8)
RECORD_WORDS = 8                         # one scan record (include/e2e_hip.h, N8)
DEP_VALUE = 15                           # a nibble of a record's tail descriptor: the byte is a value, not a byte of the tail before
_MARKER = re.compile(b"\x00\x00\xff\xff")          # the empty stored block that closes a Huffman record (and whatever looks like it)


def candidate_cap(nbytes, chunk=CHUNK):
    """how many candidate starts ``inflate`` scans at most: 8 per record and 64"""
    return 8 * (-(-int(nbytes) // chunk)) + 64


def candidate_starts(stream, nbytes, chunk=CHUNK):
    """Sorted offsets at which a record may start, or None when there are more than ``candidate_cap``: offset 0, the byte behind
    every ``00 00 FF FF``, and transitively the byte behind every candidate that looks like a stored block (first byte 0, LEN =
    ~NLEN, 0 < LEN <= chunk): a stored record is not followed by the marker, so the record behind it is found only this way."""
    n, cap = len(stream), candidate_cap(nbytes, chunk)
    if n == 0:
        return []
    found = {0}
    for m in _MARKER.finditer(stream):
        if m.end() < n:
            found.add(m.end())
            if len(found) > cap:
                return None
    first = np.fromiter(found, dtype=np.int64, count=len(found))
    view = stream if isinstance(stream, np.ndarray) else np.frombuffer(stream, dtype=np.uint8)
    todo = first[view[first] == 0].tolist()            # (only a candidate whose first byte is 0 can look like a stored block)
    while todo:
        s = todo.pop()
        head = bytes(stream[s:s + 5])
        if len(head) < 5 or head[0] != 0:
            continue
        length, nlength = struct.unpack("<HH", head[1:])
        t = s + 5 + length
        if length == (~nlength & 0xFFFF) and 0 < length <= chunk and t < n and t not in found:
            found.add(t)
            todo.append(t)
            if len(found) > cap:
                return None
    return sorted(found)


def unpack_record(words):
    """one scan record as a dict: ``ok``, and for a valid record ``kind``, ``d``, ``reach``, ``length``, ``end`` and ``tail``, the
    last 8 output bytes oldest first, each ``(value, None)`` or ``(None, j)`` = byte j of the 8 bytes in front of the record"""
    w = [int(v) for v in words]
    if w[0] != 0:
        return {"ok": False}
    vals = struct.pack("<II", w[5], w[6])
    deps = [(w[7] >> (4 * i)) & 15 for i in range(TAIL)]
    return {"ok": True, "kind": w[1] & 0xFF, "d": (w[1] >> 8) & 0xFF, "reach": (w[1] >> 16) & 0xFF, "length": w[2],
            "end": w[3] | (w[4] << 32), "tail": [(vals[i], None) if deps[i] == DEP_VALUE else (None, deps[i]) for i in range(TAIL)]}


def inflate_plan(stream, nbytes, scan, chunk=CHUNK):
    """The host half of ``inflate``: ``(starts int64 [n], prev_tails uint8 [n, 8], candidates)`` of the n = ceil(nbytes / chunk)
    records of ``stream``, or None when the stream is not a chain of this encoder's records: too many candidates, a record that is
    invalid or missing where the one before ends, a record whose output is not a whole chunk (the last: the remainder), a first
    record that reads in front of itself, a chain that does not end with the stream.  ``scan(stream, starts) -> uint32 [len(starts),
    8]`` parses one record per candidate (the device's ``e2e_inflate_scan``; ``tests/inflate_oracle.py`` without one).
    prev_tails[k] are the 8 bytes in front of record k: the tail descriptors resolved with a forward fill per byte index."""
    nbytes = int(nbytes)
    nrec = -(-nbytes // chunk)
    if nbytes < 0 or (nbytes == 0) != (len(stream) == 0):
        return None
    if nbytes == 0:
        return np.zeros(0, dtype=np.int64), np.zeros((0, TAIL), dtype=np.uint8), 0
    cands = candidate_starts(stream, nbytes, chunk)
    if cands is None:
        return None
    cands = np.asarray(cands, dtype=np.int64)
    ncand = len(cands)
    table = np.ascontiguousarray(np.asarray(scan(stream, cands), dtype=np.uint32).reshape(ncand, RECORD_WORDS))
    # the chain: every valid record points at the candidate that is its end (whole arrays; the walk itself is a loop over ints)
    ok = table[:, 0] == 0
    ends = table[:, 3].astype(np.int64) | (table[:, 4].astype(np.int64) << 32)
    at = np.minimum(np.searchsorted(cands, ends), ncand - 1)
    follower = np.where(ok & (cands[at] == ends), at, -1).tolist()
    chain, i = [], 0                                  # (candidate 0 is offset 0)
    for k in range(nrec):
        if i < 0 or not ok[i]:
            return None
        chain.append(i)
        i = follower[i]
    chain = np.asarray(chain, dtype=np.int64)
    lengths = table[chain, 2].astype(np.int64)
    if (lengths[:-1] != chunk).any() or lengths[-1] != nbytes - (nrec - 1) * chunk or ends[chain[-1]] != len(stream) \
            or (table[chain[0], 1] >> 16) & 0xFF:
        return None
    # the tails: values where the record has them; a dependent byte takes byte j of the resolved tail in front (records in order)
    resolved = np.ascontiguousarray(table[chain, 5:7]).view(np.uint8).reshape(nrec, TAIL).copy()
    deps = (table[chain, 7][:, None] >> (4 * np.arange(TAIL, dtype=np.uint32))[None, :]) & 15
    rows = np.flatnonzero((deps != DEP_VALUE).any(axis=1)).tolist()
    if rows:
        res, dep = resolved.tolist(), deps.tolist()
        for k in rows:
            front = res[k - 1] if k else [0] * TAIL
            res[k] = [v if j == DEP_VALUE else front[j & 7] for v, j in zip(res[k], dep[k])]
        resolved = np.asarray(res, dtype=np.uint8).reshape(nrec, TAIL)
    tails = np.zeros((nrec, TAIL), dtype=np.uint8)
    tails[1:] = resolved[:-1]
    return cands[chain], tails, ncand


def _byte_array(stream):
    """the stream as a writable uint8 array (torch.from_numpy does not take a read-only one silently)"""
    a = stream if isinstance(stream, np.ndarray) else np.frombuffer(stream, dtype=np.uint8)
    if a.dtype != np.uint8 or a.ndim != 1 or not a.flags.c_contiguous:
        raise ValueError("inflate: the stream must be bytes or a contiguous uint8 array")
    return a if a.flags.writeable else a.copy()


def inflate(stream, nbytes, device="cuda", stats=None, scan=None, chunks=None):
    """The ``nbytes`` bytes that the chunk records ``stream`` inflate to, as a uint8 device tensor; ``stream`` is what
    ``raw_deflate`` returns without its closing ``03 00`` (the device part of a member).  None when the stream is not a chain of
    this encoder's records (``inflate_plan``); nothing has been written then and host zlib gives the result.  A ValueError when a
    record of the chain turns out corrupt on the second, writing pass (``e2e_inflate_chunks`` trusts nothing of the scan).
    ``stats`` (a dict) receives ``candidates`` and ``records``.  ``scan`` and ``chunks`` replace the two device steps (tests without
    a device): ``scan`` as in ``inflate_plan``, ``chunks(stream, starts, prev_tails, nbytes) -> the result``."""
    nbytes = int(nbytes)
    data = _byte_array(stream)
    dev = {}

    def upload():
        import torch
        from ._lib import lib
        if "comp" not in dev:
            dev["lib"], dev["torch"] = lib(), torch
            assert int(dev["lib"].deflate_chunk_bytes()) == CHUNK and int(dev["lib"].inflate_record_words()) == RECORD_WORDS
            dev["comp"] = torch.from_numpy(data).to(device)
            dev["stream"] = torch.cuda.current_stream(dev["comp"].device).cuda_stream
        return dev["lib"], dev["torch"], dev["comp"], dev["stream"]

    def device_scan(_, starts):
        L, torch, comp, st = upload()
        with torch.cuda.device(comp.device):
            starts_d = torch.from_numpy(starts).to(comp.device)
            records = torch.empty((len(starts), RECORD_WORDS), dtype=torch.int32, device=comp.device)
            L.inflate_scan(comp.data_ptr(), comp.numel(), starts_d.data_ptr(), len(starts), records.data_ptr(), st)
            return records.cpu().numpy().view(np.uint32)

    def device_chunks(_, starts, tails, nbytes):
        L, torch, comp, st = upload()
        with torch.cuda.device(comp.device):
            out = torch.empty(nbytes, dtype=torch.uint8, device=comp.device)
            status = torch.empty(1, dtype=torch.int32, device=comp.device)
            starts_d, tails_d = torch.from_numpy(starts).to(comp.device), torch.from_numpy(tails).to(comp.device)
            L.inflate_chunks(comp.data_ptr() if len(starts) else None, comp.numel(), starts_d.data_ptr() if len(starts) else None,
                             tails_d.data_ptr() if len(starts) else None, len(starts), out.data_ptr() if nbytes else None, nbytes,
                             status.data_ptr(), st)
            bad = int(status.item())
            if bad:
                raise ValueError("inflate: %d of %d records are corrupt" % (bad, len(starts)))
            return out

    plan = inflate_plan(data, nbytes, device_scan if scan is None else scan)
    if plan is None:
        return None
    starts, tails, ncand = plan
    if stats is not None:
        stats["candidates"], stats["records"] = ncand, len(starts)
    return (device_chunks if chunks is None else chunks)(data, starts, tails, nbytes)


# ------------------------------------------------------------------------------------------------------------------ inflate any
# Any raw DEFLATE stream (csrc/inflate_any.hip; opt-in).  The compressed bytes are cut into segments; ``e2e_inflate_find`` reports
# the first valid non-final dynamic block header of every segment; the stream is cut into spans at those bit positions; the spans
# are counted, then decoded into 16-bit symbols (a byte, or "byte j of the 32 KiB in front of this span"), the windows are handed
# down the chain of spans and the markers replaced.  The host sees three small tables: the starts, the span records, the offsets.
WINDOW = 32768
SPAN_RECORD_WORDS = 8                    # one record of e2e_inflate_spans_count (include/e2e_hip.h, N9)
SEGMENT_BYTES = 16384                    # default segment: zlib at its default settings starts a dynamic block every 15-25 KiB
SPAN_STATUS = ("good", "BTYPE 11", "a block header rule", "a bit pattern without a symbol", "a symbol over 285",
               "a distance code over 29", "stored LEN != ~NLEN", "BFINAL before the end of the stream", "a block runs behind the stream",
               "overshoot", "a span over the cap", "length", "a reach in front of the output", "a start outside the stream")
OVERSHOOT = 9


def span_gaps(starts, n):
    """bits from every start to the next, the last to the end of the ``n`` compressed bytes"""
    return np.diff(np.concatenate([np.asarray(starts, dtype=np.int64), [8 * int(n)]]))


def unpack_span_records(records):
    """``(status, final, end bit, output length)`` of span records as int64 arrays"""
    r = np.asarray(records, dtype=np.uint32).reshape(-1, SPAN_RECORD_WORDS).astype(np.int64)
    return r[:, 0], r[:, 1], r[:, 2] | (r[:, 3] << 32), r[:, 4] | (r[:, 5] << 32)


def inflate_any(stream, nbytes, device="cuda", segment_bytes=None, max_span_bytes=None, stats=None, find=None, count=None, write=None):
    """The ``nbytes`` bytes that the raw DEFLATE stream ``stream`` (RFC 1951, any encoder's) inflates to, as a uint8 device tensor.
    ``stream``: bytes, a uint8 array, or a uint8 device tensor, which is used as it is.  ``segment_bytes`` (S >= 16, default
    ``SEGMENT_BYTES``): the stream is searched for one block start per S compressed bytes.  ``max_span_bytes`` (default 8 S): no
    span of more compressed bytes is ever decoded by one wave.

    None -- take the host route, which gives the default's result or the default's error -- when a gap between two starts is over
    the cap (a stream of stored or fixed blocks only has no start at all), a span has a status (a start that is no block start ends
    in ``overshoot``), the counted lengths do not sum to ``nbytes``, or the last span does not end with the final block at the
    stream's end.  All of that is decided on the count pass: nothing has been written.  A status of the writing kernels after a clean
    count pass is a ValueError.  ``stats`` (a dict) receives ``starts`` (found by the search), ``spans``, ``largest_gap`` (bits),
    ``sym_bytes``, ``window_bytes`` and ``refused`` (None, or the rule that said None).

    ``find(data, S) -> int64 [ceil(n / S)]``, ``count(data, starts, cap) -> uint32 [m, 8]`` and ``write(data, starts, offs, cap,
    nbytes) -> the result`` replace the device steps (tests without a device; tests/inflate_any_oracle.py)."""
    nbytes = int(nbytes)
    S = SEGMENT_BYTES if segment_bytes is None else int(segment_bytes)
    cap = 8 * S if max_span_bytes is None else int(max_span_bytes)
    if S < 16 or cap < 1 or nbytes < 0:
        raise ValueError("inflate_any: segment_bytes %d (at least 16), max_span_bytes %d (at least 1), nbytes %d" % (S, cap, nbytes))
    hooks = (find, count, write)
    on_device = not isinstance(stream, (bytes, bytearray, memoryview, np.ndarray))
    dev = {}

    def host_bytes():
        if "data" not in dev:
            dev["data"] = stream.cpu().numpy() if on_device else _byte_array(stream)
        return dev["data"]

    def upload():
        import torch
        from ._lib import lib
        if "comp" not in dev:
            L = lib()
            assert int(L.inflate_any_record_words()) == SPAN_RECORD_WORDS and int(L.inflate_any_window_bytes()) == WINDOW
            if on_device:
                nb, _ = _as_device_bytes(stream, 1, "inflate_any")
                if stream.dtype != torch.uint8 or stream.dim() != 1:
                    raise ValueError("inflate_any: a device stream is a one-dimensional uint8 tensor")
                comp = stream
            else:
                comp = torch.from_numpy(host_bytes()).to(device)
            dev.update(lib=L, torch=torch, comp=comp, stream=torch.cuda.current_stream(comp.device).cuda_stream)
        return dev["lib"], dev["torch"], dev["comp"], dev["stream"]

    def device_find(_, seg):
        L, torch, comp, st = upload()
        with torch.cuda.device(comp.device):
            nseg = -(-comp.numel() // seg)
            starts_d = torch.full((max(nseg, 1),), -1, dtype=torch.int64, device=comp.device)
            L.inflate_find(comp.data_ptr(), comp.numel(), seg, nseg, starts_d.data_ptr(), st)
            return starts_d.cpu().numpy()

    def device_count(_, starts, span_cap):
        L, torch, comp, st = upload()
        with torch.cuda.device(comp.device):
            dev["starts"] = torch.from_numpy(np.ascontiguousarray(starts, dtype=np.int64)).to(comp.device)
            records = torch.empty((len(starts), SPAN_RECORD_WORDS), dtype=torch.int32, device=comp.device)
            L.inflate_spans_count(comp.data_ptr(), comp.numel(), dev["starts"].data_ptr(), len(starts), span_cap, records.data_ptr(), st)
            return records.cpu().numpy().view(np.uint32)

    def device_write(_, starts, offs, span_cap, total):
        L, torch, comp, st = upload()
        with torch.cuda.device(comp.device):
            m = len(starts)
            out = torch.empty(total, dtype=torch.uint8, device=comp.device)
            if total == 0:
                return out
            starts_d = dev["starts"] if "starts" in dev else torch.from_numpy(np.ascontiguousarray(starts, dtype=np.int64)).to(comp.device)
            offs_d = torch.from_numpy(np.ascontiguousarray(offs, dtype=np.int64)).to(comp.device)
            sym = torch.empty(total, dtype=torch.int16, device=comp.device)
            wins = torch.empty(m * WINDOW, dtype=torch.uint8, device=comp.device) if m > 1 else None
            status = torch.empty(3, dtype=torch.int32, device=comp.device)
            L.inflate_spans_write(comp.data_ptr(), comp.numel(), starts_d.data_ptr(), offs_d.data_ptr(), m, span_cap, sym.data_ptr(),
                                  total, status[0:].data_ptr(), st)
            L.inflate_windows(sym.data_ptr(), offs_d.data_ptr(), m, total, wins.data_ptr() if m > 1 else None, status[1:].data_ptr(), st)
            L.inflate_resolve(sym.data_ptr(), offs_d.data_ptr(), m, wins.data_ptr() if m > 1 else None, out.data_ptr(), total,
                              status[2:].data_ptr(), st)
            bad = status.cpu().tolist()
            if any(bad):
                raise ValueError("inflate_any: the writing pass found %d corrupt spans of %d (windows: %d, markers: %d)"
                                 % (bad[0], m, bad[1], bad[2]))
            return out

    st = {} if stats is None else stats
    st.update(starts=0, spans=0, largest_gap=0, sym_bytes=0, window_bytes=0, refused=None)

    def refuse(rule):
        st["refused"] = rule
        return None

    if all(h is None for h in hooks):
        n = int(upload()[2].numel())
        data = None
    else:
        data = host_bytes()
        n = int(data.size)
    if n == 0:
        return refuse("an empty stream")
    found = np.array((device_find if find is None else find)(data, S), dtype=np.int64).reshape(-1)
    found[0] = 0                                       # the stream's first block starts at bit 0
    starts = found[found >= 0]
    gaps = span_gaps(starts, n)
    st.update(starts=len(starts) - 1, spans=len(starts), largest_gap=int(gaps.max()))
    if gaps.max() > 8 * cap or gaps.min() <= 0:
        return refuse("a gap of %d bits between block starts, over the cap of %d bytes" % (int(gaps.max()), cap))
    status, final, _, lengths = unpack_span_records((device_count if count is None else count)(data, starts, cap))
    if status.any():
        k = int(np.flatnonzero(status)[0])
        code = int(status[k])
        return refuse("span %d: %s" % (k, SPAN_STATUS[code] if code < len(SPAN_STATUS) else "status %d" % code))
    if not final[-1]:
        return refuse("the last span does not end with the final block")
    if int(lengths.sum()) != nbytes:
        return refuse("the spans inflate to %d bytes, not %d" % (int(lengths.sum()), nbytes))
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    st.update(sym_bytes=2 * nbytes, window_bytes=WINDOW * len(starts) if len(starts) > 1 else 0)
    return (device_write if write is None else write)(data, starts, offs, cap, nbytes)


def foreign_of(device_inflate, who="device_inflate"):
    """The ``device_inflate`` argument of the readers as the ``foreign`` argument of ``load_npz``: a false value is None (the host
    reads everything), ``True`` is ``"host"`` (only this package's members are inflated on the device, exactly as before),
    ``"any"`` is ``"device"`` (members of other writers go through ``inflate_any``)."""
    if not device_inflate:
        return None
    if device_inflate is True:
        return "host"
    if device_inflate == "any":
        return "device"
    raise ValueError("%s=%r: True, 'any' or False" % (who, device_inflate))


def device_crc32(tensor):
    """``zlib.crc32`` of the bytes of a contiguous device tensor (``e2e_crc32``: the encoder's two CRC kernels)"""
    import torch
    from ._lib import lib
    nbytes, _ = _as_device_bytes(tensor, 1, "device_crc32")
    with torch.cuda.device(tensor.device):
        crc = torch.empty(1, dtype=torch.int32, device=tensor.device)
        work = torch.empty(max(1, -(-nbytes // CHUNK)), dtype=torch.int32, device=tensor.device)
        lib().crc32(tensor.data_ptr() if nbytes else None, nbytes, work.data_ptr(), crc.data_ptr(),
                    torch.cuda.current_stream(tensor.device).cuda_stream)
        return int(crc.item()) & 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------------------------ reading npz
_NUMPY_TO_TORCH = {np.dtype(v): k for k, v in _TORCH_TO_NUMPY.items()}
_HEAD_WINDOW = 1 << 16                   # compressed bytes looked at for a member's .npy header


class NpzMember:
    """One ``<key>.npy`` of an archive as ``read_npz_raw`` found it.  ``stream`` is the member's raw DEFLATE stream (a view of the
    file's bytes).  ``body`` is the device part of it and ``header`` the .npy header in front when the member is laid out as this
    package's writers lay it out (``member_stream``); otherwise ``body`` is None and ``why`` says what was different."""

    def __init__(self, key, crc, size):
        self.key, self.crc, self.size = key, crc, size
        self.stream = self.body = self.header = self.foreign_header = self.dtype = self.shape = None
        self.nbytes = 0
        self.why = None


class NpzRaw:
    """what ``read_npz_raw`` returns: the file's bytes, and its members by key in directory order"""

    def __init__(self, path, data, members):
        self.path, self.data, self.members = path, data, members


def _npy_header(stream):
    """``(header bytes, dtype, shape, fortran_order)`` from the front of a member's raw stream, or None: the magic, the version and
    the header's own length are inflated under ``max_length``, so only the header is ever inflated on the host"""
    d = zlib.decompressobj(-15)
    try:
        head = d.decompress(bytes(stream[:_HEAD_WINDOW]), 10)
        if len(head) < 10 or head[:6] != b"\x93NUMPY" or head[6] not in (1, 2):
            return None
        if head[6] == 2:
            head += d.decompress(d.unconsumed_tail, 2)
            if len(head) < 12:
                return None
        total = len(head) + (struct.unpack("<H", head[8:10])[0] if head[6] == 1 else struct.unpack("<I", head[8:12])[0])
        if total > _HEAD_WINDOW:
            return None
        head += d.decompress(d.unconsumed_tail, total - len(head))
        if len(head) != total:
            return None
        f = io.BytesIO(head)
        version = np.lib.format.read_magic(f)
        shape, fortran, dtype = (np.lib.format.read_array_header_1_0 if version == (1, 0) else np.lib.format.read_array_header_2_0)(f)
    except (zlib.error, ValueError):
        return None
    return head, dtype, tuple(int(v) for v in shape), bool(fortran)


def read_npz_raw(path):
    """The host-only half of ``load_npz``, for a read-ahead thread (it shares no state and touches no device): the file's bytes, the
    zip directory, and per member the .npy header and where the device part of its stream lies."""
    import zipfile
    path = str(path)
    data = np.fromfile(path, dtype=np.uint8)
    members = {}
    with zipfile.ZipFile(path) as z:
        infos = z.infolist()
    for info in infos:
        key = info.filename[:-4] if info.filename.endswith(".npy") else info.filename
        m = members[key] = NpzMember(key, info.CRC, info.file_size)
        o = info.header_offset
        if o + 30 > data.size or bytes(data[o:o + 4]) != b"PK\x03\x04":
            raise ValueError("%s: member %s has no local header at %d" % (path, key, o))
        name_len, extra_len = struct.unpack("<HH", bytes(data[o + 26:o + 30]))
        first = o + 30 + name_len + extra_len
        if first + info.compress_size > data.size:
            raise ValueError("%s: member %s runs past the end of the file" % (path, key))
        m.stream = data[first:first + info.compress_size]
        if info.compress_type != zipfile.ZIP_DEFLATED or not info.filename.endswith(".npy"):
            m.why = "not a deflated .npy member"
            continue
        parsed = _npy_header(m.stream)
        if parsed is None:
            m.why = "no .npy header of version 1 or 2 at the front of the stream"
            continue
        head, dtype, shape, fortran = parsed
        m.dtype, m.shape = dtype, shape
        m.nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        prefix = deflate_prefix(head)
        if fortran or dtype.hasobject or dtype not in _NUMPY_TO_TORCH:
            m.why = "Fortran order, or a dtype without a device tensor"
        elif len(head) + m.nbytes != info.file_size:
            m.why = "the member's length is not header + array"
        else:
            m.foreign_header = head                    # any encoder's member that holds a C-ordered array: inflate_any can take it
        if m.why is not None:
            pass
        elif m.stream.size < len(prefix) + len(STREAM_END) or bytes(m.stream[:len(prefix)]) != prefix:
            m.why = "the stream does not begin with the header as its own sync-flushed block"
        elif bytes(m.stream[-len(STREAM_END):]) != STREAM_END:
            m.why = "the stream does not end with 03 00"
        else:
            m.header, m.body = head, m.stream[len(prefix):m.stream.size - len(STREAM_END)]
    return NpzRaw(path, data, members)


def load_npz(path, keys=None, device="cuda", stats=None, inflater=None, foreign="host"):
    """``np.load(path)`` as a dict of device tensors, the members this package's writers deflated (``savez``, ``-z`` with
    ``--device_deflate``, stage folders) inflated on the device: only compressed bytes cross the link and the host inflates a few
    hundred header bytes.  ``path``: a file, or what ``read_npz_raw`` returned for it.  ``keys``: the members wanted, default all.
    Any other member (``np.savez_compressed``'s, a stored one, Fortran order, a stream with too many candidate offsets) takes
    ``np.load`` and an upload, with the same result -- unless ``foreign="device"``: then a deflated member of any other writer that
    holds a C-ordered array of a native dtype goes through ``inflate_any`` (the whole member, .npy header included; its length is the
    directory's), and only where that says None through ``np.load``.  A device-route member whose bytes do not give the directory's
    CRC-32, or whose chain has a corrupt record, is a ValueError that names the file and the member.  ``stats`` (a dict) receives
    per member ``route`` ("device" / "any" / "host"), ``candidates``, ``records``, ``compressed`` and ``inflated`` bytes, and for the
    members ``inflate_any`` was asked about its statistics under ``any``.  ``inflater`` replaces ``inflate`` / ``inflate_any`` and
    the CRC of the result: ``inflater(stream, nbytes, stats) -> (tensor or None, crc32)`` (tests without a device)."""
    import torch
    if foreign not in ("host", "device"):
        raise ValueError("load_npz: foreign=%r is neither 'host' nor 'device'" % (foreign,))
    raw = path if isinstance(path, NpzRaw) else read_npz_raw(path)
    missing = [k for k in (keys or ()) if k not in raw.members]
    if missing:
        raise KeyError("%s: no member %s (it holds %s)" % (raw.path, ", ".join(missing), ", ".join(raw.members)))
    out, host = {}, None

    def typed(flat, m):
        if not isinstance(flat, torch.Tensor):
            flat = torch.from_numpy(np.ascontiguousarray(flat))
        dtype = getattr(torch, _NUMPY_TO_TORCH[m.dtype][6:])
        if flat.data_ptr() % m.dtype.itemsize:
            flat = flat.clone()                        # (a header that is no multiple of the element size: one device copy)
        # (an empty tensor has no stride to view by)
        return flat.view(dtype).reshape(m.shape) if m.nbytes else torch.empty(m.shape, dtype=dtype, device=flat.device)

    for key in (raw.members if keys is None else keys):
        m = raw.members[key]
        st = {"route": "host", "candidates": 0, "records": 0, "compressed": int(m.stream.size), "inflated": int(m.size)}
        got = None
        try:
            if m.body is not None:
                if inflater is None:
                    got = inflate(m.body, m.nbytes, device, st)
                    crc = device_crc32(got) if got is not None else 0
                else:
                    got, crc = inflater(m.body, m.nbytes, st)
                if got is not None:
                    crc = crc32_combine(zlib.crc32(m.header), crc, m.nbytes)
                    st["route"] = "device"
            elif foreign == "device" and m.foreign_header is not None:
                if inflater is None:
                    got = inflate_any(m.stream, m.size, device, stats=st.setdefault("any", {}))
                    crc = device_crc32(got) if got is not None else 0
                else:
                    got, crc = inflater(m.stream, m.size, st)
                if got is not None:
                    got = got[len(m.foreign_header):]
                    st["route"] = "any"
        except ValueError as e:
            raise ValueError("%s: member %s: %s" % (raw.path, key, e)) from None
        if got is not None:
            if crc != m.crc:
                raise ValueError("%s: member %s: the inflated bytes do not give the CRC-32 of the directory (%08x)"
                                 % (raw.path, key, m.crc))
            if isinstance(got, torch.Tensor) or st["route"] == "any":
                got = typed(got, m)
        if got is None:
            if host is None:
                host = np.load(io.BytesIO(raw.data.tobytes()))
            got = torch.from_numpy(np.ascontiguousarray(host[key])).to(device)
        out[key] = got
        if stats is not None:
            stats[key] = st
    return out


class _DynamicHuffman(argparse.Action):
    """``--dynamic_huffman`` sets ``--device_deflate`` too"""

    def __call__(self, parser, namespace, values, option_string=None):
        namespace.dynamic_huffman = True
        namespace.device_deflate = True


def add_argument(parser, what=".npz class probabilities, .nii.gz of the native NIfTI writer"):
    """the ``--device_deflate`` and ``--dynamic_huffman`` switches of the command-line tools; ``from_args`` reads them"""
    parser.add_argument("--device_deflate", action="store_true", default=False,
                        help="compress what is written (%s) on the GPU and download only compressed bytes; default: download and "
                             "compress with zlib on the host" % what)
    parser.add_argument("--dynamic_huffman", action=_DynamicHuffman, nargs=0, default=False,
                        help="implies --device_deflate: every 32 KiB chunk gets a Huffman code built from its own bytes instead of "
                             "DEFLATE's fixed code (smaller files, floating-point data above all)")


def from_args(args):
    """the ``device_deflate`` argument of the writers from the parsed switches: False, True or ``"dynamic"``"""
    if getattr(args, "dynamic_huffman", False):
        return "dynamic"
    return bool(getattr(args, "device_deflate", False))
