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
and the device's with the GF(2) shift operator (``crc32_combine``; Python's zlib module does not export zlib's)."""
import argparse
import io
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
