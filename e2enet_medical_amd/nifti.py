"""Native NIfTI-1 input and output, opt-in (``--native_nifti`` of the command-line tools, or ``reader=nifti.reader`` and so on).

The host does what only the host can: gzip and the 348-byte header (``read_raw``, ``write``; numpy and the standard library, no
device).  The voxel payload is uploaded as the file stores it -- 1 to 8 bytes per voxel, in the file's byte order -- and decoded on
the device (csrc/nifti.hip) into the tensors the other kernels take: fp32 in a channel of the case's ``[C, Z, Y, X]`` tensor
(``decode_f32``, ``reader``) or the uint8 label volume of the census and component kernels (``decode_u8``, ``gt_reader``,
``evaluator_reader``).  ``scan`` reads the same bytes once for the dataset integrity check and brings back 260 words.

Read: single-file NIfTI-1 (``.nii``, ``.nii.gz``; magic ``n+1``, either byte order), three spatial dimensions (``dim[0]`` 3, or 4-7
with every further dimension 1), the ten scalar datatypes of ``DATATYPES``.  Everything else -- NIfTI-2, ``.hdr``/``.img`` pairs, RGB
and complex data, time series, a truncated payload -- is a ``ValueError`` that names the file and the field, raised on the host
before anything is uploaded.

Geometry is the NIfTI-1 standard's, reported the way ITK reports it (LPS): the qform when ``qform_code > 0``, else the sform when
``sform_code > 0``, else identity; ``itk_direction = diag(-1, -1, 1) R``, ``itk_origin = (-x, -y, z)``, lengths in millimetres.  The
voxel array is ``[dim3, dim2, dim1]`` exactly as stored; nothing is reoriented (``sitk.GetArrayFromImage``).  SimpleITK is not
available to check against: parity with ITK's NiftiImageIO is unpinned."""
import gzip
import math
import os
import struct
from collections import OrderedDict, namedtuple

import numpy as np

HEADER_BYTES = 348
GZIP_LEVEL = 6                      # of ``write``: with mtime 0 and no file name in the member, one volume gives one byte string
MM_PER_UNIT = {1: 1000., 2: 1., 3: 0.001}          # xyzt_units & 7: metre, millimetre, micron (0, unknown: taken as millimetres)

# NIfTI-1 datatype code -> (numpy kind and size, bytes per element): what csrc/nifti.hip decodes
DATATYPES = OrderedDict([(2, ("u1", 1)), (4, ("i2", 2)), (8, ("i4", 4)), (16, ("f4", 4)), (64, ("f8", 8)), (256, ("i1", 1)),
                         (512, ("u2", 2)), (768, ("u4", 4)), (1024, ("i8", 8)), (1280, ("u8", 8))])

# the header fields that are read: name -> (offset, struct format without the byte order)
_FIELDS = OrderedDict([("sizeof_hdr", (0, "i")), ("dim", (40, "8h")), ("datatype", (70, "h")), ("bitpix", (72, "h")),
                       ("pixdim", (76, "8f")), ("vox_offset", (108, "f")), ("scl_slope", (112, "f")), ("scl_inter", (116, "f")),
                       ("xyzt_units", (123, "B")), ("qform_code", (252, "h")), ("sform_code", (254, "h")),
                       ("quatern", (256, "3f")), ("qoffset", (268, "3f")), ("srow_x", (280, "4f")), ("srow_y", (296, "4f")),
                       ("srow_z", (312, "4f")), ("magic", (344, "4s"))])

NiftiRaw = namedtuple("NiftiRaw", "path shape datatype elsize swap scale slope inter payload itk_spacing itk_origin itk_direction")
NiftiRaw.__doc__ = """One file as ``read_raw`` leaves it on the host.
  shape          (dim3, dim2, dim1): the voxel array's, C-contiguous as stored
  datatype       NIfTI-1 code (a key of DATATYPES); elsize: bytes per element
  swap           the file's byte order is not the host's
  scale          apply ``value * slope + inter`` (off for scl_slope 0 or non-finite, and for slope 1 with inter 0)
  payload        uint8 host array of prod(shape) * elsize bytes: the voxels as the file stores them
  itk_spacing, itk_origin, itk_direction   what SimpleITK's GetSpacing / GetOrigin / GetDirection report (x, y, z; LPS; mm)"""

NiftiScan = namedtuple("NiftiScan", "nan_count first_nan non_label_count first_non_label histogram")
NiftiScan.__doc__ = """What ``scan`` says about a payload (fp32 values, the header's scaling applied).
  nan_count, first_nan              voxels that are NaN; raster index of the first, -1 without one
  non_label_count, first_non_label  voxels that are not NaN and no whole number in [0, 255]; raster index of the first, or -1
  histogram                         np.int64[256]: voxels per label value"""
SCAN_WORDS = 4 + 256


def _refuse(path, field, what):
    raise ValueError("%s: %s %s" % (path, field, what))


def _opener(path):
    low = path.lower()
    if low.endswith(".hdr") or low.endswith(".img") or low.endswith(".hdr.gz") or low.endswith(".img.gz"):
        _refuse(path, "file name", "is half of an Analyze / NIfTI .hdr/.img pair; only single-file .nii and .nii.gz are read")
    return (lambda: gzip.open(path, "rb")) if low.endswith(".gz") else (lambda: open(path, "rb"))


def _read_exact(f, n):
    """n bytes of a stream, fewer at its end"""
    parts, got = [], 0
    while got < n:
        b = f.read(n - got)
        if not b:
            break
        parts.append(b)
        got += len(b)
    return b"".join(parts)


def parse_header(hdr, path="<header>"):
    """The fields of ``_FIELDS`` of a 348-byte NIfTI-1 header as a dict, plus ``byteorder`` ('<' or '>').  Refuses NIfTI-2, a bad
    ``sizeof_hdr`` and a magic other than ``n+1``."""
    if len(hdr) < HEADER_BYTES:
        _refuse(path, "header", "has %d bytes, a NIfTI-1 header has %d" % (len(hdr), HEADER_BYTES))
    for order in "<>":
        size = struct.unpack_from(order + "i", hdr, 0)[0]
        if size == HEADER_BYTES:
            break
        if size == 540:
            _refuse(path, "sizeof_hdr", "is 540: a NIfTI-2 file, only NIfTI-1 is read")
    else:
        _refuse(path, "sizeof_hdr", "is %d, a NIfTI-1 header says 348 (in either byte order)" % struct.unpack_from("<i", hdr, 0)[0])
    h = {"byteorder": order}
    for name, (off, fmt) in _FIELDS.items():
        v = struct.unpack_from(order + fmt, hdr, off)
        h[name] = v[0] if len(v) == 1 else v
    magic = h["magic"]
    if magic == b"ni1\0":
        _refuse(path, "magic", "is 'ni1': the header of a .hdr/.img pair; only single-file NIfTI-1 ('n+1') is read")
    if magic != b"n+1\0":
        _refuse(path, "magic", "is %r, a single-file NIfTI-1 has 'n+1'" % (magic,))
    return h


def _quatern_to_mat(b, c, d, qfac):
    """nifti1.h, 'QUATERNION REPRESENTATION OF ROTATION MATRIX' (fp64)"""
    a = 1.0 - (b * b + c * c + d * d)
    if a < 1e-7:                               # a = 0 within rounding: a 180 degree rotation, (b, c, d) re-normalised
        s = 1.0 / math.sqrt(b * b + c * c + d * d)
        a, b, c, d = 0.0, b * s, c * s, d * s
    else:
        a = math.sqrt(a)
    R = np.array([[a * a + b * b - c * c - d * d, 2 * b * c - 2 * a * d, 2 * b * d + 2 * a * c],
                  [2 * b * c + 2 * a * d, a * a + c * c - b * b - d * d, 2 * c * d - 2 * a * b],
                  [2 * b * d - 2 * a * c, 2 * c * d + 2 * a * b, a * a + d * d - c * c - b * b]], dtype=np.float64)
    R[:, 2] *= qfac
    return R


def _mat_to_quatern(R):
    """The inverse (nifti_mat44_to_quatern) of a proper rotation matrix: (b, c, d) with a >= 0"""
    r11, r12, r13 = R[0]
    r21, r22, r23 = R[1]
    r31, r32, r33 = R[2]
    a = r11 + r22 + r33 + 1.0
    if a > 0.5:
        a = 0.5 * math.sqrt(a)
        b, c, d = 0.25 * (r32 - r23) / a, 0.25 * (r13 - r31) / a, 0.25 * (r21 - r12) / a
    else:
        xd, yd, zd = 1.0 + r11 - (r22 + r33), 1.0 + r22 - (r11 + r33), 1.0 + r33 - (r11 + r22)
        if xd > 1.0:
            b = 0.5 * math.sqrt(xd)
            c, d, a = 0.25 * (r12 + r21) / b, 0.25 * (r13 + r31) / b, 0.25 * (r32 - r23) / b
        elif yd > 1.0:
            c = 0.5 * math.sqrt(yd)
            b, d, a = 0.25 * (r12 + r21) / c, 0.25 * (r23 + r32) / c, 0.25 * (r13 - r31) / c
        else:
            d = 0.5 * math.sqrt(zd)
            b, c, a = 0.25 * (r13 + r31) / d, 0.25 * (r23 + r32) / d, 0.25 * (r21 - r12) / d
        if a < 0.0:
            b, c, d = -b, -c, -d
    return b, c, d


def geometry(h, path="<header>"):
    """``(itk_spacing, itk_origin, itk_direction)`` of a parsed header: tuples of 3, 3 and 9 (row-major) floats"""
    unit = MM_PER_UNIT.get(h["xyzt_units"] & 7, 1.)
    pixdim = [float(v) for v in h["pixdim"]]
    spacing = np.array([abs(v) for v in pixdim[1:4]], dtype=np.float64) * unit
    if h["qform_code"] > 0:
        R = _quatern_to_mat(*(float(v) for v in h["quatern"]), -1.0 if pixdim[0] < 0 else 1.0)
        offset = np.array(h["qoffset"], dtype=np.float64) * unit
    elif h["sform_code"] > 0:
        A = np.array([h["srow_x"][:3], h["srow_y"][:3], h["srow_z"][:3]], dtype=np.float64)
        norms = np.sqrt((A * A).sum(axis=0))
        if not (np.all(np.isfinite(norms)) and np.all(norms > 0)):
            _refuse(path, "srow_x/y/z", "has a column of length %s: no direction" % (norms.tolist(),))
        R, spacing = A / norms, norms * unit
        offset = np.array([h["srow_x"][3], h["srow_y"][3], h["srow_z"][3]], dtype=np.float64) * unit
    else:
        R, offset = np.eye(3), np.zeros(3)
    if not (np.all(np.isfinite(spacing)) and np.all(spacing > 0)):
        _refuse(path, "pixdim", "gives the spacing %s: not positive and finite" % (spacing.tolist(),))
    lps = np.diag([-1., -1., 1.])
    # (+ 0.0: a zero that the sign flip made -0.0 is reported as 0.0)
    return (tuple(float(v) for v in spacing), tuple(float(v) + 0.0 for v in lps @ offset),
            tuple(float(v) + 0.0 for v in (lps @ R).reshape(9)))


def _volume_shape(h, path):
    dim = h["dim"]
    nd = dim[0]
    if nd < 3 or nd > 7:
        _refuse(path, "dim[0]", "is %d: a volume has 3 dimensions (4 to 7 with every further one equal to 1)" % nd)
    for k in range(4, nd + 1):
        if dim[k] != 1:
            _refuse(path, "dim[%d]" % k, "is %d: only three-dimensional volumes are read (no time series, no vectors)" % dim[k])
    for k in (1, 2, 3):
        if dim[k] < 1:
            _refuse(path, "dim[%d]" % k, "is %d" % dim[k])
    return int(dim[3]), int(dim[2]), int(dim[1])


class DeferredPayload:
    """The voxels of a ``.nii.gz`` that ``read_raw(inflate="device")`` left compressed: ``stream`` (uint8 host array) is the raw
    DEFLATE stream of the gzip member, ``total`` the length it inflates to (header included), ``offset`` / ``size`` where the
    payload lies in that, ``crc`` the member's CRC-32.  ``_upload`` resolves it on the thread that owns the GPU."""
    __slots__ = ("stream", "total", "offset", "size", "crc")

    def __init__(self, stream, total, offset, size, crc):
        self.stream, self.total, self.offset, self.size, self.crc = stream, total, offset, size, crc


def gzip_member(data):
    """``(offset of the raw DEFLATE stream, crc32, isize)`` of a file's bytes that hold one gzip member (RFC 1952): magic, CM = 8,
    FEXTRA, FNAME, FCOMMENT and FHCRC honoured, the trailer taken from the last 8 bytes.  None for anything else (a reserved flag
    bit, a header that runs over the end): such a file is the host route's to read or to refuse."""
    n = len(data)
    if n < 18 or bytes(data[:3]) != b"\x1f\x8b\x08":
        return None
    flags = int(data[3])
    if flags & 0xE0:
        return None
    at = 10
    if flags & 4:                                      # FEXTRA: XLEN and that many bytes
        at += 2 + int(data[at]) + (int(data[at + 1]) << 8)
        if at + 8 > n:
            return None
    for bit in (8, 16):                                # FNAME, FCOMMENT: zero-terminated
        if flags & bit:
            while at < n and data[at] != 0:
                at += 1
            at += 1
    if flags & 2:                                      # FHCRC
        at += 2
    if at + 8 > n:
        return None
    crc, isize = struct.unpack("<II", bytes(data[n - 8:]))
    return at, crc, isize


_HEAD_WINDOW = 1 << 20              # compressed bytes looked at for the header and the gap up to vox_offset


def _read_deferred(path):
    """The device route of ``read_raw``: ``(the inflated bytes in front of the voxels' end that the host needs, DeferredPayload
    factory)`` -- or None where the host route has to take the file (see ``read_raw``)."""
    import zlib
    data = np.fromfile(path, dtype=np.uint8)
    member = gzip_member(data)
    if member is None:
        return None
    at, crc, isize = member
    d = zlib.decompressobj(-15)
    try:
        hdr = d.decompress(bytes(data[at:at + _HEAD_WINDOW]), HEADER_BYTES)
    except zlib.error:
        return None
    if len(hdr) < HEADER_BYTES:
        return None
    return data, at, crc, isize, d, hdr


def read_raw(path, inflate="host"):
    """Header and payload of a ``.nii`` / ``.nii.gz`` file as a ``NiftiRaw``.  Host only (safe in a thread pool): the payload is
    inflated straight into one preallocated buffer, which is what gets uploaded.  Every refusal is a ValueError naming the file
    and the field.

    ``inflate="device"`` (``.gz`` files; any other file is read as before): the host parses the gzip member header and inflates
    only the bytes in front of ``vox_offset``; the payload stays compressed in a ``DeferredPayload`` and is inflated on the device
    (``deflate.inflate_any``) when a decoder uploads it.  Still host only.  The header is parsed and refused exactly as on the host
    route.  What the device route does not serve is read on the host route here and now, with its result or its refusal: a file
    that is no single plain gzip member, a stream that fails in front of ``vox_offset``, an ISIZE that is not ``vox_offset`` + the
    payload's size (a truncated payload, a second member, a total of 4 GiB or more)."""
    import io
    if inflate not in ("host", "device"):
        raise ValueError("read_raw: inflate=%r is neither 'host' nor 'device'" % (inflate,))
    path = os.fspath(path)
    opener = _opener(path)
    deferred = _read_deferred(path) if inflate == "device" and path.lower().endswith(".gz") else None
    if inflate == "device" and deferred is None:
        return read_raw(path)
    with (io.BytesIO(deferred[5]) if deferred else opener()) as f:
        hdr = _read_exact(f, HEADER_BYTES)
        h = parse_header(hdr, path)
        shape = _volume_shape(h, path)
        datatype = int(h["datatype"])
        if datatype not in DATATYPES:
            _refuse(path, "datatype", "is %d: read are %s (uint8, int16, int32, float32, float64, int8, uint16, uint32, int64, "
                    "uint64)" % (datatype, ", ".join(str(k) for k in DATATYPES)))
        elsize = DATATYPES[datatype][1]
        if h["bitpix"] != 8 * elsize:
            _refuse(path, "bitpix", "is %d, datatype %d has %d bits" % (h["bitpix"], datatype, 8 * elsize))
        vox_offset = float(h["vox_offset"])
        if not (math.isfinite(vox_offset) and vox_offset == int(vox_offset) and HEADER_BYTES <= vox_offset <= 2 ** 24):
            _refuse(path, "vox_offset", "is %r: the voxels of a single-file NIfTI-1 start at or after byte 348" % vox_offset)
        spacing, origin, direction = geometry(h, path)
        skip = int(vox_offset) - HEADER_BYTES
        nbytes = shape[0] * shape[1] * shape[2] * elsize
        if deferred:
            import zlib
            data, at, crc, isize, d, _ = deferred
            try:
                skipped = len(d.decompress(d.unconsumed_tail, skip)) if skip else 0
            except zlib.error:
                skipped = -1
            if skipped != skip or isize != int(vox_offset) + nbytes:
                return read_raw(path)
            payload = DeferredPayload(data[at:data.size - 8], int(vox_offset) + nbytes, int(vox_offset), nbytes, crc)
        else:
            if len(_read_exact(f, skip)) != skip:
                _refuse(path, "vox_offset", "is %d, past the end of the file" % int(vox_offset))
            payload = np.empty(nbytes, dtype=np.uint8)          # (numpy's allocation: aligned to any element size)
            view, got = memoryview(payload), 0
            while got < nbytes:
                n = f.readinto(view[got:])
                if not n:
                    break
                got += n
            if got != nbytes:
                _refuse(path, "payload", "is truncated: %d bytes after vox_offset, dim and bitpix ask for %d" % (got, nbytes))
    slope, inter = float(h["scl_slope"]), float(h["scl_inter"])
    scale = slope != 0. and math.isfinite(slope) and not (slope == 1. and inter == 0.)
    if scale and not math.isfinite(inter):
        _refuse(path, "scl_inter", "is %r" % inter)
    swap = h["byteorder"] != ("<" if np.little_endian else ">")
    return NiftiRaw(path, shape, datatype, elsize, swap, scale, slope, inter, payload, spacing, origin, direction)


def properties_of(raw, list_of_files=None):
    """the reference's ``load_case_from_list_of_files`` keys (e2enet/preprocessing/cropping.py:61-81) from a ``NiftiRaw``"""
    properties = OrderedDict()
    properties["original_size_of_raw_data"] = np.array(raw.shape)
    properties["original_spacing"] = np.array(raw.itk_spacing)[[2, 1, 0]]
    properties["list_of_data_files"] = list_of_files
    properties["seg_file"] = None
    properties["itk_origin"] = raw.itk_origin
    properties["itk_spacing"] = raw.itk_spacing
    properties["itk_direction"] = raw.itk_direction
    return properties


# ---------------------------------------------------------------------------------------------------------------- device half
def _require_device():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("NIfTI voxels are decoded on the GPU (csrc/nifti.hip); there is no host fallback")


def resolve_payload(raw, inflater=None):
    """The stored bytes of a ``NiftiRaw`` whose payload is a ``DeferredPayload``, as a uint8 device tensor: the member inflated on
    the device, its CRC-32 checked there (a ValueError that names the file), the payload sliced out at ``vox_offset`` (one device
    copy when that is no multiple of the element size).  Where ``inflate_any`` says None the file is read on the host route and
    uploaded, with that route's refusals.  ``inflater(stream, total) -> (bytes as a tensor or array, or None; crc32)`` replaces the
    device steps (tests without a device)."""
    import torch
    from . import deflate
    p = raw.payload
    if inflater is None:
        _require_device()
        try:
            got = deflate.inflate_any(p.stream, p.total)
        except ValueError as e:
            raise ValueError("%s: %s" % (raw.path, e)) from None
        crc = deflate.device_crc32(got) if got is not None else 0
    else:
        got, crc = inflater(p.stream, p.total)
    if got is None:
        host = torch.from_numpy(read_raw(raw.path).payload)
        return host.to("cuda") if inflater is None else host
    if crc != p.crc:
        raise ValueError("%s: the inflated bytes do not give the CRC-32 of the gzip trailer (%08x)" % (raw.path, p.crc))
    if not isinstance(got, torch.Tensor):
        got = torch.from_numpy(np.ascontiguousarray(got))
    body = got[p.offset:p.offset + p.size]
    return body.clone() if p.offset % raw.elsize else body


def _upload(raw):
    import torch
    if isinstance(raw.payload, DeferredPayload):
        return resolve_payload(raw)
    _require_device()
    return torch.from_numpy(raw.payload).to("cuda")


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def decode_f32(raw, out=None):
    """The voxels of a ``NiftiRaw`` as fp32 on the device: one upload of the stored bytes, one kernel.  ``out``: a contiguous fp32
    device tensor of the volume's shape to write into (a channel of a case), default a new one.  Returns it."""
    import torch
    from ._lib import lib
    dev = _upload(raw)
    if out is None:
        out = torch.empty(raw.shape, dtype=torch.float32, device=dev.device)
    if not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == tuple(raw.shape)):
        raise ValueError("decode_f32: out must be a contiguous fp32 device tensor of shape %s" % (tuple(raw.shape),))
    lib().nifti_decode_f32(dev.data_ptr(), dev.numel() // raw.elsize, raw.datatype, int(raw.swap), int(raw.scale), raw.slope,
                           raw.inter, out.data_ptr(), _stream())
    return out


def decode_u8(raw):
    """The voxels of a ``NiftiRaw`` as a uint8 label volume on the device.  A voxel that is no whole number in [0, 255] (after the
    header's scaling) is a ValueError."""
    import torch
    from ._lib import lib
    dev = _upload(raw)
    out = torch.empty(raw.shape, dtype=torch.uint8, device=dev.device)
    rejected = torch.zeros(1, dtype=torch.int64, device=dev.device)
    lib().nifti_decode_u8(dev.data_ptr(), dev.numel() // raw.elsize, raw.datatype, int(raw.swap), int(raw.scale), raw.slope,
                          raw.inter, out.data_ptr(), rejected.data_ptr(), _stream())
    bad = int(rejected.item())
    if bad:
        raise ValueError("%s: %d voxel(s) are no whole-number labels in [0, 255]: not a label volume" % (raw.path, bad))
    return out


def scan(raw):
    """The integrity scan of a ``NiftiRaw`` (``e2e_nifti_scan``): one upload of the stored bytes, one pass over them on the device,
    260 words back.  Returns a ``NiftiScan``."""
    import torch
    from ._lib import lib
    dev = _upload(raw)
    out = torch.empty(SCAN_WORDS, dtype=torch.int64, device=dev.device)
    lib().nifti_scan(dev.data_ptr(), dev.numel() // raw.elsize, raw.datatype, int(raw.swap), int(raw.scale), raw.slope, raw.inter,
                     out.data_ptr(), _stream())
    words = out.cpu().numpy()                                    # (~0 of the two index words reads -1)
    return NiftiScan(int(words[0]), int(words[1]), int(words[2]), int(words[3]), words[4:].copy())


# ------------------------------------------------------------------------------------------------------------------ callbacks
def reader(list_of_files, inflate="host"):
    """``reader(list_of_files) -> (data, properties)`` of the cropping, preprocessing and prediction entry points: ``data`` is an
    fp32 device tensor ``[C, Z, Y, X]``, every modality decoded straight into its channel; ``properties`` are those of the first
    file (the reference's keys).  ``inflate``: as in ``read_raw`` (``callbacks("device")`` binds it)."""
    import torch
    assert isinstance(list_of_files, (list, tuple)), "case must be either a list or a tuple"
    raws = [read_raw(f, inflate) for f in list_of_files]         # (host; every refusal comes before the first upload)
    first = raws[0]
    for raw in raws[1:]:
        if raw.shape != first.shape:
            raise ValueError("%s: dim gives the shape %s, %s has %s: the modalities of a case share one grid"
                             % (raw.path, raw.shape, first.path, first.shape))
    _require_device()
    data = torch.empty((len(raws),) + first.shape, dtype=torch.float32, device="cuda")
    for c in range(len(raws)):
        decode_f32(raws[c], data[c])
        raws[c] = None                                           # (the host copy of a modality goes once it is decoded)
    return data, properties_of(first, list_of_files)


def _axes_identity():
    return (1., 1., 1.), (0., 0., 0.), (1., 0., 0., 0., 1., 0., 0., 0., 1.)


def build_header(shape, itk_spacing, itk_origin, itk_direction):
    """The 348 bytes ``write`` stores for a uint8 volume ``[Z, Y, X]`` (little-endian): the inverse of ``geometry``, qform and
    sform both with code 1, millimetres, scl_slope 1."""
    spacing = np.array([float(v) for v in itk_spacing], dtype=np.float64)
    lps = np.diag([-1., -1., 1.])
    R = lps @ np.array([float(v) for v in itk_direction], dtype=np.float64).reshape(3, 3)
    offset = lps @ np.array([float(v) for v in itk_origin], dtype=np.float64)
    if not (spacing.shape == (3,) and np.all(np.isfinite(spacing)) and np.all(spacing > 0)):
        raise ValueError("write: itk_spacing %r is not three positive lengths" % (itk_spacing,))
    qfac = -1.0 if np.linalg.det(R) < 0 else 1.0
    P = R.copy()
    P[:, 2] *= qfac
    b, c, d = _mat_to_quatern(P)
    hdr = bytearray(HEADER_BYTES)
    put = lambda off, fmt, *v: struct.pack_into("<" + fmt, hdr, off, *v)
    put(0, "i", HEADER_BYTES)
    put(38, "c", b"r")
    put(40, "8h", 3, int(shape[2]), int(shape[1]), int(shape[0]), 1, 1, 1, 1)
    put(70, "h", 2)
    put(72, "h", 8)
    put(76, "8f", qfac, spacing[0], spacing[1], spacing[2], 0., 0., 0., 0.)
    put(108, "f", float(HEADER_BYTES + 4))
    put(112, "f", 1.)
    put(116, "f", 0.)
    put(123, "B", 2)
    put(252, "h", 1)
    put(254, "h", 1)
    put(256, "3f", b, c, d)
    put(268, "3f", *offset)
    A = R * spacing
    for row, off in enumerate((280, 296, 312)):
        put(off, "4f", A[row, 0], A[row, 1], A[row, 2], offset[row])
    put(344, "4s", b"n+1\0")
    return bytes(hdr)


def _geometry_of(properties):
    properties = properties or {}
    if all(k in properties for k in ("itk_spacing", "itk_origin", "itk_direction")):
        return properties["itk_spacing"], properties["itk_origin"], properties["itk_direction"]
    return _axes_identity()


def _check_shape(shape):
    if len(shape) != 3:
        raise ValueError("write: the volume has shape %s, not three axes" % (tuple(shape),))
    if any(int(v) < 1 or int(v) > 32767 for v in shape):
        raise ValueError("write: an axis of %s does not fit dim (1 .. 32767)" % (tuple(shape),))


def _write_device(seg, path, properties, codes="fixed"):
    """``write`` of a device label volume: the 352 bytes in front of the voxels go through host zlib, the voxels are deflated on the
    device (deflate.gzip_member, ``codes`` as there) and only compressed bytes are downloaded"""
    import torch
    from . import deflate
    if not (isinstance(seg, torch.Tensor) and seg.is_cuda):
        raise ValueError("write(device_deflate=True): the volume must be a device tensor (got %s); without the flag the host "
                         "compresses" % ("a CPU tensor" if isinstance(seg, torch.Tensor) else type(seg).__name__))
    if not seg.is_contiguous():
        raise ValueError("write(device_deflate=True): the volume is not contiguous (shape %s, strides %s)"
                         % (tuple(seg.shape), tuple(seg.stride())))
    _check_shape(seg.shape)
    if not str(path).lower().endswith(".gz"):
        raise ValueError("write(device_deflate=True): %s is no .gz path, there is nothing to compress" % (path,))
    if seg.dtype != torch.uint8:
        as_u8 = seg.to(torch.uint8)
        if not bool((as_u8.to(seg.dtype) == seg).all().item()):
            raise ValueError("write: the volume holds values that are no labels in [0, 255]")
        seg = as_u8
    body = build_header(tuple(seg.shape), *_geometry_of(properties)) + b"\0\0\0\0"
    member = deflate.gzip_member(body, seg, codes)
    with open(path, "wb") as fh:
        fh.write(member)


def write(seg, path, properties=None, device_deflate=False):
    """A uint8 label volume ``[Z, Y, X]`` as a NIfTI-1 ``.nii.gz`` (``.nii`` for a path without ``.gz``) with the geometry of
    ``properties`` (``itk_origin``, ``itk_spacing``, ``itk_direction``; without them identity LPS and spacing 1).  Deterministic:
    the same volume and geometry give the same bytes.  ``device_deflate``: the volume is a contiguous device tensor (anything else
    is a ValueError) and is compressed where it lies (csrc/deflate.hip), with the fixed Huffman code for ``True`` and a code per
    chunk for ``"dynamic"``; the file inflates to the same bytes as the default route's, its compressed bytes differ."""
    if device_deflate:
        from . import deflate
        return _write_device(seg, path, properties, deflate.codes_of(device_deflate, "write: device_deflate"))
    if hasattr(seg, "cpu"):
        seg = seg.cpu().numpy()
    seg = np.asarray(seg)
    _check_shape(seg.shape)
    if seg.dtype != np.uint8:
        as_u8 = seg.astype(np.uint8)
        if not np.array_equal(as_u8, seg):
            raise ValueError("write: the volume holds values that are no labels in [0, 255]")
        seg = as_u8
    spacing, origin, direction = _geometry_of(properties)
    body = build_header(seg.shape, spacing, origin, direction) + b"\0\0\0\0"
    with open(path, "wb") as fh:
        if str(path).lower().endswith(".gz"):
            with gzip.GzipFile(filename="", mode="wb", compresslevel=GZIP_LEVEL, fileobj=fh, mtime=0) as gz:
                gz.write(body)
                gz.write(memoryview(np.ascontiguousarray(seg)).cast("B"))
        else:
            fh.write(body)
            fh.write(memoryview(np.ascontiguousarray(seg)).cast("B"))


def writer(seg, path, properties, device_deflate=False):
    """``writer(seg_uint8, path, properties)`` of ``predict_cases``, ``validate`` and ``ensemble_predictions``.  ``accepts_device``:
    ``predict_cases(device_deflate=True or "dynamic")`` hands it the device label volume and the flag"""
    write(seg, path, properties, device_deflate=device_deflate)


writer.accepts_device = True


def gt_reader(path, inflate="host"):
    """``gt_reader(path) -> label array`` of ``validate``: the uint8 volume (decoded on the device), None for a missing file"""
    if not os.path.isfile(path):
        return None
    return decode_u8(read_raw(path, inflate)).cpu().numpy()


def evaluator_reader(path, inflate="host"):
    """``reader(path) -> (volume, spacing)`` of ``NiftiEvaluator``.  This is the host half, run by the evaluator's read-ahead
    threads: the volume is the ``NiftiRaw``, which ``set_test`` / ``set_reference`` decode on the thread that owns the GPU.  The
    spacing is ``itk_spacing[::-1]``, array-axis order.  ``.npy`` volumes are read as before, without spacing."""
    if path.endswith(".npy"):
        return np.load(path), None
    raw = read_raw(path, inflate)
    return raw, tuple(raw.itk_spacing)[::-1]


class Callbacks:
    """``reader``, ``gt_reader`` and ``evaluator_reader`` bound to one ``inflate`` route of ``read_raw``, ``writer`` beside them"""

    def __init__(self, inflate):
        import functools
        self.inflate = inflate
        self.reader = functools.partial(reader, inflate=inflate)
        self.gt_reader = functools.partial(gt_reader, inflate=inflate)
        self.evaluator_reader = functools.partial(evaluator_reader, inflate=inflate)
        self.writer = writer


def callbacks(inflate="host"):
    """The callbacks of this module for one route of ``read_raw``: for ``"host"`` the module's own functions, the very objects;
    for ``"device"`` the same functions with ``inflate="device"`` bound (``.nii.gz`` payloads are inflated on the GPU)."""
    import sys
    if inflate == "host":
        return sys.modules[__name__]
    if inflate != "device":
        raise ValueError("callbacks: inflate=%r is neither 'host' nor 'device'" % (inflate,))
    return Callbacks(inflate)


def inflate_from_args(args, also=()):
    """``"device"`` with ``--inflate_any``, else ``"host"``.  The flag without ``--native_nifti`` does nothing to any .nii.gz and is
    refused by name (a ValueError) before any work -- unless one of the switches named in ``also`` is set, for which the command
    gives the flag a meaning of its own (``--resident_data`` of the training, ``--device_inflate`` of the ensembling)."""
    if not getattr(args, "inflate_any", False):
        return "host"
    if getattr(args, "native_nifti", False):
        return "device"
    if any(getattr(args, name, None) not in (None, False) for name in also):
        return "host"
    raise ValueError("--inflate_any inflates the .nii.gz files that --native_nifti reads on the GPU: it needs --native_nifti%s"
                     % "".join(" or --%s" % name for name in also))


def from_args(args, also=()):
    """``callbacks`` for the parsed switches of a command that called ``add_argument``"""
    return callbacks(inflate_from_args(args, also))


def add_argument(parser):
    """the ``--native_nifti`` and ``--inflate_any`` switches of the command-line tools; ``from_args`` reads them"""
    parser.add_argument("--native_nifti", action="store_true", default=False,
                        help="read and write .nii.gz with this package's own NIfTI-1 code (header and gzip on the host, the voxels "
                             "decoded on the GPU) instead of SimpleITK; default: SimpleITK when it is installed")
    parser.add_argument("--inflate_any", action="store_true", default=False,
                        help="with --native_nifti: inflate the .nii.gz files that are read on the GPU as well (any gzip writer's; "
                             "a file the GPU route does not serve is inflated on the host as before, with the same result)")
