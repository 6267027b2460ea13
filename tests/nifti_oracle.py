"""Test-local oracle of the NIfTI-1 tests: a header builder and a parser written with ``struct`` against the field table of
nifti1.h (independent of e2enet_medical_amd/nifti.py), ``gzip`` for the container and numpy for the voxel rule."""
import gzip
import struct

import numpy as np

# nifti1.h, struct nifti_1_header, field by field (348 bytes without padding)
FIELDS = [("sizeof_hdr", "i"), ("data_type", "10s"), ("db_name", "18s"), ("extents", "i"), ("session_error", "h"), ("regular", "c"),
          ("dim_info", "B"), ("dim", "8h"), ("intent_p1", "f"), ("intent_p2", "f"), ("intent_p3", "f"), ("intent_code", "h"),
          ("datatype", "h"), ("bitpix", "h"), ("slice_start", "h"), ("pixdim", "8f"), ("vox_offset", "f"), ("scl_slope", "f"),
          ("scl_inter", "f"), ("slice_end", "h"), ("slice_code", "c"), ("xyzt_units", "B"), ("cal_max", "f"), ("cal_min", "f"),
          ("slice_duration", "f"), ("toffset", "f"), ("glmax", "i"), ("glmin", "i"), ("descrip", "80s"), ("aux_file", "24s"),
          ("qform_code", "h"), ("sform_code", "h"), ("quatern_b", "f"), ("quatern_c", "f"), ("quatern_d", "f"), ("qoffset_x", "f"),
          ("qoffset_y", "f"), ("qoffset_z", "f"), ("srow_x", "4f"), ("srow_y", "4f"), ("srow_z", "4f"), ("intent_name", "16s"),
          ("magic", "4s")]
FORMAT = "".join(f for _, f in FIELDS)
assert struct.calcsize("<" + FORMAT) == 348

# NIfTI-1 datatype code -> numpy dtype (native byte order)
NUMPY = {2: np.uint8, 4: np.int16, 8: np.int32, 16: np.float32, 64: np.float64, 256: np.int8, 512: np.uint16, 768: np.uint32,
         1024: np.int64, 1280: np.uint64}


def _defaults():
    d = {}
    for name, fmt in FIELDS:
        n = int(fmt[:-1]) if len(fmt) > 1 and fmt[-1] != "s" else 1
        if fmt[-1] == "s":
            d[name] = b""
        elif fmt[-1] == "c":
            d[name] = b"\0"
        else:
            d[name] = (0,) * n if n > 1 else 0
    return d


def build_header(shape_zyx, datatype, order="<", **fields):
    """348 header bytes for a volume whose array is ``shape_zyx`` (dim1 = x runs fastest).  ``fields`` override any field by name;
    defaults: dim[0] 3, bitpix of the datatype, pixdim 1, vox_offset 352, mm, no form, magic n+1."""
    d = _defaults()
    z, y, x = shape_zyx
    d.update(sizeof_hdr=348, regular=b"r", dim=(3, x, y, z, 1, 1, 1, 1), datatype=datatype,
             bitpix=8 * np.dtype(NUMPY[datatype]).itemsize if datatype in NUMPY else 8, pixdim=(1.,) * 8, vox_offset=352.,
             xyzt_units=2, magic=b"n+1\0")
    unknown = set(fields) - set(d)
    assert not unknown, unknown
    d.update(fields)
    flat = []
    for name, fmt in FIELDS:
        v = d[name]
        flat.extend(v if isinstance(v, (tuple, list)) else [v])
    return struct.pack(order + FORMAT, *flat)


def parse_header(hdr):
    """every field by name, plus 'order'; the byte order is the one in which sizeof_hdr reads 348"""
    order = "<" if struct.unpack_from("<i", hdr, 0)[0] == 348 else ">"
    assert struct.unpack_from(order + "i", hdr, 0)[0] == 348
    values = struct.unpack(order + FORMAT, hdr[:348])
    out, i = {"order": order}, 0
    for name, fmt in FIELDS:
        n = int(fmt[:-1]) if len(fmt) > 1 and fmt[-1] != "s" else 1
        out[name] = values[i] if n == 1 else tuple(values[i:i + n])
        i += n
    return out


def voxel_bytes(array, order="<"):
    """the payload of a native array in the file's byte order"""
    a = np.ascontiguousarray(array)
    return a.astype(a.dtype.newbyteorder(order)).tobytes()


def file_bytes(header, payload, extension=b"\0\0\0\0"):
    """header + the 4-byte extension flag (+ extensions, for a larger vox_offset) + payload"""
    return header + extension + payload


def write_file(path, blob, members=1):
    """``blob`` at ``path``: as it is for .nii, gzipped for .gz, in ``members`` gzip members"""
    if not str(path).endswith(".gz"):
        with open(path, "wb") as f:
            f.write(blob)
        return
    cuts = [len(blob) * k // members for k in range(members + 1)]
    with open(path, "wb") as f:
        for a, b in zip(cuts[:-1], cuts[1:]):
            f.write(gzip.compress(blob[a:b], 1, mtime=0))


def read_file(path):
    """(parsed header, voxel array [dim3, dim2, dim1] in native byte order) of a file, by this module's own reading"""
    if str(path).endswith(".gz"):
        with gzip.open(path, "rb") as f:
            blob = f.read()
    else:
        with open(path, "rb") as f:
            blob = f.read()
    h = parse_header(blob)
    dt = np.dtype(NUMPY[h["datatype"]]).newbyteorder(h["order"])
    shape = (h["dim"][3], h["dim"][2], h["dim"][1])
    n = shape[0] * shape[1] * shape[2]
    vox = np.frombuffer(blob, dtype=dt, count=n, offset=int(h["vox_offset"])).reshape(shape)
    return h, vox.astype(dt.newbyteorder("="))


def voxel_rule(raw, scale, slope=1.0, inter=0.0):
    """fp32 of the stored values: ``raw.astype(f4)``, or ``(raw.astype(f8) * slope + inter).astype(f4)``"""
    with np.errstate(over="ignore", invalid="ignore"):
        if not scale:
            return raw.astype(np.float32)
        return (raw.astype(np.float64) * slope + inter).astype(np.float32)
