"""The dynamic-Huffman entry of the device DEFLATE encoder (``e2e_deflate_encode_dynamic``) against its restatement in Python
(tests/deflate_dynamic_oracle.py) and host zlib: the exact bytes, the CRC, the form of every chunk, never more bytes than the fixed
entry; then the writers with ``device_deflate="dynamic"``: ``nifti.write``, ``deflate.savez``, and the two dataset folders."""
import gzip
import os
import pickle
import zlib

import numpy as np
import pytest
import torch

from tests import deflate_dynamic_oracle as oracle
from tests.test_gpu_deflate import CHUNK

gpu = pytest.mark.gpu
pytestmark = gpu


def _deflate():
    from e2enet_medical_amd import deflate
    assert deflate.chunk_bytes() == CHUNK
    return deflate


def _device(case):
    return torch.from_numpy(oracle.inputs()[case].copy()).cuda()


def _encode(dev, elem, dynamic):
    """(slots, counts, kinds, crc) of one call of the C entry, on the host"""
    from e2enet_medical_amd._lib import lib
    L = lib()
    slot = int(L.deflate_slot_bytes())
    nchunks = -(-dev.numel() // CHUNK)
    slots = torch.zeros(nchunks * slot, dtype=torch.uint8, device="cuda")
    counts = torch.zeros(nchunks, dtype=torch.int32, device="cuda")
    kinds = torch.full((nchunks,), 9, dtype=torch.uint8, device="cuda")
    crcs = torch.zeros(nchunks, dtype=torch.int32, device="cuda")
    crc = torch.zeros(1, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    if dynamic:
        L.deflate_encode_dynamic(dev.data_ptr(), dev.numel(), elem, slots.data_ptr(), counts.data_ptr(), kinds.data_ptr(),
                                 crcs.data_ptr(), crc.data_ptr(), st)
    else:
        L.deflate_encode(dev.data_ptr(), dev.numel(), elem, slots.data_ptr(), counts.data_ptr(), crcs.data_ptr(), crc.data_ptr(), st)
    return slots.cpu().numpy().reshape(nchunks, slot), counts.cpu().numpy(), kinds.cpu().numpy(), int(crc.item()) & 0xFFFFFFFF


@pytest.mark.parametrize("case,elem", oracle.cases())
def test_stream_equals_the_restatement(case, elem):
    """1, 2, 4: byte for byte the restatement, which inflates to the input; zlib's CRC; the kinds; the same bytes on a second call"""
    d = _deflate()
    host = oracle.inputs()[case]
    dev = _device(case)
    want = oracle.reference(case, elem)
    stream, crc, nbytes = d.raw_deflate(dev, elem, codes="dynamic")
    assert nbytes == host.size and crc == zlib.crc32(host.tobytes())
    inflater = zlib.decompressobj(-15)
    assert inflater.decompress(stream) == host.tobytes() and inflater.eof and inflater.unused_data == b""
    assert stream == b"".join(c for c, _ in want) + b"\x03\x00"
    kinds = d.chunk_kinds(dev, elem, codes="dynamic")
    assert kinds.dtype == np.uint8 and kinds.tolist() == [k for _, k in want]
    if case in ("b", "c"):
        assert set(kinds.tolist()) == {0}
    if case in ("d", "e", "f", "g", "h"):
        assert set(kinds.tolist()) == {2}
    if case == "i":
        assert kinds.tolist() == [0, 2]
    again = d.raw_deflate(dev, elem, codes="dynamic")
    assert again[0] == stream and again[1] == crc


@pytest.mark.parametrize("case,elem", [(c, e) for c, e in oracle.cases() if c in ("a65542", "b", "d", "f", "h", "i", "j")])
def test_never_more_bytes_than_the_fixed_entry(case, elem):
    """3: per chunk, counts of the dynamic entry <= counts of e2e_deflate_encode; a chunk that is stored or fixed has that entry's
    bytes"""
    dev = _device(case)
    slots_d, counts_d, kinds, crc_d = _encode(dev, elem, True)
    slots_f, counts_f, _, crc_f = _encode(dev, elem, False)
    assert crc_d == crc_f
    assert (counts_d <= counts_f).all(), (counts_d, counts_f)
    assert set(kinds.tolist()) <= {0, 1, 2}
    for c in range(len(kinds)):
        if kinds[c] != 2:
            assert counts_d[c] == counts_f[c] and slots_d[c, :counts_d[c]].tobytes() == slots_f[c, :counts_f[c]].tobytes()
            assert (slots_f[c, 0] == 0) == (kinds[c] == 0)
        else:
            assert counts_d[c] < counts_f[c]


def test_fixed_codes_are_the_default_and_report_their_kinds():
    d = _deflate()
    dev = _device("i")
    assert d.raw_deflate(dev, 1) == d.raw_deflate(dev, 1, codes="fixed")
    assert d.chunk_kinds(dev, 1, codes="fixed").tolist() == [0, 1]
    with pytest.raises(ValueError, match="codes"):
        d.raw_deflate(dev, 1, codes="huffman")


# ----------------------------------------------------------------------------------------------------------------- the writers
def test_nifti_write_dynamic_reads_back_as_the_default(tmp_path):
    """5: (f) as a label volume"""
    from e2enet_medical_amd import nifti
    seg = oracle.inputs()["f"].reshape(24, 64, 64)
    props = {"itk_spacing": (0.5, 0.75, 2.0), "itk_origin": (1., -2., 3.), "itk_direction": (1., 0., 0., 0., 1., 0., 0., 0., 1.)}
    a, b, c = (str(tmp_path / n) for n in ("a.nii.gz", "b.nii.gz", "c.nii.gz"))
    nifti.write(seg.copy(), a, props)
    nifti.write(torch.from_numpy(seg.copy()).cuda(), b, props, device_deflate="dynamic")
    nifti.writer(torch.from_numpy(seg.copy()).cuda(), c, props, device_deflate=True)
    assert gzip.decompress(open(b, "rb").read()) == gzip.decompress(open(a, "rb").read()) == gzip.decompress(open(c, "rb").read())
    assert os.path.getsize(b) < os.path.getsize(c)
    raw = nifti.read_raw(b)
    assert raw.shape == seg.shape and raw.itk_spacing == nifti.read_raw(a).itk_spacing
    assert np.array_equal(nifti.decode_u8(raw).cpu().numpy(), seg)


def test_savez_dynamic_reads_back_as_the_default(tmp_path):
    """5: (g) as fp16 probabilities through deflate.savez, npz_parts and save_softmax_npz"""
    import zipfile
    from e2enet_medical_amd import deflate
    from e2enet_medical_amd.inference.predict import save_softmax_npz
    soft = oracle.inputs()["g"].view(np.float16).reshape(4, 24, 64, 64)
    dev = torch.from_numpy(soft.copy()).cuda()
    a, b, c, e = (str(tmp_path / n) for n in ("a.npz", "b.npz", "c.npz", "e.npz"))
    np.savez_compressed(a, softmax=soft)
    deflate.savez(b, codes="dynamic", softmax=dev)
    deflate.savez(c, softmax=dev)
    assert zipfile.ZipFile(b).testzip() is None
    got = np.load(b)["softmax"]
    assert got.dtype == np.float16 and got.shape == soft.shape and got.tobytes() == np.load(a)["softmax"].tobytes()
    assert os.path.getsize(b) < 0.7 * os.path.getsize(c)
    assert b"".join(deflate.npz_parts(codes="dynamic", softmax=dev)) == open(b, "rb").read()
    props = {"itk_spacing": (1., 1., 2.), "size_after_cropping": (24, 64, 64)}
    save_softmax_npz(dev, e, props, device_deflate="dynamic")
    assert open(e, "rb").read() == open(b, "rb").read()
    assert pickle.load(open(e[:-4] + ".pkl", "rb"))["size_after_cropping"] == (24, 64, 64)


def _same_folder(a, b, names, npz_bytes):
    """``data`` and the pickles of two folders are equal; the ``.npz`` bytes too where asked"""
    for name in names:
        x, y = np.load(os.path.join(a, name + ".npz")), np.load(os.path.join(b, name + ".npz"))
        assert x.files == y.files == ["data"]
        assert x["data"].dtype == y["data"].dtype and x["data"].shape == y["data"].shape
        assert x["data"].tobytes() == y["data"].tobytes()
        assert open(os.path.join(a, name + ".pkl"), "rb").read() == open(os.path.join(b, name + ".pkl"), "rb").read()
        if npz_bytes:
            assert open(os.path.join(a, name + ".npz"), "rb").read() == open(os.path.join(b, name + ".npz"), "rb").read()


def _raw_cases(folder):
    """two raw cases of two modalities of 16 x 32 x 32 held in memory: ``(lists, reader)`` as run_cropping takes them; the label
    files exist because run_cropping copies them"""
    os.makedirs(folder)
    store, lists = {}, []
    for ci in range(2):
        rng = np.random.default_rng(70 + ci)
        body = np.zeros((16, 32, 32), dtype=bool)
        body[2:14, 3 + ci:29, 4:30 - ci] = True
        names = ["case%d_0000.nii.gz" % ci, "case%d_0001.nii.gz" % ci, "case%d.nii.gz" % ci]
        for m in range(2):
            store[names[m]] = np.where(body, rng.normal(100 * (m + 1), 20, body.shape), 0).astype(np.float32)
        store[names[2]] = ((body & (rng.random(body.shape) < 0.3)) * (1 + ci)).astype(np.float32)
        with open(os.path.join(folder, names[2]), "wb") as f:
            f.write(b"gt of case%d" % ci)
        lists.append([os.path.join(folder, n) for n in names])

    def reader(list_of_files):
        data = np.stack([store[os.path.basename(f)] for f in list_of_files])
        return data, {"original_spacing": np.array([2.5, 1.0, 1.0]), "itk_spacing": (1.0, 1.0, 2.5), "itk_origin": (0.0, 0.0, 0.0)}
    return lists, reader


def test_preprocessed_folder_through_the_device_encoder(tmp_path):
    """6: a two-case cropped folder of 2 x 16 x 32 x 32 through run_preprocessing: host route, ``"dynamic"`` with 1 and with 4 writer
    threads"""
    from e2enet_medical_amd.preprocessing import ImageCropper, run_preprocessing
    from tests.test_gpu_dataset import ALL_CLASSES, DATA_IDENTIFIER, _plans
    from tests.test_gpu_preprocess import _raw_case
    cropped = str(tmp_path / "cropped")
    os.makedirs(os.path.join(cropped, "gt_segmentations"))
    names = ("case_a", "case_b")
    for ci, name in enumerate(names):
        x, props = _raw_case(80 + ci, shape=(16, 32, 32))
        zz, yy, xx = np.meshgrid(*[np.arange(s) for s in x.shape[1:]], indexing="ij")
        seg = ((((zz // 2 + yy // 4 + xx // 5 + ci) % 4) < 2).astype(np.float32) + ((zz + yy // 3 + xx // 3) % 5 == 0)).astype(np.float32)
        data, seg, props = ImageCropper.crop(x, props, np.minimum(seg, 2.0)[None])
        np.savez_compressed(os.path.join(cropped, name + ".npz"), data=np.vstack((data, seg)))
        with open(os.path.join(cropped, name + ".pkl"), "wb") as f:
            pickle.dump(props, f)
        with open(os.path.join(cropped, "gt_segmentations", name + ".nii.gz"), "wb") as f:
            f.write(b"gt of " + name.encode())
    with open(os.path.join(cropped, "dataset_properties.pkl"), "wb") as f:
        pickle.dump({"all_classes": ALL_CLASSES}, f)
    host, one, four = (str(tmp_path / n) for n in ("host", "one", "four"))
    run_preprocessing(_plans(), cropped, host, 1)
    run_preprocessing(_plans(), cropped, one, 1, device_deflate="dynamic")
    run_preprocessing(_plans(), cropped, four, 4, unpack_npy=True, device_deflate="dynamic")
    for i in range(2):
        a, b, c = (os.path.join(o, "%s_stage%d" % (DATA_IDENTIFIER, i)) for o in (host, one, four))
        assert sorted(os.listdir(b)) == sorted(os.listdir(a))
        _same_folder(a, b, names, npz_bytes=False)
        _same_folder(b, c, names, npz_bytes=True)
        for name in names:
            assert np.array_equal(np.load(os.path.join(c, name + ".npy"), "r"), np.load(os.path.join(a, name + ".npz"))["data"])


def test_cropped_folder_through_the_device_encoder(tmp_path):
    """6: the same for run_cropping, from raw NIfTI cases"""
    from e2enet_medical_amd.preprocessing import ImageCropper
    lists, reader = _raw_cases(str(tmp_path / "raw"))
    host, one, four = (str(tmp_path / n) for n in ("host", "one", "four"))
    ImageCropper(1, host).run_cropping(lists, reader=reader)
    ImageCropper(1, one).run_cropping(lists, reader=reader, device_deflate="dynamic")
    ImageCropper(4, four).run_cropping(lists, reader=reader, device_deflate="dynamic")
    names = ("case0", "case1")
    assert sorted(os.listdir(one)) == sorted(os.listdir(host))
    _same_folder(host, one, names, npz_bytes=False)
    _same_folder(one, four, names, npz_bytes=True)
    data = np.load(os.path.join(one, "case0.npz"))["data"]
    assert data.dtype == np.float32 and data.shape == (3, 12, 26, 26)
    ImageCropper(1, str(tmp_path / "single")).load_crop_save(lists[1], "case1", reader=reader, device_deflate="dynamic")
    _same_folder(str(tmp_path / "single"), one, names[1:], npz_bytes=True)


# -------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_match_the_fixed_entry():
    """7: elem, null pointers, slot alignment"""
    from e2enet_medical_amd._lib import lib, E2EError
    L = lib()
    x = torch.arange(64, dtype=torch.uint8, device="cuda")
    slot = int(L.deflate_slot_bytes())
    slots = torch.zeros(slot + 16, dtype=torch.uint8, device="cuda")
    words = torch.zeros(4, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    p = words.data_ptr()

    def both(match, src, nbytes, elem, slots_p, counts_p, kinds_p, crcs_p, crc_p):
        with pytest.raises(E2EError, match=match):
            L.deflate_encode(src, nbytes, elem, slots_p, counts_p, crcs_p, crc_p, st)
        with pytest.raises(E2EError, match=match):
            L.deflate_encode_dynamic(src, nbytes, elem, slots_p, counts_p, kinds_p, crcs_p, crc_p, st)
    both("elem", x.data_ptr(), 64, 3, slots.data_ptr(), p, p, p, p)
    both("elem", x.data_ptr(), 6, 4, slots.data_ptr(), p, p, p, p)
    both("null", x.data_ptr(), 64, 1, slots.data_ptr(), p, p, p, None)
    both("null", None, 64, 1, slots.data_ptr(), p, p, p, p)
    both("null", x.data_ptr(), 64, 1, None, p, p, p, p)
    both("null", x.data_ptr(), 64, 1, slots.data_ptr(), None, p, p, p)
    both("null", x.data_ptr(), 64, 1, slots.data_ptr(), p, p, None, p)
    both("aligned", x.data_ptr(), 64, 1, slots.data_ptr() + 4, p, p, p, p)
    with pytest.raises(E2EError, match="null"):
        L.deflate_encode_dynamic(x.data_ptr(), 64, 1, slots.data_ptr(), p, None, p, p, st)
    L.deflate_encode_dynamic(None, 0, 1, None, None, None, None, p, st)        # nothing to encode: only the CRC word is written
    torch.cuda.synchronize()
    assert int(words[0].item()) == 0
