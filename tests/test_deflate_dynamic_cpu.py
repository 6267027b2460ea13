"""The dynamic-Huffman format of the device DEFLATE encoder, checked on its restatement in Python (tests/deflate_dynamic_oracle.py)
without a device: host zlib inflates every stream and every chunk, the codes are complete and within their length limits, a chunk
is never longer than its fixed or stored form, and the sizes stand against zlib's own Huffman coding of the same chunks.  Then the
argument plumbing of ``codes`` / ``device_deflate="dynamic"`` / ``--dynamic_huffman``."""
import inspect
import zlib
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import deflate_dynamic_oracle as oracle
from tests.test_gpu_deflate import CHUNK, reference_chunk


def _chunks_of(data):
    return [(c, min(c + CHUNK, len(data))) for c in range(0, len(data), CHUNK)]


@pytest.mark.parametrize("case,elem", oracle.cases())
def test_streams_and_chunks_inflate_and_are_never_longer(case, elem):
    """1, 2, 4: the stream inflates to the input; every chunk alone, closed with 03 00, inflates to its bytes; per chunk the size
    is at most the fixed restatement's and at most n + 5"""
    data = oracle.inputs()[case].tobytes()
    chunks = oracle.reference(case, elem)
    assert len(chunks) == len(_chunks_of(data))
    inflater = zlib.decompressobj(-15)
    assert inflater.decompress(b"".join(c for c, _ in chunks) + b"\x03\x00") == data and inflater.eof and inflater.unused_data == b""
    for (a, b), (body, kind) in zip(_chunks_of(data), chunks):
        fixed = reference_chunk(data, a, b, elem)
        assert len(body) <= len(fixed) and len(body) <= b - a + 5
        assert kind in (oracle.STORED, oracle.FIXED, oracle.DYNAMIC)
        if kind != oracle.DYNAMIC:
            assert body == fixed
        else:
            assert len(body) < len(fixed) and body[0] & 7 == 4          # BFINAL 0, BTYPE 10
        if elem <= a:
            # (a chunk behind the first may begin with a match that reaches back: alone it inflates only with its window)
            d = zlib.decompressobj(-15, zdict=data[max(0, a - 32768):a])
            assert d.decompress(body + b"\x03\x00") == data[a:b] and d.eof
        else:
            assert zlib.decompress(body + b"\x03\x00", -15) == data[a:b]


def test_kinds_of_the_inputs():
    """what the GPU test expects of ``kinds``, on the restatement"""
    for case, elem in oracle.cases():
        kinds = [k for _, k in oracle.reference(case, elem)]
        if case in ("b", "c"):
            assert set(kinds) == {oracle.STORED}, (case, elem)
        if case in ("d", "e", "f", "g", "h"):
            assert set(kinds) == {oracle.DYNAMIC}, (case, elem)
        if case == "i":
            assert kinds == [oracle.STORED, oracle.DYNAMIC], (case, elem)
    assert len(oracle.reference("f", 1)) == 3 and len(oracle.reference("g", 2)) == 24 and len(oracle.reference("h", 4)) == 3


def _kraft(lengths):
    return sum(Fraction(1, 2 ** v) for v in lengths if v)


@pytest.mark.parametrize("elem", [1, 2, 4])
def test_length_limit_and_complete_codes(elem):
    """3: in (e) the unconstrained tree is deeper than 15, no emitted length exceeds 15 (7 for the code-length code), and the Kraft
    sum of every emitted code is exactly 1; the one-symbol distance code is exempt"""
    data = oracle.inputs()["e"].tobytes()
    body, info = oracle.dynamic_block(data, 0, len(data), elem)
    assert max(oracle.code_lengths(info["counts"], 64)) > 15
    assert max(info["ll"]) == 15 and _kraft(info["ll"]) == 1
    assert max(info["cl"]) <= 7 and _kraft(info["cl"]) == 1
    assert info["dl"] == [0]                                            # (no match in this chunk)
    assert all((c > 0) == (v > 0) for c, v in zip(info["counts"], info["ll"]))
    assert zlib.decompress(body + b"\x03\x00", -15) == data


def test_every_emitted_code_is_complete():
    """the same two sums for every dynamic chunk of every input, and the length rule: of two symbols the more frequent one never has
    the longer code, of two equally frequent ones the smaller symbol number never has"""
    for case, elem in oracle.cases():
        data = oracle.inputs()[case].tobytes()
        for (a, b), (_, kind) in zip(_chunks_of(data), oracle.reference(case, elem)):
            if kind != oracle.DYNAMIC:
                continue
            _, info = oracle.dynamic_block(data, a, b, elem)
            assert _kraft(info["ll"]) == 1 and max(info["ll"]) <= 15, (case, elem, a)
            assert _kraft(info["cl"]) == 1 and max(info["cl"]) <= 7, (case, elem, a)
            for counts, lengths in ((info["counts"], info["ll"]), (info["cl_counts"], info["cl"])):
                used = sorted((s for s in range(len(counts)) if counts[s]), key=lambda s: (-counts[s], s))
                assert [lengths[s] for s in used] == sorted(lengths[s] for s in used), (case, elem, a)
            assert info["dl"] in ([0], [0] * {1: 0, 2: 1, 4: 3, 8: 5}[elem] + [1])


def test_code_lengths_on_small_counts():
    assert oracle.code_lengths([0, 5, 0], 15) == [0, 1, 0]
    assert oracle.code_lengths([1, 1], 15) == [1, 1]
    assert oracle.code_lengths([1, 1, 2], 15) == [2, 2, 1]
    assert oracle.code_lengths([3, 3, 3, 3], 15) == [2, 2, 2, 2]
    assert oracle.code_lengths([1, 2, 4, 8, 16], 3) == [3, 3, 3, 3, 1]      # (depths 4 4 3 2 1: one step of the limit)
    deep = oracle.code_lengths([1, 2, 4, 8, 16, 32, 64, 128, 256], 4)
    assert max(deep) == 4 and _kraft(deep) == 1 and deep == sorted(deep, reverse=True)
    assert oracle.canonical([3, 3, 3, 3, 3, 2, 4, 4]) == [2, 3, 4, 5, 6, 0, 14, 15]        # RFC 1951, 3.2.2


def _yardstick(data, strategy):
    total = 0
    for a, b in _chunks_of(data):
        z = zlib.compressobj(9, zlib.DEFLATED, -15, 9, strategy)
        total += len(z.compress(data[a:b]) + z.flush(zlib.Z_SYNC_FLUSH))
    return total


@pytest.mark.parametrize("case,elem,strategy", [("d", 1, zlib.Z_RLE), ("f", 1, zlib.Z_RLE), ("g", 2, zlib.Z_HUFFMAN_ONLY),
                                                ("h", 4, zlib.Z_HUFFMAN_ONLY)])
def test_size_against_zlib_per_chunk(case, elem, strategy):
    """5: summed over the chunks, at most 1.01 x zlib's size + 4 bytes per chunk, zlib at level 9 and memLevel 9 with one object per
    chunk ended by a sync flush (which carries the same empty stored block).  Z_RLE where the token models coincide (elem 1),
    Z_HUFFMAN_ONLY for the floating-point inputs."""
    data = oracle.inputs()[case].tobytes()
    chunks = oracle.reference(case, elem)
    mine, theirs = sum(len(c) for c, _ in chunks), _yardstick(data, strategy)
    print("%s elem %d: %d bytes, zlib %d" % (case, elem, mine, theirs))
    assert mine <= 1.01 * theirs + 4 * len(chunks), (mine, theirs)


# -------------------------------------------------------------------------------------------------------------------- plumbing
def test_dynamic_huffman_switch_on_the_five_commands():
    """6: --dynamic_huffman parses on the five commands and implies device deflate"""
    from e2enet_medical_amd import crop_and_fingerprint, deflate, preprocess_dataset, simple_main, simple_predict
    from e2enet_medical_amd.experiment_planning import nnUNet_plan_and_preprocess
    required = {simple_predict: [], simple_main: [], preprocess_dataset: ["-t", "1"], crop_and_fingerprint: ["-t", "1"],
                nnUNet_plan_and_preprocess: ["-t", "1"]}
    for module, argv in required.items():
        parser = module.build_parser()
        assert parser.get_default("device_deflate") is False and parser.get_default("dynamic_huffman") is False, module
        plain = parser.parse_args(argv)
        assert plain.device_deflate is False and deflate.from_args(plain) is False
        fixed = parser.parse_args(argv + ["--device_deflate"])
        assert fixed.device_deflate is True and fixed.dynamic_huffman is False and deflate.from_args(fixed) is True
        for extra in (["--dynamic_huffman"], ["--dynamic_huffman", "--device_deflate"], ["--device_deflate", "--dynamic_huffman"]):
            dyn = parser.parse_args(argv + extra)
            assert dyn.device_deflate is True and dyn.dynamic_huffman is True and deflate.from_args(dyn) == "dynamic", (module, extra)
    actions = {a.dest: a for a in simple_main.build_parser()._actions}
    assert actions["dynamic_huffman"].nargs == 0 and "--dynamic_huffman" in actions["dynamic_huffman"].option_strings


def test_codes_argument_and_defaults(tmp_path):
    from e2enet_medical_amd import deflate, nifti
    from e2enet_medical_amd.experiment_planning import crop
    from e2enet_medical_amd.experiment_planning.experiment_planner_baseline_3DUNet import ExperimentPlanner
    from e2enet_medical_amd.inference.predict import save_softmax_npz
    from e2enet_medical_amd.preprocessing import GenericPreprocessor, ImageCropper, run_preprocessing
    for fn in (deflate.raw_deflate, deflate.gzip_member, deflate.savez, deflate.npz_parts):
        assert inspect.signature(fn).parameters["codes"].default == "fixed", fn
    for fn in (GenericPreprocessor.run, run_preprocessing, ImageCropper.run_cropping, ImageCropper.load_crop_save, crop,
               ExperimentPlanner.run_preprocessing):
        assert inspect.signature(fn).parameters["device_deflate"].default is False, fn
    assert deflate.codes_of(False) is None and deflate.codes_of(True) == "fixed" and deflate.codes_of("dynamic") == "dynamic"
    with pytest.raises(ValueError, match="huffman"):
        deflate.codes_of("huffman")
    host = torch.zeros(8, dtype=torch.uint8)
    for call in (lambda: deflate.raw_deflate(host, codes="huffman"), lambda: deflate.gzip_member(b"", host, codes="huffman"),
                 lambda: deflate.savez(str(tmp_path / "a.npz"), codes="huffman", x=host),
                 lambda: deflate.npz_parts(codes="huffman", x=host), lambda: deflate.chunk_kinds(host, codes="huffman")):
        with pytest.raises(ValueError, match="codes 'huffman'"):
            call()
    # a host tensor with device_deflate="dynamic" is refused the way True is
    for flag in (True, "dynamic"):
        with pytest.raises(ValueError, match="device tensor"):
            nifti.write(torch.zeros((2, 3, 4), dtype=torch.uint8), str(tmp_path / "a.nii.gz"), None, device_deflate=flag)
        with pytest.raises(ValueError, match="device tensor"):
            nifti.write(np.zeros((2, 3, 4), dtype=np.uint8), str(tmp_path / "a.nii.gz"), None, device_deflate=flag)
        with pytest.raises(ValueError, match="device tensor"):
            save_softmax_npz(torch.zeros((2, 3, 4, 5), dtype=torch.float16), str(tmp_path / "a.npz"), {}, device_deflate=flag)
        with pytest.raises(ValueError, match="device tensor"):
            deflate.raw_deflate(host, codes=deflate.codes_of(flag))
    with pytest.raises(ValueError, match="huffman"):
        nifti.write(torch.zeros((2, 3, 4), dtype=torch.uint8), str(tmp_path / "a.nii.gz"), None, device_deflate="huffman")
    assert not (tmp_path / "a.nii.gz").exists() and not (tmp_path / "a.npz").exists()


def test_write_parts_writes_what_it_is_given(tmp_path):
    """the writer thread's half: the parts of a ``.npz`` (here from host streams) land in the file in order, ``.npz`` appended"""
    from e2enet_medical_amd import deflate
    a = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = c.compress(a.tobytes()) + c.flush(zlib.Z_SYNC_FLUSH)
    header = deflate.npy_header(a.dtype, a.shape)
    members = [("data",) + deflate.member_stream(header, body, zlib.crc32(a.tobytes()), a.nbytes)]
    parts = deflate.zip_bytes_parts([(k + ".npy", s, crc, n) for k, s, crc, n in members])
    deflate.write_parts(str(tmp_path / "case"), parts)
    deflate.write_npz(str(tmp_path / "same.npz"), members)
    assert open(str(tmp_path / "case.npz"), "rb").read() == b"".join(parts) == open(str(tmp_path / "same.npz"), "rb").read()
    assert np.array_equal(np.load(str(tmp_path / "case.npz"))["data"], a)
