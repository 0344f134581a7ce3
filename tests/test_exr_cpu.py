"""The OpenEXR reader and the Synthetic4Relight reader on the host (relightable3dgaussian_amd/exr.py, dataset.read_syn4relight,
dataset.detect_layout).  The chain of trust: exr.decode_reference is pinned to the reference's own record of a decode (the PNG twin
of env_map/envmap3.exr, tests/golden/make_exr_golden.py); the test-side writer tests/exr_writer.py must round-trip through it; the
device path (tests/test_exr_gpu.py) is pinned to it bit for bit.

`c_ref` (test 7): the largest distance of the reference's float32 sRGB arithmetic from the float64 value of the same expression,
over the golden crop's power-branch samples, in units of 2^-24 * 1.055 * x^(1/2.4): measured 2.845 here (NumPy 2.2, x86-64).  It is
printed by the test, and tests/test_exr_gpu.py allows the device c_ref + 2 of the same units."""
import json
import os
import struct

import numpy as np
import pytest

from relightable3dgaussian_amd import dataset, exr
from tests import exr_cases, exr_writer


# ---- 1, 2. the golden crop ---------------------------------------------------------------------------------------------------------
def test_decoder_reproduces_the_references_png_twin():
    png_rows = np.load(os.path.join(exr_cases.GOLDEN, "exr_reference.npz"))["png_rows"]
    samples = exr.decode_reference(exr_cases.GOLDEN_EXR)                           # [32,500,3] R,G,B
    assert samples.dtype == np.float32 and samples.shape == (32, 500, 3)
    # env_map/convert.py: rgb_to_srgb (clip=True) -> * 255 -> astype(uint8), all in float32
    srgb = np.clip(exr_cases.srgb_float32(samples), 0.0, 1.0)
    assert srgb.dtype == np.float32
    got = (srgb * 255).astype(np.uint8)
    assert png_rows.shape == got.shape and int((got == png_rows).sum()) == 48000
    assert float((samples > 1.0).mean()) > 0.3 and float(samples.max()) == 4.0       # values the PNG clips are in the fixture
    assert np.array_equal(exr.read_image(exr_cases.GOLDEN_EXR), samples)


def test_header_fields_of_the_golden_file():
    h = exr.read_header(exr_cases.GOLDEN_EXR)
    assert h.channels == [("B", "FLOAT"), ("G", "FLOAT"), ("R", "FLOAT")]
    assert h.compression == "ZIP" and h.rows_per_chunk == 16 and h.bytes_per_sample == 4
    assert h.data_window == (0, 0, 499, 31) and (h.width, h.height) == (500, 32) and h.line_order == "INCREASING_Y"
    assert h.offsets.dtype == np.uint64 and h.offsets.shape == (2,)
    with open(exr_cases.GOLDEN_EXR, "rb") as fh:
        data = fh.read()
    ys_sizes = [struct.unpack_from("<ii", data, int(o)) for o in h.offsets]
    assert [y for y, _ in ys_sizes] == [0, 16] and sum(s for _, s in ys_sizes) + 16 == 183517
    assert int(h.offsets[1]) == int(h.offsets[0]) + 8 + ys_sizes[0][1] and int(h.offsets[1]) + 8 + ys_sizes[1][1] == len(data)
    assert exr.channel_indexes(h, ("R", "G", "B")) == [2, 1, 0]
    assert exr.inflated_nbytes(h) == 2 * 16 * 500 * 3 * 4


# ---- 3. the writer round trip --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind,compression", exr_cases.CASES)
def test_writer_round_trips_through_the_decoder(tmp_path, name, kind, compression):
    W, H, channels, origin, decreasing, _content, _kinds = exr_cases.SHAPES[name]
    path, planes, stored_raw = exr_cases.write_case(tmp_path, name, kind, compression)
    h = exr.read_header(path)
    assert [c for c, _ in h.channels] == sorted(channels) and all(t == kind for _, t in h.channels)
    assert h.compression == compression and (h.width, h.height) == (W, H)
    assert h.data_window == (origin[0], origin[1], origin[0] + W - 1, origin[1] + H - 1)
    assert h.line_order == ("DECREASING_Y" if decreasing else "INCREASING_Y")
    if decreasing and len(h.offsets) > 1:
        assert int(h.offsets[0]) > int(h.offsets[-1])                                # (the first rows sit last in the file)
    got = exr.decode_reference(path, ("R", "G", "B"))
    assert got.dtype == exr_cases.DTYPES[kind] and got.shape == (H, W, 3)
    for j, c in enumerate("RGB"):
        assert np.array_equal(exr_cases.bits_of(got[..., j]), exr_cases.bits_of(planes[c])), (name, kind, compression, c)
    everything = exr.decode_reference(path, tuple(sorted(channels)))
    for j, c in enumerate(sorted(channels)):
        assert np.array_equal(exr_cases.bits_of(everything[..., j]), exr_cases.bits_of(planes[c]))
    if name == "257x33_noise":
        assert (stored_raw >= 1) == (compression != "NONE")                          # deflate cannot shrink it: stored raw
        with np.errstate(invalid="ignore"):
            values = got.astype(np.float64)
        assert np.isnan(values).any() and np.isinf(values).any()
        assert ((np.abs(values) > 0) & (np.abs(values) < float(np.finfo(got.dtype).tiny))).any()       # denormals
    if name in ("33x16", "33x32", "64x40_abgrz", "1024x16_ramp", "2048x16_four_float") and compression != "NONE":
        assert stored_raw == 0                                                       # ... and these do go through the predictor
    # the inflate-only path of the product: the same chunks, each at a multiple of 16 bytes
    table, used = exr.inflate_chunks(path, h)
    assert table.shape == (len(h.offsets), 4) and used == exr.inflated_nbytes(h) and not (table[:, 0] % 16).any()
    assert sorted(table[:, 1].tolist()) == list(range(0, H, h.rows_per_chunk)) and int(table[:, 2].sum()) == H
    assert int(table[:, 3].sum()) == (len(h.offsets) if compression == "NONE" else stored_raw)


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------------
def _written(tmp_path, kinds=None):
    planes = exr_cases.planes_of("5x17", "HALF")
    path = str(tmp_path / "base.exr")
    exr_writer.write_exr(path, planes, "ZIP")
    with open(path, "rb") as fh:
        return path, bytearray(fh.read())


def _patched(tmp_path, data, name="patched.exr"):
    path = str(tmp_path / name)
    with open(path, "wb") as fh:
        fh.write(bytes(data))
    return path


def _compression_at(data):
    return data.index(b"compression\0compression\0") + len(b"compression\0compression\0") + 4


def _channel_type_at(data, channel):
    return data.index(b"channels\0chlist\0") + len(b"channels\0chlist\0") + 4 + 18 * "BGR".index(channel) + 2


@pytest.mark.parametrize("feature,match", [("PIZ", "PIZ"), ("RLE", "RLE"), ("UINT", "UINT"), ("mixed", "mixed sample types"),
                                           ("tiled", "tiled"), ("multipart", "multipart"), ("offsets", "offset table")])
def test_out_of_scope_files_are_refused_by_name(tmp_path, feature, match):
    path, data = _written(tmp_path)
    exr.read_header(path)                                                            # (the unpatched file is read)
    if feature == "PIZ":
        data[_compression_at(data)] = 4
    elif feature == "RLE":
        data[_compression_at(data)] = 1
    elif feature == "UINT":
        data[_channel_type_at(data, "G")] = 0
    elif feature == "mixed":
        data[_channel_type_at(data, "G")] = 2
    elif feature == "tiled":
        data[5] |= 0x02
    elif feature == "multipart":
        data[5] |= 0x10
    else:
        data = data[:int(exr.read_header(path).offsets[0]) - 8 * 2 + 5]              # the file ends inside its offset table
    bad = _patched(tmp_path, data)
    for call in (exr.read_header, exr.decode_reference, exr.read_image):
        with pytest.raises(RuntimeError, match=match) as e:
            call(bad)
        assert "patched.exr" in str(e.value)


# ---- 5, 6. the Synthetic4Relight reader --------------------------------------------------------------------------------------------------
def _syn4_root(tmp_path, z, name="Synthetic4Relight"):
    root = tmp_path / name / "toy"
    (root / "train").mkdir(parents=True)
    W, H = int(z["width"][0]), int(z["height"][0])
    frames = []
    for i, m in enumerate(z["transform_matrix"]):
        exr_writer.write_exr(str(root / "train" / ("%03d_rgb.exr" % i)),
                             {c: np.zeros((H, W), np.float16) for c in "RGB"}, "ZIP")
        frames.append({"file_path": "./train/%03d" % i, "transform_matrix": m.tolist()})
    with open(root / "transforms_train.json", "w") as fh:
        json.dump({"camera_angle_x": float(z["camera_angle_x"]), "frames": frames}, fh)
    return str(root)


def test_read_syn4relight_matches_the_references_reader(tmp_path):
    z = np.load(os.path.join(exr_cases.GOLDEN, "syn4relight_reference.npz"))
    records = dataset.read_syn4relight(_syn4_root(tmp_path, z), "train")
    assert len(records) == 3 and int(z["width"][0]) != int(z["height"][0])
    for j, r in enumerate(records):
        assert r["name"] == str(z["image_name"][j]) and r["path"].endswith("%03d_rgb.exr" % j) and r["mask_path"] is None
        assert (r["width"], r["height"]) == (int(z["width"][j]), int(z["height"][j]))
        np.testing.assert_allclose(r["R"], z["R"][j], rtol=0, atol=1e-12)
        np.testing.assert_allclose(r["T"], z["T"][j], rtol=0, atol=1e-12)
        assert r["FovX"] == float(z["FovX"][j]) and abs(r["FovY"] - float(z["FovY"][j])) <= 1e-12
        assert r["FovY"] != r["FovX"]                                                # (the height is the focal-length base)


def test_detect_layout_knows_the_three_layouts(tmp_path):
    z = np.load(os.path.join(exr_cases.GOLDEN, "syn4relight_reference.npz"))
    assert dataset.detect_layout(_syn4_root(tmp_path, z)) == "syn4relight"
    assert dataset.detect_layout(_syn4_root(tmp_path, z, name="SomethingElse")) == "blender"
    neilf = tmp_path / "dtu"
    (neilf / "inputs").mkdir(parents=True)
    (neilf / "inputs" / "sfm_scene.json").write_text("{}")
    assert dataset.detect_layout(str(neilf)) == "neilf"
    with pytest.raises(RuntimeError):
        dataset.detect_layout(str(tmp_path))


# ---- 7. the float64 restatement of the per-iteration launch ----------------------------------------------------------------------------
def test_unpack_hdr_reference_against_the_references_float32_arithmetic():
    samples = exr_cases.golden_planes()                                                # [3,32,500]
    x = np.concatenate([samples.reshape(-1), exr_cases.HAND_PICKED])
    want32 = exr_cases.srgb_float32(x)
    got64 = exr_cases.srgb_float64(x)
    assert want32.dtype == np.float32 and got64.dtype == np.float64
    linear = ~(x > np.float32(0.0031308))
    assert linear.any() and (~linear).sum() > 40000
    assert np.array_equal(got64[linear].astype(np.float32), want32[linear])            # 12.92 * x: one rounding of an exact product
    c_ref, power = exr_cases.reference_deviation(x)
    assert np.array_equal(power, ~linear)
    print("c_ref = %.3f units of 2^-24 * 1.055 * x^(1/2.4) over %d power-branch samples" % (c_ref, int((~linear).sum())))
    # a unit is at least half an ulp of every intermediate: powf within 1 ulp (2 units), the product and the difference rounded once
    # each (1 unit each), the constant 1/2.4 as float32 on both sides
    assert 0.0 < c_ref <= 4.0
    # the whole restatement: select, clamp, mask
    mask_bytes = np.zeros((32, 500), np.uint8)
    mask_bytes[:, 100:300], mask_bytes[:, 300:] = 1, 255
    for bg in ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)):
        image, mask = exr_cases.unpack_hdr_reference(samples, mask_bytes, bg)
        assert image.shape == (3, 32, 500) and mask.shape == (1, 32, 500) and set(np.unique(mask)) == {0.0, 1.0}
        assert (image[:, :, :100] == bg[0]).all() and (mask[0, :, :100] == 0).all() and (mask[0, :, 100:] == 1).all()
        inside = np.clip(exr_cases.srgb_float64(samples), 0, 1)[:, :, 100:]
        assert np.array_equal(image[:, :, 100:], inside) and float(image.max()) == 1.0
        image, mask = exr_cases.unpack_hdr_reference(samples, None, bg)
        assert (mask == 1).all() and np.array_equal(image, np.clip(exr_cases.srgb_float64(samples), 0, 1))
    hand = exr_cases.unpack_hdr_reference(np.tile(exr_cases.HAND_PICKED.reshape(1, 1, -1), (3, 1, 1)), None, (0, 0, 0))[0][0, 0]
    assert hand[0] == 0 and hand[1] == 0 and hand[6] == 1 and all(0.0404 < hand[j] < 0.0405 for j in (2, 3, 4))
    assert 1 - 2.0 ** -23 < hand[5] < 1                   # (x = 1: float32(1.055) - float32(0.055) is just below 1)


# ---- the device decode's source under the CPU wave emulation -----------------------------------------------------------------------------
_EMU = {}


def _emu_lib(tmp_path_factory):
    import ctypes
    import subprocess
    if "lib" not in _EMU:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        path = str(tmp_path_factory.mktemp("exr_emu") / "libexr_emu.so")
        r = subprocess.run(["g++", "-std=c++20", "-O1", "-pthread", "-shared", "-fPIC", "-I",
                            os.path.join(root, "relightable3dgaussian_amd", "csrc"), os.path.join(root, "tests", "emu", "exr_emu.cpp"),
                            "-o", path], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        _EMU["lib"] = ctypes.CDLL(path)
    return _EMU["lib"]


@pytest.mark.parametrize("name,kind,compression", [
    ("3x1", "HALF", "ZIPS"), ("5x17", "FLOAT", "ZIP"), ("33x32", "HALF", "ZIP"), ("64x40_abgrz", "FLOAT", "ZIP"),
    ("64x40_decreasing", "HALF", "ZIPS"), ("257x33_noise", "HALF", "ZIP"), ("1024x16_ramp", "HALF", "ZIP"),
    ("1024x16_ramp", "FLOAT", "ZIP"), ("2048x16_four_float", "FLOAT", "ZIP"), ("golden", "FLOAT", "ZIP")])
def test_decode_kernels_source_runs_in_the_cpu_wave_emulation(tmp_path, tmp_path_factory, name, kind, compression):
    """csrc/exr_decode.hpp, the source exr_unpack.hip compiles for gfx950, compiled for the host against tests/emu/exr_emu.cpp
    (every lane a thread, shuffles and __shared__ emulated in lock step): tile sums, carries, the packed wave scan, the byte
    interleave and the plane indexing against decode_reference bit for bit, with canaries behind the planes.  The parity test
    proper runs the same source on the MI355X (tests/test_exr_gpu.py)."""
    import ctypes as C
    lib = _emu_lib(tmp_path_factory)
    path = exr_cases.GOLDEN_EXR if name == "golden" else exr_cases.write_case(tmp_path, name, kind, compression)[0]
    h = exr.read_header(path)
    keep = np.array(exr.channel_indexes(h, ("R", "G", "B")), np.int32)
    staging = np.zeros(exr.inflated_nbytes(h) + 16, np.uint8)
    staging = staging[(-staging.ctypes.data) % 16:][:exr.inflated_nbytes(h)]            # 16-byte aligned, exact size
    table, used = exr.inflate_chunks(path, h, staging)
    tiles = -(-(h.rows_per_chunk * h.width * len(h.channels) * h.bytes_per_sample // 2) // 4096)
    sums = np.full(len(table) * 2 * tiles, 0xDEAD, np.uint32)
    n = 3 * h.height * h.width * h.bytes_per_sample
    planes = np.full(n + 64, 0xAB, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    lib.emu_exr_unpack_chunks(C.c_int(h.width), C.c_int(h.height), C.c_int(len(h.channels)), C.c_int(h.bytes_per_sample),
                              C.c_int(len(table)), C.c_int(h.rows_per_chunk), p(staging), C.c_longlong(used), p(table), C.c_int(3),
                              p(keep), p(sums), p(planes))
    assert (planes[n:] == 0xAB).all()
    got = planes[:n].view(np.uint16 if h.bytes_per_sample == 2 else np.uint32).reshape(3, h.height, h.width)
    assert np.array_equal(got, exr_cases.bits_of(exr.decode_reference(path)).transpose(2, 0, 1))
