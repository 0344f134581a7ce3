"""The OpenEXR cases shared by tests/test_exr_cpu.py and tests/test_exr_gpu.py, and `unpack_hdr_reference`, the float64 restatement
of r3dg_view_unpack_hdr.  Each case is the smallest shape at which one step of the decode can still go wrong; each is written in
HALF and in FLOAT under NONE, ZIPS and ZIP by tests/exr_writer.py.

    1x1                  smallest file                       3x1              odd sample count
    5x17                 a last chunk of one row             33x16, 33x32     exactly one and two full chunks, odd width
    64x40 A,B,G,R,Z      keep R,G,B; skip before, between and after
    64x40 origin (7,-3)  dataWindow origin                   64x40 decreasing chunks placed by their own y
    257x33 noise         uniform random bit patterns: deflate cannot shrink them, at least one chunk is stored raw (asserted by
                         the tests); carries NaN, inf and denormals
    1024x16 ramp         a chunk of 48-192 KB crossing many 4 KB scan tiles: the carry between tiles and waves
    2048x16 four FLOAT   a 512 KB chunk, larger than LDS (FLOAT only: the case is about the chunk's size)
"""
import os

import numpy as np

from tests import exr_writer

COMPRESSIONS = ("NONE", "ZIPS", "ZIP")
DTYPES = {"HALF": np.float16, "FLOAT": np.float32}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN_EXR = os.path.join(GOLDEN, "envmap3_rows96_127.exr")

# name -> (width, height, channel names, origin, decreasing, content, sample types)
SHAPES = {
    "1x1": (1, 1, "BGR", (0, 0), False, "smooth", ("HALF", "FLOAT")),
    "3x1": (3, 1, "BGR", (0, 0), False, "smooth", ("HALF", "FLOAT")),
    "5x17": (5, 17, "BGR", (0, 0), False, "smooth", ("HALF", "FLOAT")),
    "33x16": (33, 16, "BGR", (0, 0), False, "smooth", ("HALF", "FLOAT")),
    "33x32": (33, 32, "BGR", (0, 0), False, "smooth", ("HALF", "FLOAT")),
    "64x40_abgrz": (64, 40, "ABGRZ", (0, 0), False, "smooth", ("HALF", "FLOAT")),
    "64x40_origin": (64, 40, "BGR", (7, -3), False, "smooth", ("HALF", "FLOAT")),
    "64x40_decreasing": (64, 40, "BGR", (0, 0), True, "smooth", ("HALF", "FLOAT")),
    "257x33_noise": (257, 33, "BGR", (0, 0), False, "noise", ("HALF", "FLOAT")),
    "1024x16_ramp": (1024, 16, "BGR", (0, 0), False, "ramp", ("HALF", "FLOAT")),
    "2048x16_four_float": (2048, 16, "ABGR", (0, 0), False, "ramp", ("FLOAT",)),
}
CASES = [(name, kind, compression) for name, shape in SHAPES.items() for kind in shape[6] for compression in COMPRESSIONS]


def planes_of(name, kind):
    """{channel: [H,W] array of the case's sample type}: seeded, the same in every process."""
    W, H, channels, _origin, _decreasing, content, _kinds = SHAPES[name]
    dtype = np.dtype(DTYPES[kind])
    rng = np.random.RandomState(sum(map(ord, name)) * 7 + dtype.itemsize)
    planes = {}
    for j, c in enumerate(channels):
        y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        if content == "noise":                                # every bit pattern: NaN payloads, inf, denormals
            bits = rng.randint(0, 1 << 16, size=(H, W, dtype.itemsize // 2)).astype(np.uint16)
            plane = np.ascontiguousarray(bits).view(dtype).reshape(H, W).copy()
            info = np.finfo(dtype)                            # ... and, whatever the draw held: inf, a denormal, a NaN payload
            plane[0, :4] = [np.inf, -np.inf, info.smallest_subnormal, -3 * info.smallest_subnormal]
            plane.view(np.uint16 if dtype.itemsize == 2 else np.uint32)[0, 4] = 0x7e55 if dtype.itemsize == 2 else 0x7fc12345
            planes[c] = plane
        elif content == "ramp":
            planes[c] = ((x + 3 * y + 11 * j) / float(W + 3 * H + 44) * 4.0).astype(dtype)
        else:                                                 # smooth, 0..3 in steps of 1/64: deflate shrinks it in both types
            planes[c] = (np.round((1.5 + 1.5 * np.sin(0.37 * x + 0.61 * y + j)) * 64) / 64).astype(dtype)
    return planes


def write_case(directory, name, kind, compression):
    """-> (path, planes, number of chunks stored raw)."""
    _W, _H, _channels, origin, decreasing, _content, _kinds = SHAPES[name]
    planes = planes_of(name, kind)
    path = os.path.join(str(directory), "%s_%s_%s.exr" % (name, kind, compression))
    stored_raw = exr_writer.write_exr(path, planes, compression, origin=origin, decreasing=decreasing)
    return path, planes, stored_raw


def bits_of(a):
    """The integer view of float16 / float32 samples (NaN payloads compare)."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype.itemsize == 2 else np.uint32)


# ---- the float64 restatement of r3dg_view_unpack_hdr ---------------------------------------------------------------------------
THRESHOLD = float(np.float32(0.0031308))                       # the float32-rounded constants NumPy uses beside a float32 array
HAND_PICKED = np.array([0.0, -0.25, np.nextafter(np.float32(0.0031308), np.float32(0)), np.float32(0.0031308),
                        np.nextafter(np.float32(0.0031308), np.float32(1)), 1.0, 65504.0], np.float32)


def srgb_float32(x):
    """The reference's own arithmetic (utils/graphics_utils.py rgb_to_srgb(clip=False) on a float32 NumPy array), float32."""
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        return np.where(x > 0.0031308, np.power(np.maximum(x, 0.0031308), 1.0 / 2.4) * 1.055 - 0.055, 12.92 * x)


def srgb_float64(x):
    """The same curve in float64 on the float32 samples, with the float32-rounded constants."""
    x = np.asarray(x, np.float32).astype(np.float64)
    c = lambda v: float(np.float32(v))
    with np.errstate(all="ignore"):
        return np.where(x > THRESHOLD, np.power(np.maximum(x, THRESHOLD), c(1.0 / 2.4)) * c(1.055) - c(0.055), c(12.92) * x)


def power_unit(x):
    """The rounding scale of a power-branch element: 2^-24 * 1.055 * x^(1/2.4), the largest intermediate of the curve."""
    x = np.asarray(x, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        return 2.0 ** -24 * 1.055 * np.power(np.maximum(x, THRESHOLD), 1.0 / 2.4)


def reference_deviation(x):
    """c_ref over the samples x: the largest |float32 arithmetic - float64 value| on the power branch, in power_unit units; and
    the boolean array of the power-branch samples."""
    x = np.asarray(x, np.float32).reshape(-1)
    power = x > np.float32(0.0031308)
    return float(np.max(np.abs(srgb_float32(x)[power] - srgb_float64(x)[power]) / power_unit(x[power]))), power


def golden_planes():
    """The golden crop as the planar view [3,32,500] float32 (R,G,B)."""
    from relightable3dgaussian_amd import exr
    return np.ascontiguousarray(exr.decode_reference(GOLDEN_EXR).transpose(2, 0, 1))


def unpack_hdr_reference(view, mask_bytes, background):
    """view [3,H,W] float16 / float32 (planar R,G,B), mask_bytes [H,W] uint8 or None, background 3 floats -> (image [3,H,W]
    float64, mask [1,H,W] float64): m = byte > 0, image = m ? clamp(srgb(x), 0, 1) : background, mask = m; without a mask plane
    the image alone and an all-ones mask.  A NaN sample stays NaN (torch.clamp keeps it)."""
    y = srgb_float64(np.asarray(view).astype(np.float32))
    with np.errstate(all="ignore"):
        y = np.where(np.isnan(y), y, np.clip(y, 0.0, 1.0))
    m = np.ones(y.shape[1:], bool) if mask_bytes is None else np.asarray(mask_bytes) > 0
    bg = np.asarray(background, np.float32).astype(np.float64).reshape(3, 1, 1)
    return np.where(m[None], y, bg), m[None].astype(np.float64)
