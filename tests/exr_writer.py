"""A NumPy + zlib writer of OpenEXR scanline files, TEST SIDE ONLY (the product writes no EXR): compression NONE / ZIPS / ZIP, HALF or
FLOAT samples, any channel set, any dataWindow origin, either line order.  A ZIP / ZIPS chunk that deflate does not shrink is
stored raw, as the format requires.  It is not trusted: tests/test_exr_cpu.py pins exr.decode_reference to reference data first
and then requires every file written here to come back bit for bit through it.

    write_exr(path, {"R": r, "G": g, "B": b}, compression="ZIP", origin=(0, 0), decreasing=False) -> number of chunks stored raw
"""
import struct
import zlib

import numpy as np

_COMPRESSION = {"NONE": (0, 1), "ZIPS": (2, 1), "ZIP": (3, 16)}
_TYPES = {np.dtype("float16"): 1, np.dtype("float32"): 2}


def apply_split_and_predictor(raw):
    """Raw chunk bytes (uint8 array) -> what zlib deflates: even bytes then odd bytes, then d[i] = t[i] - t[i-1] + 128 mod 256."""
    t = np.concatenate([raw[0::2], raw[1::2]]).astype(np.int64)
    d = t.copy()
    d[1:] = (t[1:] - t[:-1] + 128) % 256
    return d.astype(np.uint8).tobytes()


def _attribute(name, kind, value):
    return name.encode() + b"\0" + kind.encode() + b"\0" + struct.pack("<i", len(value)) + value


def write_exr(path, planes, compression="ZIP", origin=(0, 0), decreasing=False, level=6):
    """`planes`: {channel name: [H,W] array}, all float16 or all float32 (their bit patterns are stored untouched).  Channels are
    stored in alphabetical order.  -> how many chunks were stored raw."""
    names = sorted(planes)
    arrays = [np.ascontiguousarray(planes[n]) for n in names]
    dtype = arrays[0].dtype
    assert dtype in _TYPES and all(a.dtype == dtype and a.shape == arrays[0].shape and a.ndim == 2 for a in arrays)
    H, W = arrays[0].shape
    code, rows_per_chunk = _COMPRESSION[compression]
    x0, y0 = origin
    window = struct.pack("<4i", x0, y0, x0 + W - 1, y0 + H - 1)
    chlist = b"".join(n.encode() + b"\0" + struct.pack("<iB3xii", _TYPES[dtype], 0, 1, 1) for n in names) + b"\0"
    header = struct.pack("<iI", 20000630, 2) + b"".join([
        _attribute("channels", "chlist", chlist), _attribute("compression", "compression", bytes([code])),
        _attribute("dataWindow", "box2i", window), _attribute("displayWindow", "box2i", window),
        _attribute("lineOrder", "lineOrder", bytes([1 if decreasing else 0])),
        _attribute("pixelAspectRatio", "float", struct.pack("<f", 1.0)),
        _attribute("screenWindowCenter", "v2f", struct.pack("<2f", 0.0, 0.0)),
        _attribute("screenWindowWidth", "float", struct.pack("<f", 1.0))]) + b"\0"
    chunks, stored_raw = [], 0
    for first in range(0, H, rows_per_chunk):
        rows = min(rows_per_chunk, H - first)
        # rows of channel-planar samples, little endian
        raw = np.stack([a[first:first + rows].astype(dtype.newbyteorder("<"), copy=False) for a in arrays], axis=1)
        raw = np.frombuffer(raw.tobytes(), np.uint8)
        payload = raw.tobytes()
        if code:
            packed = zlib.compress(apply_split_and_predictor(raw), level)
            if len(packed) < len(payload):
                payload = packed
            else:
                stored_raw += 1
        chunks.append(struct.pack("<ii", y0 + first, len(payload)) + payload)
    # the offset table is in increasing y; the chunks themselves follow in the file's line order
    order = list(range(len(chunks)))[::-1] if decreasing else list(range(len(chunks)))
    at, offsets = len(header) + 8 * len(chunks), [0] * len(chunks)
    for i in order:
        offsets[i] = at
        at += len(chunks[i])
    with open(path, "wb") as fh:
        fh.write(header + struct.pack("<%dQ" % len(chunks), *offsets) + b"".join(chunks[i] for i in order))
    return stored_raw
