"""OpenEXR scanline files, the container side on the host: what the Synthetic4Relight train split (`*_rgb.exr`,
scene/dataset_readers.py:526-604) and the reference's `env_map/envmap3.exr` are.  No EXR library is needed or used: the header is
a list of named attributes, a chunk is (y, size, payload), and a ZIP payload is zlib over a byte predictor over an even / odd byte
split.

    header = read_header(path)                        # channels, compression, data window, line order, chunk offset table
    image = read_image(path)                          # [H,W,3] float32 R,G,B: what pyexr.open(path).get()[..., :3] yields
    samples = decode_reference(path, ("R","G","B"))   # the same in the file's own sample type; the yardstick of the device path
    table, nbytes = inflate_chunks(path, header, out) # the product path: zlib only; the rest is r3dg_exr_unpack_chunks

In scope: single-part scanline files of version 2; compression NONE (0), ZIPS (2: one row per chunk) and ZIP (3: 16 rows per
chunk); HALF or FLOAT samples, one type for the whole file; x / y sampling 1; a dataWindow with any origin; either line order
(every chunk carries its own y and is placed by it).  A ZIP / ZIPS chunk whose stored size is not smaller than its raw size is
stored raw: no predictor, no byte split.  Everything else raises a RuntimeError naming the file and the feature: RLE, PIZ, PXR24,
B44, B44A, DWAA, DWAB, UINT samples, mixed sample types, subsampled channels, tiled, multipart and deep files, long names.  PIZ (a
Huffman + wavelet codec; the reference's envmap6.exr and envmap12.exr) is out of scope on purpose: nothing here could check it.

A ZIP chunk, after inflate, d[0..n): t[0] = d[0], t[i] = (t[i-1] + d[i] - 128) mod 256 (the predictor: a running sum over the
whole chunk), then raw[2j] = t[j], raw[2j+1] = t[half + j] with half = (n + 1) / 2 (the split into even bytes then odd bytes), and
raw is rows of channel-planar little-endian samples: row 0 channel 0 x 0..W-1, row 0 channel 1, ..., the channels in the file's
(alphabetical) order.
"""
import struct
import types
import zlib

import numpy as np

MAGIC = 20000630
COMPRESSIONS = ("NONE", "RLE", "ZIPS", "ZIP", "PIZ", "PXR24", "B44", "B44A", "DWAA", "DWAB")
ROWS_PER_CHUNK = {"NONE": 1, "ZIPS": 1, "ZIP": 16}            # the codecs that are read
SAMPLE_TYPES = ("UINT", "HALF", "FLOAT")
SAMPLE_DTYPES = {"HALF": np.dtype("<f2"), "FLOAT": np.dtype("<f4")}
LINE_ORDERS = ("INCREASING_Y", "DECREASING_Y", "RANDOM_Y")
ALIGN = 16                                                     # every inflated chunk starts at a multiple of this
_FLAGS = ((0x200, "tiled"), (0x400, "long names"), (0x800, "deep (non-image) data"), (0x1000, "multipart"))


def _cstring(data, at, path):
    end = data.find(b"\0", at)
    if end < 0:
        raise RuntimeError("%s: the header ends inside a name (truncated file)" % path)
    return data[at:end].decode("latin-1"), end + 1


def read_header(path):
    """-> namespace: channels [(name, "HALF" | "FLOAT")] in the file's order, compression (a name of COMPRESSIONS), data_window
    (xMin, yMin, xMax, yMax), line_order (a name of LINE_ORDERS), width, height, bytes_per_sample, rows_per_chunk, offsets (the
    chunk offset table, uint64 [chunks], as the file holds it) and attributes {name: (type, raw bytes)}.  RuntimeError naming the
    file and the feature for anything out of scope (module docstring), and for an offset table that is cut short or points outside
    the file."""
    with open(path, "rb") as fh:
        data = fh.read()
    if len(data) < 8 or struct.unpack_from("<i", data, 0)[0] != MAGIC:
        raise RuntimeError("%s: not an OpenEXR file (magic number)" % path)
    version = struct.unpack_from("<I", data, 4)[0]
    if version & 0xff != 2:
        raise RuntimeError("%s: OpenEXR version %d is not read (version 2 only)" % (path, version & 0xff))
    for bit, what in _FLAGS:
        if version & bit:
            raise RuntimeError("%s: %s files are not read (single-part scanline files only)" % (path, what))
    attributes, at = {}, 8
    while True:
        if at >= len(data):
            raise RuntimeError("%s: the header does not end (truncated file)" % path)
        if data[at] == 0:
            at += 1
            break
        name, at = _cstring(data, at, path)
        kind, at = _cstring(data, at, path)
        if at + 4 > len(data):
            raise RuntimeError("%s: the header does not end (truncated file)" % path)
        size = struct.unpack_from("<i", data, at)[0]
        attributes[name] = (kind, data[at + 4:at + 4 + size])
        at += 4 + size
    for name in ("channels", "compression", "dataWindow", "lineOrder"):
        if name not in attributes:
            raise RuntimeError("%s: the header has no %s attribute" % (path, name))
    code = attributes["compression"][1][0]
    compression = COMPRESSIONS[code] if code < len(COMPRESSIONS) else "code %d" % code
    if compression not in ROWS_PER_CHUNK:
        raise RuntimeError("%s: %s compression is not read (NONE, ZIPS and ZIP only)" % (path, compression))
    channels, raw, c = [], attributes["channels"][1], 0
    while c < len(raw) and raw[c] != 0:
        name, c = _cstring(raw, c, path)
        kind, _linear, xs, ys = struct.unpack_from("<iB3xii", raw, c)
        c += 16
        if kind not in (1, 2):
            raise RuntimeError("%s: channel %s holds %s samples; only HALF and FLOAT are read" % (
                path, name, "UINT" if kind == 0 else "type %d" % kind))
        if (xs, ys) != (1, 1):
            raise RuntimeError("%s: channel %s is subsampled (%d x %d); only sampling 1 is read" % (path, name, xs, ys))
        channels.append((name, SAMPLE_TYPES[kind]))
    if not channels:
        raise RuntimeError("%s: no channels" % path)
    if len(set(kind for _, kind in channels)) != 1:
        raise RuntimeError("%s: mixed sample types (%s) are not read; one type for the whole file" % (
            path, ", ".join("%s %s" % c for c in channels)))
    x0, y0, x1, y1 = struct.unpack_from("<4i", attributes["dataWindow"][1], 0)
    width, height = x1 - x0 + 1, y1 - y0 + 1
    if width < 1 or height < 1:
        raise RuntimeError("%s: an empty dataWindow %s" % (path, (x0, y0, x1, y1)))
    order = attributes["lineOrder"][1][0]
    rows = ROWS_PER_CHUNK[compression]
    chunks = -(-height // rows)
    if at + 8 * chunks > len(data):
        raise RuntimeError("%s: the chunk offset table is cut short (%d chunks of 8 bytes from byte %d, the file has %d bytes)"
                           % (path, chunks, at, len(data)))
    offsets = np.frombuffer(data, "<u8", chunks, at).copy()
    if int(offsets.min()) < at + 8 * chunks or int(offsets.max()) + 8 > len(data):
        raise RuntimeError("%s: the chunk offset table points outside the chunk data (an incomplete file)" % path)
    return types.SimpleNamespace(path=str(path), channels=channels, compression=compression, data_window=(x0, y0, x1, y1),
                                 line_order=LINE_ORDERS[order] if order < 3 else "code %d" % order, width=width, height=height,
                                 bytes_per_sample=SAMPLE_DTYPES[channels[0][1]].itemsize, rows_per_chunk=rows, offsets=offsets,
                                 attributes=attributes, nbytes=len(data))


def channel_indexes(header, channels):
    """The file-channel index of each name of `channels`; RuntimeError naming the file and the missing channel."""
    names = [n for n, _ in header.channels]
    for c in channels:
        if c not in names:
            raise RuntimeError("%s: no channel %s (the file has %s)" % (header.path, c, ", ".join(names)))
    return [names.index(c) for c in channels]


def _chunks(header, data):
    """(first row, rows, payload bytes, stored raw) of every chunk, in the order of the offset table."""
    y0, y1 = header.data_window[1], header.data_window[3]
    row_bytes = header.width * len(header.channels) * header.bytes_per_sample
    for offset in header.offsets.tolist():
        y, size = struct.unpack_from("<ii", data, offset)
        rows = min(header.rows_per_chunk, y1 - y + 1)
        if y < y0 or y > y1 or (y - y0) % header.rows_per_chunk:
            raise RuntimeError("%s: a chunk at y = %d outside the dataWindow's chunk grid" % (header.path, y))
        raw = rows * row_bytes
        if size < 0 or size > raw or offset + 8 + size > len(data) or (header.compression == "NONE" and size != raw):
            raise RuntimeError("%s: the chunk at y = %d holds %d bytes (%d raw; the file has %d)" % (
                header.path, y, size, raw, len(data)))
        yield y - y0, rows, data[offset + 8:offset + 8 + size], size == raw


def inflate_chunks(path, header=None, out=None):
    """The serial part of the decode, for the device path: every chunk of the file zlib-inflated (a chunk stored raw: copied) into
    the uint8 array `out` (None: a new one of `inflated_nbytes(header)`), chunk after chunk in the order of the offset table, each
    at a multiple of 16 bytes.  -> (table int32 [chunks,4]: byte offset, first row, rows, stored-raw flag -- what
    r3dg_exr_unpack_chunks takes --, bytes used)."""
    header = header or read_header(path)
    with open(path, "rb") as fh:
        data = fh.read()
    need = inflated_nbytes(header)
    out = np.empty(need, np.uint8) if out is None else out
    if out.dtype != np.uint8 or out.ndim != 1 or out.size < need:
        raise RuntimeError("inflate_chunks: the output must be a uint8 array of at least %d bytes" % need)
    table, at = np.zeros((len(header.offsets), 4), np.int32), 0
    for i, (row, rows, payload, stored_raw) in enumerate(_chunks(header, data)):
        raw = rows * header.width * len(header.channels) * header.bytes_per_sample
        chunk = payload if stored_raw else zlib.decompress(payload)
        if len(chunk) != raw:
            raise RuntimeError("%s: the chunk at row %d inflates to %d bytes, not %d" % (header.path, row, len(chunk), raw))
        out[at:at + raw] = np.frombuffer(chunk, np.uint8)
        table[i] = (at, row, rows, int(stored_raw))
        at += -(-raw // ALIGN) * ALIGN
    return table, at


def inflated_nbytes(header):
    """Bytes `inflate_chunks` fills: the raw size of every chunk rounded up to 16."""
    row_bytes = header.width * len(header.channels) * header.bytes_per_sample
    full, last = divmod(header.height, header.rows_per_chunk)
    pad = lambda n: -(-n // ALIGN) * ALIGN
    return full * pad(header.rows_per_chunk * row_bytes) + (pad(last * row_bytes) if last else 0)


def undo_predictor_and_split(chunk):
    """An inflated ZIP / ZIPS chunk (bytes) -> its raw bytes (uint8 array): the running sum mod 256, then even / odd interleave."""
    d = np.frombuffer(chunk, np.uint8).astype(np.int64)
    t = ((np.cumsum(d) - 128 * np.arange(d.size)) % 256).astype(np.uint8)
    half = (d.size + 1) // 2
    raw = np.empty(d.size, np.uint8)
    raw[0::2] = t[:half]
    raw[1::2] = t[half:]
    return raw


def decode_reference(path, channels=("R", "G", "B")):
    """The whole decode in NumPy + zlib -> [H,W,len(channels)] in the file's sample type (float16 or float32), the bit patterns
    exactly as stored.  Slow; not on the product path; the yardstick of r3dg_exr_unpack_chunks and of the tests."""
    header = read_header(path)
    keep = channel_indexes(header, channels)
    with open(path, "rb") as fh:
        data = fh.read()
    dtype = SAMPLE_DTYPES[header.channels[0][1]]
    out = np.zeros((header.height, header.width, len(keep)), dtype)
    filled = np.zeros(header.height, bool)
    for row, rows, payload, stored_raw in _chunks(header, data):
        raw = np.frombuffer(payload, np.uint8) if stored_raw else undo_predictor_and_split(zlib.decompress(payload))
        if raw.size != rows * header.width * len(header.channels) * dtype.itemsize:
            raise RuntimeError("%s: the chunk at row %d inflates to %d bytes" % (header.path, row, raw.size))
        planes = raw.view(dtype).reshape(rows, len(header.channels), header.width)
        out[row:row + rows] = planes[:, keep, :].transpose(0, 2, 1)
        filled[row:row + rows] = True
    if not filled.all():
        raise RuntimeError("%s: no chunk holds row %d" % (header.path, int(np.argmin(filled))))
    return out


def read_image(path, channels=("R", "G", "B")):
    """[H,W,3] float32: what `pyexr.open(path).get()[..., :3]` yields (HALF samples widened exactly).  This is also what an `.npy`
    environment map holds: np.save("envmap3.npy", read_image("envmap3.exr")) is the bridge to relighting.load_envmap."""
    return decode_reference(path, channels).astype(np.float32)
