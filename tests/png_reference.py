"""The device PNG encoder's format (include/r3dg_hip.h "r3dg_png_encode") restated in plain loops: NumPy, zlib and struct only.
It is the yardstick for the device, byte for byte, and takes nothing from the package but a table's code lengths
(`table.lengths`, the 286 literal/length lengths, and `table.cl_lengths`, the 19 lengths of the code-length code): the canonical
codes, the block header and every bit of the stream are built here."""
import struct
import zlib

import numpy as np

CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LENGTH_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)


def _as_image(x):
    x = np.asarray(x)
    assert x.dtype == np.uint8 and x.ndim == 3 and 1 <= x.shape[2] <= 4
    return x


def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    if pa <= pb and pa <= pc:
        return a
    return b if pb <= pc else c


def filter_rows(x):
    """-> (filtered stream uint8 [H, 1 + W*C], the filter type of every row)."""
    x = _as_image(x)
    H, W, C = x.shape
    n = W * C
    rows = x.reshape(H, n).astype(np.int64)
    out = np.zeros((H, n + 1), np.uint8)
    types = []
    for y in range(H):
        cur = rows[y]
        up = rows[y - 1] if y > 0 else np.zeros(n, np.int64)
        cand = np.zeros((5, n), np.int64)
        for i in range(n):
            a = cur[i - C] if i >= C else 0
            b = up[i]
            c = up[i - C] if i >= C else 0
            v = cur[i]
            cand[0, i] = v
            cand[1, i] = v - a
            cand[2, i] = v - b
            cand[3, i] = v - (a + b) // 2
            cand[4, i] = v - paeth(a, b, c)
        cand &= 255
        scores = [int(np.where(cand[t] < 128, cand[t], 256 - cand[t]).sum()) for t in range(5)]
        t = scores.index(min(scores))                       # (the first minimum: ties go to the lowest type)
        types.append(t)
        out[y, 0] = t
        out[y, 1:] = cand[t]
    return out, types


def rows_per_segment(H, row_bytes):
    assert row_bytes <= 65535
    return max(1, min(H, 16384 // row_bytes))


def run_tokens(n):
    """The tokens of one run of n equal bytes: ('lit',) and ('match', length) entries."""
    tokens = [("lit",)]
    rest = n - 1
    while rest >= 261 or rest == 258:
        tokens.append(("match", 258))
        rest -= 258
    if rest in (259, 260):
        tokens += [("match", rest - 3), ("match", 3)]
    elif rest >= 3:
        tokens.append(("match", rest))
    else:
        tokens += [("lit",)] * rest
    return tokens


def parse(data):
    """Segment bytes -> [('lit', byte) | ('match', length)] (every match has distance 1)."""
    data = bytes(data)
    tokens, i = [], 0
    while i < len(data):
        j = i
        while j < len(data) and data[j] == data[i]:
            j += 1
        tokens += [("lit", data[i]) if t[0] == "lit" else t for t in run_tokens(j - i)]
        i = j
    return tokens


def canonical_codes(lengths):
    codes, code = [0] * len(lengths), 0
    for bits in range(1, max(lengths) + 1):
        for s, n in enumerate(lengths):
            if n == bits:
                codes[s] = code
                code += 1
        code <<= 1
    return codes


class _Bits:
    def __init__(self):
        self.bits = []

    def field(self, value, n):                              # LSB first
        for i in range(n):
            self.bits.append((value >> i) & 1)

    def code(self, value, n):                               # a Huffman code: MSB first
        for i in range(n - 1, -1, -1):
            self.bits.append((value >> i) & 1)

    def align(self):
        while len(self.bits) % 8:
            self.bits.append(0)

    def tobytes(self):
        assert len(self.bits) % 8 == 0
        return bytes(np.packbits(np.array(self.bits, np.uint8), bitorder="little").tolist())


def write_header(w, table):
    lengths, cl = list(table.lengths), list(table.cl_lengths)
    assert len(lengths) == 286 and len(cl) == 19 and not any(cl[16:])
    cl_codes = canonical_codes(cl)
    hclen = max(i for i, s in enumerate(CL_ORDER) if cl[s]) + 1
    w.field(0, 1), w.field(2, 2), w.field(29, 5), w.field(0, 5), w.field(hclen - 4, 4)
    for s in CL_ORDER[:hclen]:
        w.field(cl[s], 3)
    for n in lengths + [1]:
        w.code(cl_codes[n], cl[n])


def coded_segment(data, table):
    lengths = list(table.lengths)
    codes = canonical_codes(lengths)
    w = _Bits()
    write_header(w, table)
    for t in parse(data):
        if t[0] == "lit":
            w.code(codes[t[1]], lengths[t[1]])
        else:
            k = max(i for i, b in enumerate(LENGTH_BASE) if b <= t[1])
            w.code(codes[257 + k], lengths[257 + k])
            w.field(t[1] - LENGTH_BASE[k], LENGTH_EXTRA[k])
            assert t[1] - LENGTH_BASE[k] < 1 << LENGTH_EXTRA[k]
            w.field(0, 1)                                   # the one distance code: distance 1
    w.code(codes[256], lengths[256])
    w.field(0, 3)                                           # an empty stored block, not final
    w.align()
    return w.tobytes() + b"\x00\x00\xff\xff"


def encode_segment(data, table):
    """-> (the segment's bytes in the stream, whether it is the stored form)."""
    data = bytes(data)
    assert 1 <= len(data) <= 65535
    coded = coded_segment(data, table)
    if len(coded) > len(data) + 5:
        return b"\x00" + struct.pack("<HH", len(data), len(data) ^ 0xFFFF) + data, True
    return coded, False


def segment_ranges(H, row_bytes):
    r = rows_per_segment(H, row_bytes)
    return [(y * row_bytes, min(y + r, H) * row_bytes) for y in range(0, H, r)]


def zlib_stream(x, table, stored=None):
    """The zlib stream of picture x [H,W,C] uint8.  `stored`: a list that receives one flag per segment."""
    filtered, _ = filter_rows(x)
    H, row_bytes = filtered.shape
    flat = filtered.tobytes()
    out = b"\x78\x01"
    for lo, hi in segment_ranges(H, row_bytes):
        seg, st = encode_segment(flat[lo:hi], table)
        out += seg
        if stored is not None:
            stored.append(st)
    return out + b"\x03\x00" + struct.pack(">I", zlib.adler32(flat) & 0xFFFFFFFF)


def zlib_bound(W, H, C):
    row_bytes = W * C + 1
    return 2 + sum(hi - lo + 5 for lo, hi in segment_ranges(H, row_bytes)) + 6


def png_file(x, table):
    x = _as_image(x)
    H, W, C = x.shape

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, {1: 0, 2: 4, 3: 2, 4: 6}[C], 0, 0, 0)) + \
        chunk(b"IDAT", zlib_stream(x, table)) + chunk(b"IEND", b"")
