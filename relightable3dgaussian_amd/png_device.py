"""PNG frames encoded on the device (r3dg_png_encode, csrc/png_encode.hip): the scanline filter, the deflate stream and the
Adler-32 run in three launches; the host is left with a CRC-32 over the compressed bytes and a write().

The stream is ordinary zlib / deflate, cut so that every row segment is an independent unit of work (include/r3dg_hip.h
"r3dg_png_encode" states it in full): rows are filtered by the minimum sum of absolute differences, a segment of rows is parsed
into literals and distance-1 matches (runs of equal bytes; after filtering, flat regions are runs of zeros) and coded with ONE
dynamic-Huffman table that is chosen here, on the host, and handed to the kernel as data.  A segment that would come out larger
than its raw bytes is written as a stored block instead, which gives the stream a hard bound.

  CodeTable       the 286 literal/length code lengths -> canonical codes, the packed `code_table` (uint32[286]: bits 0..15 the code,
                  bit-reversed for LSB-first packing, bits 16..20 its length), the constant `block_header` bit string of a
                  non-final dynamic block (HLIT = 29, HDIST = 0, lengths written with code-length symbols 0..15 only) and
                  `header_bits`; validate() checks what the kernel relies on.
  DEFAULT_TABLE   a Huffman code over a Laplacian on the signed filter residual (generated below from its weights).
  FIXED_TABLE     deflate's fixed lengths (8 / 9 / 7 / 8, symbols 286 and 287 left out, 284 and 285 at 7 bits so that the code stays
                  complete) as a dynamic header: a cross-check.
  encode          device bytes [H,W,C] -> (zlib stream on the device, its length on the device); works on the current stream.
  wrap            zlib stream -> the PNG file (signature, IHDR, one IDAT, IEND), on the host.
"""
import heapq
import math
import struct
import zlib

SYMBOLS = 286                                  # literal/length symbols 0..285 (HLIT = 29)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
COLOR_TYPE = {1: 0, 2: 4, 3: 2, 4: 6}          # channels -> PNG colour type
SEGMENT_BYTES = 16384                          # rows_per_segment = max(1, min(H, SEGMENT_BYTES // row_bytes))
MAX_ROW_BYTES = 65535
MAX_HEADER_BITS = 2048


def _huffman_lengths(weights, limit):
    """Huffman code lengths of the symbols with weight > 0 (0 elsewhere), none above `limit`: when the plain Huffman tree is
    deeper, a floor that doubles each round is added to every used weight until it is not."""
    used = [i for i, w in enumerate(weights) if w > 0]
    if len(used) < 2:
        raise ValueError("a complete code needs at least two symbols")
    floor = 0.0
    while True:
        heap = [(weights[i] + floor, i, (i,)) for i in used]
        heapq.heapify(heap)
        lengths = [0] * len(weights)
        while len(heap) > 1:
            wa, ia, sa = heapq.heappop(heap)
            wb, ib, sb = heapq.heappop(heap)
            for s in sa + sb:
                lengths[s] += 1
            heapq.heappush(heap, (wa + wb, min(ia, ib), sa + sb))
        if max(lengths) <= limit:
            return lengths
        floor = max(weights) * 2.0 ** -24 if floor == 0.0 else floor * 2.0


def _canonical(lengths):
    """Canonical codes (RFC 1951 3.2.2) of `lengths`: MSB-first values, 0 for unused symbols."""
    count = [0] * (max(lengths) + 2)
    for n in lengths:
        count[n] += 1
    count[0] = 0
    code, nxt = 0, [0] * (max(lengths) + 2)
    for bits in range(1, max(lengths) + 1):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    codes = []
    for n in lengths:
        codes.append(nxt[n] if n else 0)
        nxt[n] += 1 if n else 0
    return codes


def _reverse(value, bits):
    return int(format(value, "0%db" % bits)[::-1], 2) if bits else 0


class CodeTable:
    """One dynamic-Huffman table for every segment and frame.  `lengths`: the 286 literal/length code lengths."""

    def __init__(self, lengths):
        self.lengths = tuple(int(n) for n in lengths)
        self.validate_lengths()
        self.codes = tuple(_canonical(self.lengths))
        self.code_table = tuple(_reverse(c, n) | n << 16 for c, n in zip(self.codes, self.lengths))
        # the code-length code over the 286 + 1 lengths (the one distance code has length 1), symbols 0..15 only
        written = self.lengths + (1,)
        freq = [0] * 19
        for n in written:
            freq[n] += 1
        self.cl_lengths = tuple(_huffman_lengths(freq, 7))
        cl_codes = _canonical(self.cl_lengths)
        hclen = max(i for i, s in enumerate(CL_ORDER) if self.cl_lengths[s]) + 1
        bits = []

        def put(value, n):                     # LSB-first field
            bits.extend((value >> i) & 1 for i in range(n))

        put(0, 1), put(2, 2), put(SYMBOLS - 257, 5), put(0, 5), put(hclen - 4, 4)
        for s in CL_ORDER[:hclen]:
            put(self.cl_lengths[s], 3)
        for n in written:
            put(_reverse(cl_codes[n], self.cl_lengths[n]), self.cl_lengths[n])
        self.header_bits = len(bits)
        bits += [0] * (-len(bits) % 8)
        self.block_header = bytes(sum(b << i for i, b in enumerate(bits[k:k + 8])) for k in range(0, len(bits), 8))
        self.validate()
        self._resident = {}                    # device -> (code_table, block_header) tensors

    def validate_lengths(self):
        if len(self.lengths) != SYMBOLS:
            raise ValueError("a code table has %d literal/length lengths, got %d" % (SYMBOLS, len(self.lengths)))
        if any(not 1 <= n <= 15 for n in self.lengths):
            raise ValueError("every literal/length symbol needs a code length in 1..15")
        if sum(1 << (15 - n) for n in self.lengths) != 1 << 15:
            raise ValueError("the literal/length code is not complete (Kraft sum != 1)")

    def validate(self):
        """What the kernel and the decoder rely on; raises ValueError."""
        self.validate_lengths()
        if sum(1 << (7 - n) for n in self.cl_lengths if n) != 1 << 7 or max(self.cl_lengths) > 7 or any(self.cl_lengths[16:]):
            raise ValueError("the code-length code is not a complete code over symbols 0..15")
        if not 17 <= self.header_bits <= MAX_HEADER_BITS:
            raise ValueError("block header of %d bits (17..%d are served)" % (self.header_bits, MAX_HEADER_BITS))
        for c, n, packed in zip(self.codes, self.lengths, self.code_table):
            if packed >> 16 != n or packed & 0xFFFF != _reverse(c, n):
                raise ValueError("code_table does not hold the canonical codes")
        return self

    def resident(self, device):
        """(code_table int32-viewed uint32 [286], block_header uint8) on `device`, uploaded once."""
        import torch
        key = str(device)
        if key not in self._resident:
            ct = torch.tensor([v - (1 << 32) if v >> 31 else v for v in self.code_table], dtype=torch.int32).to(device)
            bh = torch.tensor(list(self.block_header), dtype=torch.uint8).to(device)
            self._resident[key] = (ct, bh)
        return self._resident[key]


# ---- the tables -------------------------------------------------------------------------------------------------------------------
# literal v is the signed residual s (v, or v - 256 from 128 up): Laplacian of scale 6 over a floor; length symbol 257 + k falls
# off with k, 285 (length 258: the body of every long run) raised; end of block once per segment.
RESIDUAL_SCALE, LENGTH_WEIGHT, LENGTH_SCALE, WEIGHT_FLOOR, WEIGHT_258 = 6.0, 0.02, 8.0, 1e-3, 0.02


def default_weights():
    w = [math.exp(-min(v, 256 - v) / RESIDUAL_SCALE) + WEIGHT_FLOOR for v in range(256)]
    w.append(WEIGHT_FLOOR)
    w += [LENGTH_WEIGHT * math.exp(-k / LENGTH_SCALE) + WEIGHT_FLOOR for k in range(29)]
    w[285] = WEIGHT_258 + WEIGHT_FLOOR
    return w


DEFAULT_TABLE = CodeTable(_huffman_lengths(default_weights(), 15))
# deflate's fixed lengths without symbols 286 and 287 leave 2 / 256 of the code space unused, and inflate refuses an incomplete
# literal/length code: the last two length symbols (284, 285) take 7 bits instead of 8, which makes the Kraft sum exactly 1
FIXED_TABLE = CodeTable([8] * 144 + [9] * 112 + [7] * 24 + [8] * 4 + [7] * 2)


# ---- shapes -----------------------------------------------------------------------------------------------------------------------
def segments(W, H, C):
    """-> (row_bytes, rows_per_segment, number of segments)."""
    row_bytes = W * C + 1
    if not 1 <= C <= 4 or W < 1 or H < 1 or row_bytes > MAX_ROW_BYTES:
        raise RuntimeError("png: pictures are [H,W,C] with 1 <= C <= 4 and W * C + 1 <= %d, got %d x %d x %d"
                           % (MAX_ROW_BYTES, H, W, C))
    rows = max(1, min(H, SEGMENT_BYTES // row_bytes))
    return row_bytes, rows, -(-H // rows)


def zlib_bound(W, H, C):
    """r3dg_png_zlib_bound, restated: 2 + sum(raw_seg + 5) + 6."""
    row_bytes, _, n = segments(W, H, C)
    return 2 + H * row_bytes + 5 * n + 6


_scratch = {}                                  # (device, W, H, C) -> the encoder's scratch


def encode(bytes_dev, table=DEFAULT_TABLE, out=None):
    """r3dg_png_encode on the current stream: `bytes_dev` uint8 [H,W,C] on the device (contiguous; any alignment) ->
    (zlib_dev uint8 [bound], nbytes_dev int32 [1]), both on the device; nothing synchronises.  `out`: that pair, to be
    written in place (zlib_dev of at least the bound).  The scratch is kept per device and shape: encodes of one shape are ordered
    by their stream."""
    import torch
    from . import _lib
    if not isinstance(bytes_dev, torch.Tensor) or not bytes_dev.is_cuda or bytes_dev.dtype != torch.uint8 or \
            bytes_dev.dim() != 3 or not bytes_dev.is_contiguous():
        raise RuntimeError("png encode: the picture must be a contiguous uint8 [H,W,C] on the device (there is no CPU path)")
    H, W, C = (int(v) for v in bytes_dev.shape)
    bound = zlib_bound(W, H, C)
    dev = bytes_dev.device
    L = _lib.lib()
    if out is None:
        out = (torch.empty(bound, dtype=torch.uint8, device=dev), torch.empty(1, dtype=torch.int32, device=dev))
    zlib_dev, nbytes_dev = out
    if zlib_dev.dtype != torch.uint8 or zlib_dev.device != dev or not zlib_dev.is_contiguous() or \
            nbytes_dev.dtype != torch.int32 or nbytes_dev.device != dev or nbytes_dev.numel() != 1:
        raise RuntimeError("png encode: `out` is (uint8 [>= bound], int32 [1]) on the picture's device")
    key = (str(dev), W, H, C)
    scratch = _scratch.get(key)
    if scratch is None:
        scratch = _scratch[key] = torch.empty(int(L.r3dg_png_scratch_bytes(W, H, C)), dtype=torch.uint8, device=dev)
    code_table, block_header = table.resident(dev)
    with torch.cuda.device(dev):
        _lib.check(L.r3dg_png_encode(_lib.current_stream(), W, H, C, bytes_dev.data_ptr(), code_table.data_ptr(),
                                     block_header.data_ptr(), table.header_bits, scratch.data_ptr(), scratch.numel(),
                                     zlib_dev.data_ptr(), zlib_dev.numel(), nbytes_dev.data_ptr()), "png_encode")
    return zlib_dev, nbytes_dev


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def wrap(zlib_bytes, W, H, C):
    """The PNG file of a zlib stream of the filtered rows of a W x H picture of C 8-bit channels."""
    return b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, COLOR_TYPE[C], 0, 0, 0)) + \
        _chunk(b"IDAT", bytes(zlib_bytes)) + _chunk(b"IEND", b"")
