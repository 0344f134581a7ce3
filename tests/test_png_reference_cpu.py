"""The device PNG encoder's format on the CPU: tests/png_reference.py (the plain-loop restatement the device is held to, byte for
byte) decodes through zlib and PIL to its input for both tables of relightable3dgaussian_amd/png_device.py, the parse rule is met
literally, the stored fallback gives the derived bound, and the filter choice covers every type."""
import io
import zlib

import numpy as np
import pytest

from tests import png_cases
from tests import png_reference as R

MODES = {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}


def _tables():
    from relightable3dgaussian_amd import png_device
    return {"default": png_device.DEFAULT_TABLE, "fixed": png_device.FIXED_TABLE}


def test_tables_validate():
    from relightable3dgaussian_amd import png_device
    for t in _tables().values():
        assert t.validate() is t
        assert len(t.code_table) == 286 and 17 <= t.header_bits <= 2048 and len(t.block_header) == (t.header_bits + 7) // 8
        assert R.canonical_codes(list(t.lengths)) == list(t.codes)
        w = R._Bits()
        R.write_header(w, t)
        assert len(w.bits) == t.header_bits
        w.align()
        assert w.tobytes() == t.block_header
    # (the fixed lengths; 286 and 287 are left out, so 284 and 285 take 7 bits: the Kraft sum stays 1, as inflate demands)
    assert png_device.FIXED_TABLE.lengths == (8,) * 144 + (9,) * 112 + (7,) * 24 + (8,) * 4 + (7,) * 2
    d = png_device.DEFAULT_TABLE.lengths
    assert d[0] == min(d) and d[1] == d[255] and d[128] == max(d[:256]) and d[285] < d[284]


def test_bad_tables_raise():
    from relightable3dgaussian_amd import png_device
    good = list(png_device.FIXED_TABLE.lengths)
    zero = list(good)
    zero[7] = 0
    sixteen = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 6
    sixteen[200], sixteen[201] = 16, 16
    kraft = list(good)
    kraft[0] = 9
    for bad in (zero, sixteen, kraft, good[:-1]):
        with pytest.raises(ValueError):
            png_device.CodeTable(bad)


@pytest.mark.parametrize("table", ["default", "fixed"])
@pytest.mark.parametrize("name", png_cases.NAMES)
def test_round_trip(name, table):
    from PIL import Image
    x = png_cases.picture(name)
    H, W, C = x.shape
    t = _tables()[table]
    stream, stored = png_cases.reference_stream(name, table, t)
    filtered, _ = R.filter_rows(x)
    assert zlib.decompress(stream) == filtered.tobytes()
    assert len(stream) <= R.zlib_bound(W, H, C) == 2 + sum(hi - lo + 5 for lo, hi in R.segment_ranges(H, W * C + 1)) + 6
    from relightable3dgaussian_amd import png_device
    assert png_device.zlib_bound(W, H, C) == R.zlib_bound(W, H, C)
    assert len(stored) == png_device.segments(W, H, C)[2]
    with Image.open(io.BytesIO(R.png_file(x, t))) as im:
        assert im.mode == MODES[C] and im.size == (W, H)
        assert np.array_equal(np.asarray(im).reshape(H, W, C), x)
    assert png_device.wrap(stream, W, H, C) == R.png_file(x, t)


def test_segment_shapes_of_the_cases():
    assert [hi - lo for lo, hi in R.segment_ranges(17, 2101)] == [7 * 2101, 7 * 2101, 3 * 2101]
    assert [hi - lo for lo, hi in R.segment_ranges(3, 16387)] == [16387] * 3
    assert R.segment_ranges(1, 2) == [(0, 2)] and len(R.segment_ranges(1, 65533)) == 1
    _, stored = png_cases.reference_stream("17x700x3-noise-and-flat", "default", _tables()["default"])
    assert stored == [True, False, False]


@pytest.mark.parametrize("n", [1, 2, 3, 4, 258, 259, 260, 261, 262, 263, 517, 519, 520, 777])
def test_parse_of_a_run(n):
    tokens = R.parse(bytes([5]) * n)
    assert tokens[0] == ("lit", 5)
    assert sum(1 if t[0] == "lit" else t[1] for t in tokens) == n
    assert all(3 <= t[1] <= 258 for t in tokens if t[0] == "match")
    # the rule, literally
    want, rest = [("lit", 5)], n - 1
    while rest >= 261 or rest == 258:
        want.append(("match", 258))
        rest -= 258
    if rest in (259, 260):
        want += [("match", rest - 3), ("match", 3)]
    elif rest >= 3:
        want.append(("match", rest))
    else:
        want += [("lit", 5)] * rest
    assert tokens == want
    # a neighbouring run does not change it
    assert R.parse(bytes([5]) * n + bytes([6])) == want + [("lit", 6)]


@pytest.mark.parametrize("table", ["default", "fixed"])
def test_noise_is_stored_at_exactly_the_bound(table):
    x = png_cases.picture("noise-37x50x3")
    stream, stored = png_cases.reference_stream("noise-37x50x3", table, _tables()[table])
    assert stored and all(stored)
    assert len(stream) == 2 + sum(hi - lo + 5 for lo, hi in R.segment_ranges(37, 151)) + 6 == R.zlib_bound(50, 37, 3)
    assert zlib.decompress(stream) == R.filter_rows(x)[0].tobytes()


def test_every_filter_type_is_chosen_and_ties_go_low():
    W = 32
    x = np.zeros((5, W, 1), np.uint8)
    x[0, :, 0] = np.where(np.arange(W) % 2 == 0, 2, 254)       # None: every byte costs 2; Sub / Paeth / Average cost far more
    x[1, :, 0] = (np.arange(W) * 7 + 3) % 256                  # a ramp that is new to the row above: Sub costs 7 a byte
    x[2, :, 0] = x[1, :, 0]                                    # a copy of the row above: Up is all zeros
    x[2, 0, 0] ^= 1                                            # (not Paeth at no cost: the first byte differs, Up and Paeth tie -> Up)
    up = x[2, :, 0].astype(int)
    row = np.zeros(W, int)                                     # Average exact: v = floor((left + up) / 2) + small
    for i in range(W):
        row[i] = (((row[i - 1] if i else 0) + up[i]) // 2) % 256
    x[3, :, 0] = row
    a3 = x[3, :, 0].astype(int)                                # Paeth: a row that follows its predictor but for a few steps
    row, g = np.zeros(W, int), np.random.RandomState(0)
    for i in range(W):
        a, c = (row[i - 1], a3[i - 1]) if i else (0, 0)
        row[i] = (R.paeth(a, a3[i], c) + (g.randint(-1, 2) if i % 5 == 0 else 0) + (40 if i == 10 else 0)) % 256
    x[4, :, 0] = row
    _, types = R.filter_rows(x)
    assert types[0] == 0 and types[1] == 1 and types[2] == 2
    assert set(types) == {0, 1, 2, 3, 4}, types
    # ties: a constant picture of zeros scores 0 under every type -> None; a copy row scores 0 under Up and Paeth -> Up
    assert R.filter_rows(np.zeros((3, 4, 3), np.uint8))[1] == [0, 0, 0]
    flat = np.full((2, 8, 1), 9, np.uint8)
    assert R.filter_rows(flat)[1][1] == 2                      # Up, Paeth (and nothing lower) score 0 on the second row
