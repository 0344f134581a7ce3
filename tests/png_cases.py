"""The pictures both PNG test files encode ([H,W,C] uint8), by name.  They are the smallest shapes at which the encoder can still go
wrong: one pixel; a last segment shorter than the others; one row per segment; runs that cross 258 and 516 and a row boundary; a
segment that falls back to a stored block next to one that does not; and the longest row served (one segment of 65533 bytes: the
kernel's largest LDS footprint and widest chunks)."""
import numpy as np


def _rng(seed):
    return np.random.RandomState(seed)


def object_over_white(H=64, W=64):
    """A shaded disc with a little texture over a white background."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    r = np.hypot(y - H / 2, x - W / 2)
    shade = np.clip(1.0 - r / (0.4 * W), 0, 1)[..., None] * np.array([220.0, 150.0, 90.0])
    shade = shade + _rng(5).randint(0, 3, (H, W, 3))
    return np.where((r < 0.4 * W)[..., None], shade, 255.0).astype(np.uint8)


def noise_next_to_flat():
    x = np.full((17, 700, 3), 200, np.uint8)
    x[:7] = _rng(7).randint(0, 256, (7, 700, 3))
    return x


def long_runs():
    """3 x 600 x 3 zeros but for a few bytes: runs of 258 * k and around, and one over a row boundary."""
    x = np.zeros((3, 600, 3), np.uint8)
    x[0, 86, 0] = 9             # (type byte + 258 zeros in front)
    x[1, 173, 1] = 9
    return x


def flat_with_a_patch():
    """13 x 11 x 3, small and odd but flat enough to be coded rather than stored."""
    x = np.full((13, 11, 3), 200, np.uint8)
    x[4:9, 3:7] = _rng(1).randint(0, 256, (5, 4, 3)) // 64 * 64
    return x


CASES = {
    "1x1x1": lambda: np.array([[[77]]], np.uint8),
    "13x11x3": flat_with_a_patch,
    "17x5x1": lambda: (np.arange(85).reshape(17, 5, 1) * 3 % 256).astype(np.uint8),
    "33x29x4": lambda: np.repeat(_rng(2).randint(0, 256, (33, 8, 4)), 4, axis=1)[:, :29].astype(np.uint8),
    "9x7x2": lambda: _rng(3).randint(0, 4, (9, 7, 2)).astype(np.uint8) * 80,
    "3x600x3-zeros": lambda: np.zeros((3, 600, 3), np.uint8),
    "3x600x3-runs": long_runs,
    "17x700x3": lambda: (np.arange(17 * 700 * 3).reshape(17, 700, 3) // 9 % 256).astype(np.uint8),
    "17x700x3-noise-and-flat": noise_next_to_flat,
    "3x5462x3": lambda: np.repeat(_rng(4).randint(0, 256, (3, 43, 3)), 128, axis=1)[:, :5462].astype(np.uint8),
    "noise-37x50x3": lambda: _rng(6).randint(0, 256, (37, 50, 3)).astype(np.uint8),
    "object-64x64x3": object_over_white,
    "1x21844x3": lambda: np.repeat(_rng(8).randint(0, 256, (1, 172, 3)), 127, axis=1).astype(np.uint8),
}
NAMES = tuple(CASES)
_made = {}
_streams = {}


def picture(name):
    if name not in _made:
        _made[name] = CASES[name]()
        _made[name].setflags(write=False)
    return _made[name]


def reference_stream(name, table_name, table):
    """tests/png_reference.zlib_stream of a case, computed once per process: -> (stream, stored flag of every segment)."""
    from tests import png_reference as R
    key = (name, table_name)
    if key not in _streams:
        stored = []
        _streams[key] = (R.zlib_stream(picture(name), table, stored), stored)
    return _streams[key]
