"""The training contact sheet without a GPU (relightable3dgaussian_amd/training_vis.py, training.py --save_training_vis,
csrc/training_sheet.hip): the float64 restatement (tests/training_vis_reference.py) against the reference's own float32 output
(tests/golden/training_vis_reference.npz, made by tests/golden/make_training_vis_golden.py) under the acceptance rule of the GPU
tests, the index maps against torch's own resample, sheet_size, the committed colormap table, the parser, the argument checks of
r3dg_training_sheet and the kernel's code object."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import training_vis_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "training_vis_reference.npz")
PROTOTYPE = """int r3dg_training_sheet(void* stream, int width, int height, int layout, const float* d_render, const float* d_gt,
                        const float* d_opacity, const int32_t* d_n_contrib, const float* d_feature,
                        const float* d_pseudo_normal, const float* d_background, const float* d_env, int env_rows,
                        int out_width, int out_height, uint8_t* d_bytes);
"""


def _fixture(layout):
    z = np.load(GOLD)
    head = "l%d_" % layout
    return {k[len(head):]: z[k] for k in z.files if k.startswith(head) and k != head + "sheet"}, z[head + "sheet"], z


# ---- 1. the restatement and the rule ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
def test_the_restatement_reproduces_the_reference_sheet_under_the_acceptance_rule(layout):
    """The reference's own float32 bytes pass the rule at every byte: the rule rejects nothing the reference does.  And it is a
    rule: the same sheet with one byte of every panel moved by 2 is rejected at exactly those bytes."""
    m, sheet, z = _fixture(layout)
    H, W = m["opacity"].shape[1:]
    out_h, out_w = R.sheet_size(R.PANELS[layout], H, W)[:2]
    assert sheet.shape == (out_h, out_w, 3)
    ref = R.sheet_reference(layout, m, out_h, out_w, z["turbo"])
    ok, lines = R.accept(sheet, ref, z["turbo"])
    print("\n".join(lines))
    assert ok.all(), "\n".join(lines)
    assert set(np.unique(ref["panel"]).tolist()) == set(range(-1, R.PANELS[layout]))
    moved, where = sheet.copy(), []
    for k in range(-1, R.PANELS[layout]):
        y, x = np.argwhere(ref["panel"] == k)[7]
        moved[y, x, 1] = moved[y, x, 1] + 2 if moved[y, x, 1] < 128 else moved[y, x, 1] - 2
        where.append((y, x, 1))
    ok, _ = R.accept(moved, ref, z["turbo"])
    assert sorted(map(tuple, np.argwhere(~ok).tolist())) == sorted(where)


def test_the_fixture_holds_the_cases_the_kernel_can_get_wrong():
    m, _, _ = _fixture(1)
    ch = R.CHANNELS[1]
    seen, op = m["n_contrib"][0] > 0, m["opacity"][0]
    depth = np.where(seen, m["feature"][ch["depth"]] / np.maximum(op, 1e-5), 0)
    var = np.where(seen, m["feature"][ch["depth2"]] / np.maximum(op, 1e-5), 0) - depth * depth
    assert (~seen).any() and (op == 0).any() and ((op > 0) & (op < 1e-5)).any() and (op == 1).any()
    assert (depth[seen] == 0).any() and ((depth > 0) & (depth < 0.2)).any() and (depth > 13).any() and np.isnan(depth).any()
    assert (var < 0).any() and ((var > 0) & (var < 0.001)).any() and (var > 0.001).any()
    assert (m["feature"] < 0).any() and (m["render"] < 0).any() and (m["render"] > 1).any()
    assert tuple(m["background"]) == (1.0, 1.0, 1.0) and tuple(_fixture(0)[0]["background"]) == (0.0, 0.0, 0.0)


def test_depth_constants_are_the_reference_s_and_the_kernel_s():
    """NumPy's float32 values of visualize_depth's defaults: in the fixture (the reference's own lines), in the restatement, and
    as hexadecimal float literals in the kernel."""
    z = np.load(GOLD)
    assert z["c_far"].dtype == np.float32 and float(z["c_far"]) == float(R.C_FAR) and float(z["span"]) == float(R.SPAN)
    with open(os.path.join(ROOT, "relightable3dgaussian_amd", "csrc", "training_sheet.hip")) as fh:
        text = fh.read()
    c_far, span = re.search(r"c_far = (-?0x[0-9a-fp.+-]+)f, span = (0x[0-9a-fp.+-]+)f;", text).groups()
    assert float.fromhex(c_far) == float(R.C_FAR) and float.fromhex(span) == float(R.SPAN)
    assert 7e-7 < R.TOL_T < 8e-7 and R.TOL_T * 256 < 1


@pytest.mark.parametrize("out,inp", [(800, 32), (1350, 54), (800, 808), (29, 30), (800, 814), (37, 38), (800, 1606), (1599, 3210),
                                     (13, 4), (22, 8), (37, 16), (100, 32), (30, 8), (80, 16)])
def test_the_index_rule_is_torch_s(out, inp):
    src = torch.nn.functional.interpolate(torch.arange(inp, dtype=torch.float32).reshape(1, 1, 1, inp), (1, out))
    assert np.array_equal(src.reshape(-1).numpy().astype(np.int64), R.nearest_index(out, inp))


# ---- 2. sheet_size -------------------------------------------------------------------------------------------------------------------------
def test_sheet_size_is_the_reference_expression():
    """800 x 800 frames: 800 x 1599 in stage 1 (3210 / 2.0075 = 1599.003..., the double-precision division) and 800 x 800 in stage
    2.  Small frames are scaled UP to 800 rows.  (The 800 x 1550 / 800 x 800 pair belongs to a 13 x 13 frame, grid 32 x 62 and
    62 x 62; a 13-row, 11-column frame has grids of 32 x 54 and 62 x 54 and the expression gives 800 x 1350 and 800 x 696.)"""
    from relightable3dgaussian_amd.training_vis import sheet_size
    assert sheet_size(7, 800, 800) == (800, 1599, 1606, 3210)
    assert sheet_size(16, 800, 800) == (800, 800, 3210, 3210)
    assert sheet_size(7, 13, 13) == (800, 1550, 32, 62) and sheet_size(16, 13, 13) == (800, 800, 62, 62)
    assert sheet_size(7, 13, 11) == (800, 1350, 32, 54) and sheet_size(16, 13, 11) == (800, 696, 62, 54)
    assert sheet_size(7, 401, 5) == (800, 29, 808, 30) and sheet_size(16, 201, 7) == (800, 37, 814, 38)
    for panels in (7, 16):
        for H, W in ((800, 800), (13, 11), (401, 5), (201, 7), (37, 50), (30, 40), (11, 13), (1, 1), (1200, 1600)):
            rows = -(-panels // 4)
            gh, gw = rows * (H + 2) + 2, 4 * (W + 2) + 2
            scale = gh / 800
            assert sheet_size(panels, H, W) == (int(gh / scale), int(gw / scale), gh, gw) == R.sheet_size(panels, H, W)


# ---- 3. the colormap table -----------------------------------------------------------------------------------------------------------------
def test_the_committed_table_is_the_fixture_s():
    assert np.array_equal(R.turbo_table(), np.load(GOLD)["turbo"])


def test_the_committed_table_is_matplotlib_s():
    matplotlib = pytest.importorskip("matplotlib")
    colors = np.asarray(matplotlib.colormaps["turbo"].colors, np.float64)
    assert np.array_equal(R.turbo_table(), colors.astype(np.float32))
    # ... and the bin rule is matplotlib's own call on a float32 array (Colormap.__call__: x * N truncated, N -> N - 1)
    t = np.concatenate([np.linspace(0, 1, 1001), np.arange(257) / 256.0]).astype(np.float32)
    assert np.array_equal(matplotlib.colormaps["turbo"](t)[:, :3].astype(np.float32), R.turbo_table()[R.bin_of(t.astype(np.float64))])


# ---- 4. the driver's flags -----------------------------------------------------------------------------------------------------------------
def test_the_parser_takes_the_two_flags_with_the_reference_s_defaults():
    from relightable3dgaussian_amd.training import build_parser
    base = ["-s", "data", "-m", "out"]
    a = build_parser().parse_args(base)
    assert a.save_training_vis is False and a.save_training_vis_iteration == 1000            # arguments/__init__.py:67-68
    a = build_parser().parse_args(base + ["--save_training_vis"])
    assert a.save_training_vis is True and a.save_training_vis_iteration == 1000
    a = build_parser().parse_args(base + ["-t", "neilf", "--save_training_vis", "--save_training_vis_iteration", "200"])
    assert a.save_training_vis is True and a.save_training_vis_iteration == 200


# ---- 5. the C ABI --------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_and_the_library_checks_its_arguments():
    from relightable3dgaussian_amd import _abi, _lib
    with open(os.path.join(ROOT, "include", "r3dg_hip.h")) as fh:
        assert PROTOTYPE in fh.read()
    p, i = C.c_void_p, C.c_int
    assert _abi.prototypes["r3dg_training_sheet"] == (i, [p, i, i, i, p, p, p, p, p, p, p, p, i, i, i, p])
    L = _lib.lib()
    f = L.r3dg_training_sheet
    EINVAL = _abi.constants["R3DG_EINVAL"]
    # (nothing is launched: every call is refused; 16 is a 4-byte-aligned address, 17 is not)
    good = [None, 8, 8, 1, 16, 16, 16, 16, 16, 16, 16, 16, 4, 20, 20, 16]
    for at, value in ((3, 2), (3, -1), (1, 0), (2, -1), (13, 0), (14, 0), (4, None), (5, None), (6, None), (7, None), (8, None),
                      (9, None), (15, None), (10, None), (11, None), (12, 0), (12, 1 << 14), (15, 17), (15, 18)):
        bad = list(good)
        bad[at] = value
        assert f(*bad) == EINVAL, (at, value)
        assert b"training_sheet" in L.r3dg_last_error()
    for at in (10, 11):                     # the background and the texture are layout 1's: layout 0 takes NULL for them
        bad = list(good)
        bad[3], bad[at] = 0, None
        bad[6] = None                       # (still refused, for the opacity: nothing may be launched here)
        assert f(*bad) == EINVAL and b"null buffer" in L.r3dg_last_error()
    assert f(None, 1 << 16, 1 << 15, 0, *good[4:]) == EINVAL and b"too large" in L.r3dg_last_error()       # 2^31 frame pixels
    assert f(*good[:13], 1 << 16, 1 << 15, 16) == EINVAL and b"too large" in L.r3dg_last_error()           # 2^31 sheet pixels
    assert f(None, (1 << 29), 1, 0, *good[4:]) == EINVAL and b"too large" in L.r3dg_last_error()           # a grid side of 2^31


# ---- 6. the kernel's code object -----------------------------------------------------------------------------------------------------------
def test_the_kernel_uses_no_scratch_memory_and_shares_its_expressions(tmp_path):
    from relightable3dgaussian_amd import build as B, kernel_sources
    from tests.test_kernel_resources_cpu import _metadata
    csrc = os.path.join(ROOT, "relightable3dgaussian_amd", "csrc")
    read = lambda name: open(os.path.join(csrc, name)).read()
    # one definition of the quantisation and of the capture expressions, used by both kernels of each pair
    assert read("glue_math.hpp").count("quantize_byte(float x)") == 1
    assert "quantize_byte(" in read("scene_assembly.hip") and "quantize_byte(" in read("training_sheet.hip")
    assert "255.f" not in read("training_sheet.hip") and "255.f" not in read("scene_assembly.hip")
    for name in ("eval_capture.hip", "training_sheet.hip"):
        text = read(name)
        assert '#include "capture_math.hpp"' in text and "pbr_over_background(" in text and "__fdiv_rn(f" not in text
    assert kernel_sources.kernel_files()["training_sheet_kernel"] == "training_sheet.hip"
    assert "training_sheet.hip" not in B.EXTRA
    if not os.path.exists(B.HIPCC):
        pytest.skip("no hipcc")
    _, kernels = _metadata("training_sheet.hip", str(tmp_path))
    found = {k: v for k, v in kernels.items() if "training_sheet_kernel" in k}
    assert len(found) == 1, kernels
    assert all(scratch == 0 and 0 < vgprs <= 64 for scratch, vgprs in found.values()), found
