"""The float64 restatements of the image-stencil kernels (tests/stencil_reference.py) and their inputs (tests/stencil_cases.py), on
the CPU.

1. Each restatement is pinned, in float64, to the function the whole-iteration tests are pinned to: SSIM to train_step.ssim (its
   own body, with the float32 window it builds widened by a patched conv2d: the eleven taps are the kernel's bit for bit, the 121
   products are rounded to float32 there and exact here, which is the 2e-7 of that pin; the conv2d formulation with exact products
   agrees to 1e-12), the smoothness terms to train_step.stage2_smoothness (value and autograd gradients; the sRGB curve with the
   float32 knee is tests/glue_reference.py's, pinned by tests/test_glue_reference_cpu.py), the depth smoothness to
   train_step.stage1_loss with only that weight -- both with the stencil written as differences (see exact_sobel).
2. Every decision quantity of every case is either bit-equal in float32 and float64 or at least four times further from its
   threshold than the bound the tolerance rule grants it: Sobel responses against 0, sRGB arguments against the knee, curves against
   the clip, opacities against 1e-5.
3. For each term the reference gradient is not 0 on every border side and in every corner of at least one case.
4. d = max |ref32 - ref64| / scale stays below 1e-5 for every case and output the GPU module runs; an SSIM reference that is
   exactly 0 at a positive scale is exactly 0 in float32 too (a structural zero -- the GPU module demands it of the kernel, and a 0
   that only exact arithmetic delivers, such as dS/dmu1 where two flat images agree at 1.0, would be a badly posed case)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from relightable3dgaussian_amd import train_step as ts
from tests import glue_cases as gc
from tests import glue_reference as gr
from tests import stencil_cases as sc
from tests import stencil_reference as sr
from tests import test_stencil_kernels_gpu as tk

F64 = torch.float64


def _close(name, got, want, rtol):
    got, want = np.asarray(got.detach(), np.float64), np.asarray(want.detach(), np.float64)
    err, scale = np.abs(got - want).max(), max(np.abs(want).max(), 1e-300)
    print("%-28s max|err| %.3e  scale %.3e" % (name, err, scale))
    assert err <= rtol * scale, (name, err, scale)


@pytest.fixture
def widened_conv(monkeypatch):
    """train_step.ssim builds its window as a float32 tensor: let its conv2d calls widen it to the image's dtype."""
    conv = F.conv2d
    monkeypatch.setattr(F, "conv2d", lambda x, w, *a, **k: conv(x, w.to(x.dtype), *a, **k))


@pytest.fixture
def exact_sobel(monkeypatch):
    """train_step.spatial_gradient is a float convolution: over a constant neighbourhood it returns 1e-17 with a sign where the
    stencil is 0, and autograd then sends a gradient through |.|.  The pins below run train_step's objectives with the stencil
    written as differences (glue_reference.sobel, pinned to spatial_gradient by tests/test_glue_reference_cpu.py)."""
    monkeypatch.setattr(ts, "spatial_gradient", lambda x: gr.sobel(x[0])[None])


def _above_the_clamp(opacity):
    """The case's opacities with the pixel AT float32(1e-5) moved to 2e-5: train_step clamps at the double 1e-5, which lies above it."""
    return torch.where(opacity == gr.OP_MIN, torch.full_like(opacity, 2e-5), opacity)


# ---- 1. the pins ---------------------------------------------------------------------------------------------------------------------
def test_ssim_window_is_train_steps_bit_for_bit():
    g = torch.tensor([math.exp(-(x - 5) ** 2 / (2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float32)
    assert [float(v) for v in g / g.sum()] == sr.SSIM_WIN
    assert sr.SSIM_WIN == sr.SSIM_WIN[::-1]                                # symmetric: the backward's premise


@pytest.mark.parametrize("W,H,C", [(7, 5, 1), (38, 27, 3), (65, 6, 3)])
def test_ssim_restatements_are_train_steps_ssim_in_float64(W, H, C, widened_conv):
    x, _, y = (t.double() for t in sc.ssim_case(W, H, C))
    xl = x.clone().requires_grad_(True)
    want = ts.ssim(xl, y) * (C * H * W)
    gwant, = torch.autograd.grad(want, [xl])
    fwd = sr.ssim_forward(x, y)
    # train_step rounds each of the 121 products g_i g_j to float32; the kernel's separable passes (and the restatements) use the
    # eleven taps themselves: 2^-24 per tap, relative, is the distance between the two windows
    _close("sum", fwd["sum"][0], want, 2e-7)
    _close("backward of the partials", sr.ssim_backward(x, y, fwd["partials"][0], 0.37)["grad_x"][0], 0.37 * gwant, 2e-6)
    vg = sr.ssim_value_and_grad(x, y)
    _close("value_and_grad sum", vg["sum"], fwd["sum"][0], 1e-12)
    _close("value_and_grad grad", 0.37 * vg["grad"], sr.ssim_backward(x, y, fwd["partials"][0], 0.37)["grad_x"][0], 1e-10)
    assert bool((fwd["partials"][1] >= fwd["partials"][0].abs()).all()) and bool((fwd["map"][1] >= fwd["map"][0].abs()).all())


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("W,H", [(2, 2), (7, 5), (61, 3), (121, 9)])
def test_smoothness_restatement_is_train_steps_in_float64(W, H, masked, exact_sobel):
    c = sc.smooth_case(W, H)
    n = 3.0 * W * H
    lam = dict(base_color_smooth=1.0, roughness_smooth=0.5, light_smooth=0.7)
    opacity, feature = c["opacity"].double().requires_grad_(True), c["feature"].double().requires_grad_(True)
    feat = (feature / opacity.clamp_min(gr.OP_MIN) * (c["n_contrib"] > 0)).reshape(16, H, W)       # (1e-5 as the kernels' float32)
    mapped = torch.cat([feat[:8], gr.rgb_to_srgb(feat[8:11]), feat[11:12], gr.rgb_to_srgb(feat[12:15]), feat[15:]], 0)
    mask = c["mask"].double().reshape(1, H, W) if masked else None
    loss = ts.stage2_smoothness(mapped, c["gt"].double().reshape(3, H, W), mask, lam, maps_are_srgb=True)
    go, gf = torch.autograd.grad(loss, [opacity, feature])
    got = sr.stage2_smooth(W, H, c["opacity"].double(), c["feature"].double(), c["n_contrib"], c["gt"].double(),
                           c["mask"].double() if masked else None, 1.0 / n, 0.5 / n, 0.7 / n)
    value = (got["sum_base"][0] + 0.5 * got["sum_rough"][0] + 0.7 * got["sum_light"][0]) / n
    _close("loss", value, loss, 1e-12)
    _close("dL_dopacity", got["dL_dopacity"][0], go, 1e-11)
    _close("dL_dfeature", got["dL_dfeature"][0], gf[5:15], 1e-11)
    assert float(gf[:5].abs().max()) == 0.0 and float(gf[15].abs().max()) == 0.0
    for k, (v, s) in got.items():
        assert bool((s >= 0).all()) and bool(((s > 0) | (v == 0)).all()), k + ": a non-zero value with a zero scale"


@pytest.mark.parametrize("W,H", [(1, 9), (7, 5), (60, 8)])
def test_depth_smoothness_restatement_is_train_steps_stage1_loss_in_float64(W, H, widened_conv, exact_sobel):
    c = dict(sc.smooth_case(W, H))
    c["opacity"] = _above_the_clamp(c["opacity"])
    w = dict(l1=0.0, mask_entropy=0.0, normal_render_depth=0.0, normal_smooth=0.0, depth_var=0.0, depth_smooth=0.4)
    opacity, feature = c["opacity"].double().requires_grad_(True), c["feat5"].double().requires_grad_(True)
    img = lambda t: t.reshape(-1, H, W)
    z3 = torch.zeros(3, H, W, dtype=F64)
    outs = (0, img(c["n_contrib"]), z3, img(opacity), None, img(feature), z3, None, None, None)
    loss = ts.stage1_loss(outs, img(c["gt"].double()), None, w, iteration=0)
    go, gf = torch.autograd.grad(loss, [opacity, feature])
    got = sr.stage1_depth_smooth(W, H, c["opacity"].double(), c["feat5"].double(), c["n_contrib"], c["gt"].double(), 0.4 / (3.0 * W * H))
    # (stage1_loss clamps at the double 1e-5, the restatement at its float32 value: 2.5e-8, relative, at the pixels below it)
    _close("loss", 0.4 * got["sum_depth"][0] / (3.0 * W * H), loss, 1e-7)
    _close("dL_dopacity", got["dL_dopacity"][0], go, 1e-7)
    _close("dL_dfeature", got["dL_dfeature"][0], gf, 1e-7)


# ---- 2. the cases' distance from every decision ----------------------------------------------------------------------------------------
N_SOBEL = {"base": 21, "rough": 21, "light": 21, "normal": 10, "depth": 9}          # the GPU module's table


@pytest.mark.parametrize("W,H", sc.SMOOTH_SHAPES)
def test_smoothness_cases_keep_clear_of_every_decision(W, H):
    c = sc.smooth_case(W, H)
    args = (W, H, c["opacity"], c["feature"], c["n_contrib"])
    assert not sc.smooth_offenders(*args, c["mask"], c["special"]).any()
    flips = 0
    for mk in (c["mask"], torch.ones_like(c["mask"])):
        m32, x32 = sc.smooth_decision_maps(*args, mk, torch.float32)
        m64, x64 = sc.smooth_decision_maps(*args, mk, F64)
        for k, n in N_SOBEL.items():
            g32, g64 = gr.sobel(m32[k]).double(), gr.sobel(m64[k])
            s = gr._sobel_abs(m64[k].abs()[None])[0]
            d = float(((g32 - g64).abs() / s.clamp_min(1e-300)).max())
            grant = max(2.0 * d, n * gr.U32) * s                              # what the tolerance rule grants the response
            assert bool(((g32 == g64) | (g64.abs() >= 4.0 * grant)).all()), (k, W, H)
            flips += int((torch.sign(g32) != torch.sign(g64)).sum())
        # the sRGB arguments: bit-equal (opacity a power of two) or clear of the knee; the curve clear of the clip -- except at the
        # crafted pixels, which sit ON the thresholds by construction and must decide alike in both precisions
        same = x32.double() == x64
        assert bool((same | ~gc.near(x64, (gr.KNEE,), 4.0 * 2 * x64.abs())).all())
        c32, c64 = gr.srgb_curve(x32), gr.srgb_curve(x64)
        free = ~c["special"]
        sc64 = torch.where(x64 > gr.KNEE, 1.055 * torch.pow(x64.clamp_min(gr.KNEE), 1.0 / 2.4) + 0.055, 12.92 * x64.abs())
        assert bool(((c64 - 1.0).abs() >= 4.0 * 12 * gr.U32 * sc64)[:, free].all()) and bool((c64.abs() >= 4.0 * 12 * gr.U32 * sc64)[:, free].all())
        for lo, hi in ((0.0, 0.0), (1.0, 1.0)):
            assert bool(((c32 < lo) == (c64 < lo)).all()) and bool(((c32 > hi) == (c64 > hi)).all())
        assert bool(((x32 > gr.KNEE) == (x64 > gr.KNEE)).all())
    assert flips == 0
    # opacities are inputs: the same float in both precisions, on both sides of 1e-5 and on it
    op = c["opacity"]
    if W * H >= 9:
        assert bool((op == gr.OP_MIN).any()) and bool((op == gc.step32(gr.OP_MIN, 1)).any()) and bool((op < gr.OP_MIN).any())
    pow2 = torch.frexp(op)[0] == 0.5
    assert bool((pow2 | c["special"]).all())


def test_smoothness_cases_hold_what_their_docstring_says():
    c = sc.smooth_case(121, 9)
    x = gr.divided(c["opacity"], c["feature"], c["n_contrib"])[0]
    for rows in (slice(8, 11), slice(12, 15)):
        v = x[rows]
        assert bool((v < 0).any()) and bool((v > 1.0).any()) and bool((v == gr.KNEE).any()) and bool((v == gc.step32(gr.KNEE, 1)).any())
        assert bool((v == gc.step32(gr.KNEE, -1)).any()) and bool((v == gc.clip_hi()).any())
    m = c["mask"]
    assert bool((m == 0).any()) and bool((m == 1).any()) and bool(((m > 0) & (m < 1)).any())
    nc = c["n_contrib"].reshape(9, 121)
    assert int((nc == 0).sum()) >= 5 and bool((nc[[0, -1]] > 0).all()) and bool((nc[:, [0, -1]] > 0).all())
    assert int(c["block"].sum()) == 25


# ---- 3. every border side and corner carries a gradient in some case ---------------------------------------------------------------------
def test_reference_gradients_reach_every_border_and_corner():
    seen = {}
    for W, H in sc.SMOOTH_SHAPES:
        if W < 3 or H < 3:
            continue
        for masked in (False, True):
            r = tk.smooth_refs(W, H, "all", masked)[0]
            maps = {k: r["dL_dfeature"][0][s].reshape(-1, H, W) for k, s in tk.PLANES.items()}
            maps["opacity"] = r["dL_dopacity"][0].reshape(1, H, W)
            maps["depth"] = tk.depth_refs(W, H)[0]["dL_dfeature"][0][3].reshape(1, H, W)
            for k, g in maps.items():
                nz = (g != 0).any(0)
                where = dict(top=nz[0, 1:-1].any(), bottom=nz[-1, 1:-1].any(), left=nz[1:-1, 0].any(), right=nz[1:-1, -1].any(),
                             tl=nz[0, 0], tr=nz[0, -1], bl=nz[-1, 0], br=nz[-1, -1])
                for p, hit in where.items():
                    seen[(k, p)] = seen.get((k, p), False) or bool(hit)
    missing = [k for k, v in seen.items() if not v]
    assert len(seen) == 6 * 8 and not missing, missing


# ---- 4. conditioning of every case the GPU module runs -------------------------------------------------------------------------------------
def _conditioned(tag, refs, names=None, structural_zeros=False):
    for k in (names or refs[0]):
        r64, s = (np.asarray(a, np.float64) for a in refs[0][k])
        r32 = np.asarray(refs[1][k][0], np.float64)
        d, _ = gr.tolerance(r64, r32, s, 1)
        assert d < 1e-5, "%s %s: d = %.3e" % (tag, k, d)
        assert not (structural_zeros and ((r64 == 0) & (s > 0) & (r32 != 0)).any()), "%s %s: a zero of the reference that float32 does not deliver" % (tag, k)


@pytest.mark.parametrize("C", sc.SSIM_CHANNELS)
@pytest.mark.parametrize("W,H", sc.SSIM_SHAPES)
def test_ssim_cases_are_well_conditioned(W, H, C):
    x0, x1, y = sc.ssim_case(W, H, C)
    assert not torch.equal(x0, x1) and sc.ssim_scales(W, H, C)[0] != sc.ssim_scales(W, H, C)[1]
    assert float(min(x0.min(), y.min())) < 0.0 and float(max(x0.max(), y.max())) > 1.0 or W * H < 30
    for i in (0, 1):
        _conditioned("ssim forward %dx%dx%d" % (W, H, C), tk.ssim_forward_refs(W, H, C, i), ("partials", "sum"), True)
        _conditioned("ssim backward %dx%dx%d" % (W, H, C), tk.ssim_backward_refs(W, H, C, i)[1], None, True)
    blocks = sc.ssim_blocks(W, H)
    if blocks:
        # the flat regions are there: D = C2 exactly where all three images are 0, D within 1e-5 of C2 in the white block
        t = [sr.window(v) for v in (x0.double(), y.double(), x0.double() ** 2, y.double() ** 2)]
        D = (t[2] - t[0] ** 2) + (t[3] - t[1] ** 2) + sr.SSIM_C2
        assert int((D == sr.SSIM_C2).sum()) >= C and int(((D - sr.SSIM_C2).abs() < 1e-12).sum()) >= 2 * C


@pytest.mark.parametrize("W,H", sc.SMOOTH_SHAPES)
def test_smoothness_cases_are_well_conditioned(W, H):
    for subset in sc.SUBSETS:
        for masked, acc in ((True, 1), (False, 0), (True, 0)):
            _conditioned("smooth %s m%d a%d %dx%d" % (subset, masked, acc, W, H), tk.smooth_expected(W, H, subset, masked, acc))
    _conditioned("depth %dx%d" % (W, H), tk.depth_expected(W, H))
    if W >= 7 and H >= 5:
        # the constant block: the term is exactly 0 in its middle
        r = tk.smooth_refs(W, H, "all", True)[0]
        mid = (torch.nn.functional.max_pool2d(-c_block(W, H), 5, 1, 2) == -1.0)[0]
        assert int(mid.sum()) >= 1
        assert float(r["dL_dfeature"][0][:, mid.reshape(-1)].abs().max()) == 0.0 and float(r["dL_dopacity"][0][mid.reshape(-1)].abs().max()) == 0.0


def c_block(W, H):
    return sc.smooth_case(W, H)["block"].float()[None]
