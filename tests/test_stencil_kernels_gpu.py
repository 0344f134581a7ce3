"""The image-stencil kernels of the training loss on their own, through the C ABI, against their float64 restatements
(tests/stencil_reference.py): the SSIM forward / backward / two-image launches (csrc/ssim.hip), the stage-2 edge-aware smoothness in
both formulations (csrc/smooth.hip: three passes, and streamed as one kernel in all seven term subsets) and the stage-1 depth
smoothness (csrc/supervision.hip).  No element left out, no outlier fraction.  Inputs: tests/stencil_cases.py; every output is a view
into a canary-filled buffer (Out of tests/test_glue_kernels_gpu.py, whose _refs / _check / _n_sum are used as they are).

TOLERANCE: the rule of tests/test_glue_kernels_gpu.py.  d = max |ref32 - ref64| / scale; every element within
max(2 d, n 2^-24) scale + 2^-126; exactly 0 where the reference is exactly 0; d < 1e-5 (asserted for every case on the CPU too,
tests/test_stencil_reference_cpu.py).  Each test prints d, n and the largest err / bound per output (the MI355X table:
profiles/r15_stencil_parity.txt).

n = float32 roundings on the kernel's longest path to the output, COUNTED from the kernel sources (never fitted); E(x) = 4 +
ceil(|x| log2 e) for __expf, srgb_pow = 8 and "the stencil's 8" as in tests/test_glue_kernels_gpu.py.
 SSIM (ssim.hip)
  window average    w x (1), (w x) x (1), 10 additions; the column pass: 1 product, 10 additions                    23, taken 24
  C1, C2            0.01f, 0.03f: a rounded factor twice and the product                                            3 each
  S                 the averages 24; A 2, B 3, C 4, D 6 (every operation: each is bounded by 2^-24 of an addend of the scale),
                    C D, the reciprocal, A B, its product with the reciprocal 4; the two constants 6               49, taken 50
  dS/dmu1           S's 50 + B - A, D - C, five products, the difference 8                                          58, taken 60
  dS/dE[x^2]        S's 50 + the division                                                                            51, taken 52
  dS/dE[xy]         no more than S's                                                                                 50
  backward          the window 24 (22 for a plain map), 2 x a1, y a2, two additions, * scale                        29, taken 30
  chained           the backward's own bound + its linear map over absolute values applied to the forward partials' bounds
  sum               _n_sum(50, 4 pixels per thread, workgroups)
 smoothness (smooth.hip; the two formulations share every expression)
  divided map       1 / opc, F * scale 2; sRGB: srgb_pow 8, * 1.055, - 0.055 -> 12; * m 1                          13 (roughness 3)
  Sobel of a map    the map's 13 + the stencil's 8                                                                   21 (normal 10, depth 9)
  e = exp(-|G gt|)  E(1) = 6 + the stencil's 8 -> 14; the guide normal's: 6 + 10 -> 16
  edge value        base w sign e 15; roughness (e0 + e1 + e2: 2) 17; light w sign g 17; guide -w |G dl| g sign: 21 + 16 + 3  40
  adjoint           per tap a product, an fma, an addition: the first tap's 2 + nine additions 11 -> base 26, roughness 28,
                    light 28, guide 51
  dL / d map        * m 1, * srgb' 1 with srgb' 12 (x 2 -> * 0.58 -> 2, srgb_pow 8, the constant and its product 2):
                    base 40, roughness 29, light 42, guide 51
  dL_dfeature       * scale 1 + scale's reciprocal 1: base 42 | roughness 31 | light 44 | normal 53 + the addition to the old value 54
  dL_dopacity       the largest active dL / d map + F dscale (a square, a division, two products) 4 + one accumulation per active
                    map (3 / 1 / 6) + the addition to the old value: 66 with all three terms
  sums              addend |G data| e + ...: 21 + 14 + 1 + 1 = 37 (base), 21 + 16 + 2 = 39 (roughness, light); three passes:
                    _n_sum(addend, 3 | 1 | 3, workgroups); streamed: 3 | 1 | 3 additions per row x rows per wave, one atomic per WAVE
 depth smoothness (supervision.hip)
  depth             the division 1; Sobel 9; e0 + e1 + e2 accumulated from 0: 14 + 3 = 17; edge sign * e 17; adjoint 17 + 11 = 28;
                    * w 29; dL_dfeature 3: * scale 2, + old 1 -> 32; dL_dopacity: * F * dscale 4, + old 1 -> 34; sum _n_sum(28, 1, .)"""

import numpy as np
import pytest
import torch

from tests import glue_reference as gr
from tests import stencil_cases as sc
from tests import stencil_reference as sr
from tests.helpers import report_elementwise
from tests.test_glue_kernels_gpu import CANARY, SLOTS, Out, _call, _check, _dev, _n_sum, _np, _p, _refs, _release_inputs, _slot_sum  # noqa: F401

pytestmark = pytest.mark.gpu
F64 = torch.float64

# ---- SSIM --------------------------------------------------------------------------------------------------------------------------
N_PARTIALS = np.array([60.0, 52.0, 50.0]).reshape(1, 3, 1, 1)
N_SSIM, N_SSIM_BWD = 50, 30


def _tiles(W, H):
    return ((W + 31) // 32) * ((H + 31) // 32)


def ssim_forward_refs(W, H, C, i):
    x = sc.ssim_case(W, H, C)
    return _refs(("ssim_f", W, H, C, i), sr.ssim_forward, x[i], x[2])


def ssim_backward_refs(W, H, C, i):
    """The backward ALONE: fed the reference's partials rounded to float32."""
    x = sc.ssim_case(W, H, C)
    p32 = ssim_forward_refs(W, H, C, i)[0]["partials"][0].float()
    return p32, _refs(("ssim_b", W, H, C, i), sr.ssim_backward, x[i], x[2], p32, scale=sc.ssim_scales(W, H, C)[i])


def _ssim_forward(W, H, C, x, y):
    part, total = Out(C, 3, H, W), Out(SLOTS, init=0.0)
    _call("r3dg_ssim_forward", W, H, C, _p(_dev(x)), _p(_dev(y)), part.ptr(), total.ptr())
    return part, total


@pytest.mark.parametrize("C", sc.SSIM_CHANNELS)
@pytest.mark.parametrize("W,H", sc.SSIM_SHAPES)
def test_ssim_forward(W, H, C):
    x = sc.ssim_case(W, H, C)
    for i in (0, 1):
        refs = ssim_forward_refs(W, H, C, i)
        part, total = _ssim_forward(W, H, C, x[i], x[2])
        tag = "ssim_forward x%d %dx%dx%d" % (i, W, H, C)
        _check(tag, "partials", part.cpu(), refs, N_PARTIALS)
        _check(tag, "sum", _slot_sum(total), refs, _n_sum(N_SSIM, 4, _tiles(W, H) * C))


@pytest.mark.parametrize("C", sc.SSIM_CHANNELS)
@pytest.mark.parametrize("W,H", sc.SSIM_SHAPES)
def test_ssim_backward(W, H, C):
    x = sc.ssim_case(W, H, C)
    for i in (0, 1):
        p32, refs = ssim_backward_refs(W, H, C, i)
        grad = Out(C, H, W)
        _call("r3dg_ssim_backward", W, H, C, _p(_dev(x[i])), _p(_dev(x[2])), _p(_dev(p32)), sc.ssim_scales(W, H, C)[i], grad.ptr())
        _check("ssim_backward x%d %dx%dx%d" % (i, W, H, C), "grad_x", grad.cpu(), refs, N_SSIM_BWD)


@pytest.mark.parametrize("C", sc.SSIM_CHANNELS)
@pytest.mark.parametrize("W,H", sc.SSIM_SHAPES)
def test_ssim_forward_then_backward(W, H, C):
    """The kernels chained, against autograd of the conv2d formulation (train_step.ssim) in float64.  Bound: the backward's own
    (on the reference partials) + |scale| (W*b0 + 2 |x| W*b1 + |y| W*b2), b = the forward partials' bounds."""
    x = sc.ssim_case(W, H, C)
    for i in (0, 1):
        scale = sc.ssim_scales(W, H, C)[i]
        fr = ssim_forward_refs(W, H, C, i)
        _, br = ssim_backward_refs(W, H, C, i)
        d_f, b_f = gr.tolerance(_np(fr[0]["partials"][0]), _np(fr[1]["partials"][0]), _np(fr[0]["partials"][1]), N_PARTIALS)
        d_b, b_b = gr.tolerance(_np(br[0]["grad_x"][0]), _np(br[1]["grad_x"][0]), _np(br[0]["grad_x"][1]), N_SSIM_BWD)
        x64, y64 = x[i].double(), x[2].double()
        bound = b_b + _np(sr.ssim_backward_abs(x64, y64, torch.from_numpy(b_f), scale))
        want = sr.ssim_value_and_grad(x64, y64)
        part, total = _ssim_forward(W, H, C, x[i], x[2])
        grad = Out(C, H, W)
        _call("r3dg_ssim_backward", W, H, C, _p(_dev(x[i])), _p(_dev(x[2])), part.ptr(), scale, grad.ptr())
        tag = "ssim chained x%d %dx%dx%d" % (i, W, H, C)
        ok, msg = report_elementwise(tag + " grad_x", _np(grad.cpu()), _np(want["grad"]) * scale, bound)
        print("%-34s %-13s d %.2e  n %4d  %s" % (tag, "grad_x", max(d_f, d_b), N_SSIM_BWD, msg.split("max err/bound", 1)[-1].strip()))
        assert max(d_f, d_b) < 1e-5 and ok, msg
        part.cpu()


@pytest.mark.parametrize("C", sc.SSIM_CHANNELS)
@pytest.mark.parametrize("W,H", sc.SSIM_SHAPES)
def test_ssim_pair_launches(W, H, C):
    """r3dg_ssim_forward_pair / _backward_pair with two images (x0 != x1, two scales): partials and gradients bit for bit those of
    the one-image launches, the sums within their n; and with image 1 absent: image 0 as before, image 1's buffers not touched."""
    x0, x1, y = sc.ssim_case(W, H, C)
    s0, s1 = sc.ssim_scales(W, H, C)
    d0, d1, dy = _dev(x0), _dev(x1), _dev(y)
    single = [_ssim_forward(W, H, C, x, y) for x in (x0, x1)]
    sgrad = []
    for x, (part, _), s in zip((d0, d1), single, (s0, s1)):
        sgrad.append(Out(C, H, W))
        _call("r3dg_ssim_backward", W, H, C, _p(x), _p(dy), part.ptr(), s, sgrad[-1].ptr())
    for two in (True, False):
        part = [Out(C, 3, H, W), Out(C, 3, H, W)]
        total = [Out(SLOTS, init=0.0), Out(SLOTS, init=0.0)]
        grad = [Out(C, H, W), Out(C, H, W)]
        _call("r3dg_ssim_forward_pair", W, H, C, _p(d0), _p(d1) if two else None, _p(dy), part[0].ptr(), part[1].ptr(), total[0].ptr(),
              total[1].ptr())
        _call("r3dg_ssim_backward_pair", W, H, C, _p(d0), _p(d1) if two else None, _p(dy), part[0].ptr(), part[1].ptr(), s0, s1,
              grad[0].ptr(), grad[1].ptr())
        tag = "ssim pair n=%d %dx%dx%d" % (1 + two, W, H, C)
        for i in ((0, 1) if two else (0,)):
            assert torch.equal(part[i].cpu(), single[i][0].cpu()), tag + ": partials of image %d" % i
            assert torch.equal(grad[i].cpu(), sgrad[i].cpu()), tag + ": gradient of image %d" % i
            _check(tag, "sum", _slot_sum(total[i]), ssim_forward_refs(W, H, C, i), _n_sum(N_SSIM, 4, _tiles(W, H) * C * (1 + two)))
        if not two:
            assert part[1].untouched() and grad[1].untouched() and float(_slot_sum(total[1])) == 0.0, tag


# ---- edge-aware smoothness ------------------------------------------------------------------------------------------------------------
PLANES = {"normal": slice(0, 3), "base": slice(3, 6), "rough": slice(6, 7), "light": slice(7, 10)}     # of dL_dfeature 5..14
N_PLANE = {"normal": 54, "base": 42, "rough": 31, "light": 44}
N_GMAP = {"base": 40, "rough": 29, "light": 51}                 # the largest dL / d map of a term (light: its guide's)
N_ADDEND = {"base": 37, "rough": 39, "light": 39}
ADDS = {"base": 3, "rough": 1, "light": 3}


def _n_dopacity(on):
    terms = [t for t in ("base", "rough", "light") if on[t]]
    return max(N_GMAP[t] for t in terms) + 4 + sum({"base": 3, "rough": 1, "light": 6}[t] for t in terms) + 1


def smooth_refs(W, H, subset, masked):
    c = sc.smooth_case(W, H)
    w = [a * b for a, b in zip(sc.smooth_weights(W, H), sc.SUBSETS[subset])]
    return _refs(("smooth", W, H, subset, masked), sr.stage2_smooth, W, H, c["opacity"], c["feature"], c["n_contrib"], c["gt"],
                 c["mask"] if masked else None, *w)


def smooth_expected(W, H, subset, masked, acc):
    """What the buffers hold after the call: (ref64, ref32) of {sum_*, dL_dopacity = old + term, normal = acc * old + term, base,
    rough, light}."""
    c = sc.smooth_case(W, H)
    out = []
    for r, dt in zip(smooth_refs(W, H, subset, masked), (F64, torch.float32)):
        old_o, old_n = c["old_dopacity"].to(dt), c["old_normal"].to(dt) * acc
        e = {k: v for k, v in r.items() if k.startswith("sum_")}
        e["dL_dopacity"] = (old_o + r["dL_dopacity"][0], old_o.abs() + r["dL_dopacity"][1])
        for k, s in PLANES.items():
            v, sv = r["dL_dfeature"][0][s], r["dL_dfeature"][1][s]
            e[k] = (old_n + v, old_n.abs() + sv) if k == "normal" else (v, sv)
        out.append(e)
    return tuple(out)


def _smooth_launch(W, H, fused, d, mask, w, acc, dop, gf, sums):
    args = (W, H, _p(d["opacity"]), _p(d["feature"]), _p(d["n_contrib"]))
    if fused:
        _call("r3dg_stage2_smooth_fused", *args, _p(d["gt"]), mask, *w, acc, dop.ptr(), gf.ptr(), sums.ptr())
        return None
    scratch = Out(30, W * H)
    _call("r3dg_stage2_smooth_forward", *args, _p(d["gt"]), mask, *w, scratch.ptr(), sums.ptr())
    _call("r3dg_stage2_smooth_backward", *args, mask, scratch.ptr(), *w, acc, dop.ptr(), gf.ptr())
    return scratch


def _run_smooth(W, H, fused, subset):
    c = sc.smooth_case(W, H)
    HW = W * H
    d = {k: _dev(c[k]) for k in ("opacity", "feature", "n_contrib", "gt", "mask")}
    on = dict(zip(("base", "rough", "light"), sc.SUBSETS[subset]))
    w = [a * b for a, b in zip(sc.smooth_weights(W, H), sc.SUBSETS[subset])]
    for masked, acc in ((True, 1), (False, 0), (True, 0)):
        exp = smooth_expected(W, H, subset, masked, acc)
        term = smooth_refs(W, H, subset, masked)[0]
        dop, gf, sums = Out(HW), Out(16, HW), Out(3 * SLOTS, init=0.0)
        dop.t.copy_(c["old_dopacity"])
        gf.t[5:8].copy_(c["old_normal"])
        scratch = _smooth_launch(W, H, fused, d, _p(d["mask"]) if masked else None, w, acc, dop, gf, sums)
        tag = "smooth %s %s m%d a%d %dx%d" % ("fused" if fused else "3pass", subset, masked, acc, W, H)
        got_o, got_f = dop.cpu(), gf.cpu()
        _check(tag, "dL_dopacity", got_o, exp, _n_dopacity(on))
        quiet = term["dL_dopacity"][0] == 0
        assert torch.equal(got_o[quiet], c["old_dopacity"][quiet]), tag + ": dL_dopacity moved where the term is exactly 0"
        for k, first in (("base", 8), ("rough", 11), ("light", 12)):
            rows = got_f[first:first + (1 if k == "rough" else 3)]
            if on[k]:
                _check(tag, k, rows, exp, N_PLANE[k])
            else:
                assert bool((rows == CANARY).all()), tag + ": a map of the absent %s term was written" % k
        if on["light"]:
            _check(tag, "normal", got_f[5:8], exp, N_PLANE["normal"])
            quiet = term["dL_dfeature"][0][0:3] == 0
            assert torch.equal(got_f[5:8][quiet], (c["old_normal"] * acc)[quiet]), tag + ": a normal map moved where the term is 0"
        else:
            assert torch.equal(got_f[5:8], c["old_normal"]), tag + ": the normal maps were touched without the light term"
        assert bool((got_f[0:5] == CANARY).all()) and bool((got_f[15] == CANARY).all()), tag + ": a map outside 5..14 was written"
        if fused:
            strips = (W + 59) // 60
            rows_w = max(1, min(min(32, max(8, (strips * H + 2047) // 2048)), H))
            waves = strips * ((H + rows_w - 1) // rows_w)
            per, blocks = rows_w, 4 * ((waves + 3) // 4)
        else:
            per, blocks = 1, (HW + 255) // 256
            scratch.cpu()
        for q, k in enumerate(("base", "rough", "light")):
            if on[k]:
                _check(tag, "sum_" + k, _slot_sum(sums, q), exp, _n_sum(N_ADDEND[k], ADDS[k] * per, blocks))
            else:
                assert float(_slot_sum(sums, q)) == 0.0, tag + ": the sum of the absent %s term moved" % k


@pytest.mark.parametrize("subset", list(sc.SUBSETS))
@pytest.mark.parametrize("W,H", sc.SMOOTH_SHAPES)
def test_stage2_smooth_fused(W, H, subset):
    _run_smooth(W, H, True, subset)


@pytest.mark.parametrize("subset", sc.THREE_PASS_SUBSETS)
@pytest.mark.parametrize("W,H", sc.SMOOTH_SHAPES)
def test_stage2_smooth_three_passes(W, H, subset):
    _run_smooth(W, H, False, subset)


# ---- stage-1 depth smoothness ---------------------------------------------------------------------------------------------------------
def depth_refs(W, H):
    c = sc.smooth_case(W, H)
    return _refs(("depth", W, H), sr.stage1_depth_smooth, W, H, c["opacity"], c["feat5"], c["n_contrib"], c["gt"], sc.depth_weight(W, H))


def depth_expected(W, H):
    c = sc.smooth_case(W, H)
    out = []
    for r, dt in zip(depth_refs(W, H), (F64, torch.float32)):
        old_o, old_f = c["old_dopacity"].to(dt), c["old_dfeat5"].to(dt)
        out.append({"sum_depth": r["sum_depth"], "dL_dopacity": (old_o + r["dL_dopacity"][0], old_o.abs() + r["dL_dopacity"][1]),
                    "dL_dfeature": (old_f[3] + r["dL_dfeature"][0][3], old_f[3].abs() + r["dL_dfeature"][1][3])})
    return tuple(out)


@pytest.mark.parametrize("W,H", sc.SMOOTH_SHAPES)
def test_stage1_depth_smooth(W, H):
    c = sc.smooth_case(W, H)
    HW = W * H
    exp, term = depth_expected(W, H), depth_refs(W, H)[0]
    dop, gf, total, edge = Out(HW), Out(5, HW), Out(SLOTS, init=0.0), Out(2, HW)
    dop.t.copy_(c["old_dopacity"])
    gf.t.copy_(c["old_dfeat5"])
    _call("r3dg_stage1_depth_smooth", W, H, _p(_dev(c["opacity"])), _p(_dev(c["feat5"])), _p(_dev(c["n_contrib"])), _p(_dev(c["gt"])),
          sc.depth_weight(W, H), edge.ptr(), dop.ptr(), gf.ptr(), total.ptr())
    tag = "s1_depth_smooth %dx%d" % (W, H)
    got_o, got_f = dop.cpu(), gf.cpu()
    _check(tag, "dL_dopacity", got_o, exp, 34)
    _check(tag, "dL_dfeature", got_f[3], exp, 32)
    keep = [0, 1, 2, 4]
    assert torch.equal(got_f[keep], c["old_dfeat5"][keep]), tag + ": a map other than the depth's was touched"
    quiet = term["dL_dfeature"][0][3] == 0
    assert torch.equal(got_f[3][quiet], c["old_dfeat5"][3][quiet]) and torch.equal(got_o[quiet], c["old_dopacity"][quiet]), tag
    _check(tag, "sum_depth", _slot_sum(total), exp, _n_sum(28, 1, (HW + 255) // 256))
    edge.cpu()
