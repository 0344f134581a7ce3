"""The fused stage-2 image tail (r3dg_stage2_image_tail, csrc/image_tail.hip) on its own, through the C ABI, against the float64
composition of the restatements that exist (tests/image_tail_cases.tail_reference: stage2_pbr_srgb -> ssim_forward -> ssim_backward
on both images -> stage2_loss with the SSIM gradients as its extras), and a whole iteration with the tail on and off.  No element
left out, no outlier fraction; the inputs (tests/image_tail_cases.py) are checked on the CPU by tests/test_image_tail_cases_cpu.py.
Every output is a view into a canary-filled buffer (Out, _check, _refs, _n_sum of tests/test_glue_kernels_gpu.py as they are).

TOLERANCE: the rule of tests/test_glue_kernels_gpu.py and tests/test_stencil_kernels_gpu.py.  d = max |ref32 - ref64| / scale (the
whole composition in float32 against the same in float64: it carries how the earlier stages' roundings propagate); every element
within max(2 d, n 2^-24) scale + 2^-126; exactly 0 where the reference is exactly 0; d < 1e-5.  Each test prints the case, d, n and
the largest err / bound per output (the MI355X table: profiles/r16_image_tail.txt).

n = float32 roundings on the kernel's longest path to the output, COUNTED from the sources with the two modules' own counts (never
fitted): srgb 13, the window average 24, dS/dmu1 60, dS/dE[x^2] 52, dS/dE[xy] 50, S 50, the SSIM backward 30, dL_dimage's own 2,
dL_dfeature 2..4's own 20, 5..7's 10, dL_dopacity's 32.
  SSIM gradient of the SH image      its partials' 60 carried through the backward's linear map (ssim_backward_abs over the partials'
                                     scales is this output's scale) + the backward's own 30                                      90
  SSIM gradient of the PBR image     x is the sRGB value, 13 roundings of its own: every window average of x inherits them, E[x^2]
                                     twice -> the partials' 60 + 26; + the backward's 30; + 13 for the x in 2 x W*p1            129
  dL_dimage                          w sign + extra: 2 + 90                                                                      92
  dL_dfeature 2..4                   its own 20 with the extra's 129                                                            149
  dL_dfeature 5..7                   as r3dg_stage2_loss                                                                          10
  dL_dopacity                        its own 32 with the extra's 129                                                            161
  sums (one atomic per workgroup per sum, slot = linear workgroup index mod 32 of a grid of 4 x tiles workgroups)
                                     _n_sum(addend, additions per thread, 4 x tiles): L1 addend 2, 4 pixels per thread; PBR L1
                                     addend 14, normal 10, 3 channels x 4 pixels; SSIM of the SH image: addend 50, the 7 pixels of
                                     a column-pass item; of the PBR image: addend 50 + 26, 3 x 7
pseudo_normal and surface_xyz are not bounded but EQUAL to r3dg_stage2_normals_srgb's (the same device function on the same inputs);
the reference's normal term reads those values."""
import os

import numpy as np
import pytest
import torch

from tests import glue_reference as gr
from tests import image_tail_cases as tc
from tests import stencil_cases as sc
from tests.test_glue_kernels_gpu import CANARY, DEV, SLOTS, Out, _call, _check, _dev, _n_sum, _np, _p, _refs, _release_inputs, _slot_sum  # noqa: F401

pytestmark = pytest.mark.gpu

N_GRAD_IMAGE, N_GRAD_PBR = 60 + 30, 60 + 26 + 30 + 13
N_DIMAGE, N_DOPACITY = 2 + N_GRAD_IMAGE, 32 + N_GRAD_PBR
N_DFEATURE = np.zeros((16, 1))
N_DFEATURE[2:5], N_DFEATURE[5:8] = 20 + N_GRAD_PBR, 10
VARIANTS = {"no_normal_term": (False, False), "normal_term": (True, False), "normal_term_masked": (True, True)}


def _tiles(W, H):
    return ((W + tc.TILE - 1) // tc.TILE) * ((H + tc.TILE - 1) // tc.TILE)


def _launch_tail(c, d, W, H, feature, mask, w, scales):
    """-> (pseudo_normal, surface_xyz, dL_dimage, dL_dopacity, dL_dfeature, sums 0..2, SSIM sum of the image, of the PBR image)."""
    HW = W * H
    outs = Out(3, HW), Out(3, HW), Out(3, HW), Out(HW), Out(16, HW), Out(3 * SLOTS, init=0.0), Out(SLOTS, init=0.0), Out(SLOTS, init=0.0)
    outs[4].t[0:2] = float("nan")             # sentinels in the maps the kernel must not write (5..7: see the variant)
    outs[4].t[5:16] = float("nan")
    _call("r3dg_stage2_image_tail", W, H, _p(d["viewmatrix"]), tc.TAN_FOVX, tc.TAN_FOVY, c["cx"], c["cy"], _p(d["image"]),
          _p(d["opacity"]), _p(d["depth"]), _p(feature), _p(d["n_contrib"]), _p(d["gt"]), _p(d["bg"]), _p(mask), w[0], w[1], w[2],
          scales[0], scales[1], *(o.ptr() for o in outs))
    return outs


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("W,H", tc.SHAPES)
def test_image_tail(W, H, variant):
    normal_on, masked = VARIANTS[variant]
    c = tc.tail_case(W, H)
    HW = W * H
    d = {k: _dev(c[k]) for k in ("viewmatrix", "image", "opacity", "depth", "feature", "n_contrib", "gt", "bg", "mask")}
    w = list(tc.weights(W, H))
    if not normal_on:
        w[2] = 0.0
    scales = sc.ssim_scales(W, H, 3)                                  # two different scales of opposite sign
    feature = d["feature"]
    if not normal_on:                                                 # the normal maps are not read: NaN must not reach an output
        feature = _dev(c["feature"].clone())
        feature[5:8] = float("nan")
    # the four-launch path's pseudo normals, on the same inputs
    pn0, sx0, srgb0 = Out(3, HW), Out(3, HW), Out(3, HW)
    _call("r3dg_stage2_normals_srgb", W, H, _p(d["viewmatrix"]), tc.TAN_FOVX, tc.TAN_FOVY, c["cx"], c["cy"], _p(d["opacity"]),
          _p(d["depth"]), pn0.ptr(), sx0.ptr(), _p(d["feature"]), _p(d["n_contrib"]), _p(d["bg"]), srgb0.ptr())
    pn, sx, gi, go, gf, sums, ssim_i, ssim_p = _launch_tail(c, d, W, H, feature, d["mask"] if masked else None, w, scales)
    tag = "image_tail %s %dx%d" % (variant, W, H)
    pseudo = pn0.cpu().clone()
    assert torch.equal(pn.cpu(), pseudo), tag + ": pseudo normals differ from r3dg_stage2_normals_srgb's"
    assert torch.equal(sx.cpu(), sx0.cpu()), tag + ": surface points differ from r3dg_stage2_normals_srgb's"
    refs = _refs(("tail", W, H, variant), tc.tail_reference, W, H, c["image"], c["opacity"], c["feature"], pseudo, c["n_contrib"],
                 c["gt"], c["bg"], c["mask"] if masked else None, w[0], w[1], w[2], scales[0], scales[1])
    _check(tag, "dL_dimage", gi.cpu(), refs, N_DIMAGE)
    _check(tag, "dL_dopacity", go.cpu(), refs, N_DOPACITY)
    written = [2, 3, 4] + ([5, 6, 7] if normal_on else [])
    got_f = gf.cpu()
    assert bool(torch.isfinite(got_f[written]).all()) and bool(torch.isfinite(gi.cpu()).all()) and bool(torch.isfinite(go.cpu()).all()), tag
    _check(tag, "dL_dfeature", got_f[written], refs, N_DFEATURE[written], index=written)
    rest = [k for k in range(16) if k not in written]
    assert bool(torch.isnan(got_f[rest]).all()), tag + ": a feature-gradient map outside the sparse set was written"
    blocks = 4 * _tiles(W, H)
    _check(tag, "sum_l1", _slot_sum(sums, 0), refs, _n_sum(2, 4, blocks))
    _check(tag, "sum_pbr", _slot_sum(sums, 1), refs, _n_sum(14, 12, blocks))
    if normal_on:
        _check(tag, "sum_normal", _slot_sum(sums, 2), refs, _n_sum(10, 12, blocks))
    else:
        assert "sum_normal" not in refs[0] and float(_slot_sum(sums, 2)) == 0.0
    _check(tag, "ssim_image", _slot_sum(ssim_i), refs, _n_sum(50, 7, blocks))
    _check(tag, "ssim_pbr", _slot_sum(ssim_p), refs, _n_sum(50 + 26, 21, blocks))


def test_capability_and_argument_checks():
    from relightable3dgaussian_amd import _lib
    L = _lib.lib()
    assert L.r3dg_stage2_image_tail_supported(800, 800) == 1 and L.r3dg_stage2_image_tail_supported(1, 1) == 1
    assert L.r3dg_stage2_image_tail_supported(0, 5) == 0 and L.r3dg_stage2_image_tail_supported(65536, 65536) == 0
    cam, w = (0.5, 0.5, 0.0, 0.0), (0.0,) * 5
    # (no call below reaches a launch: an empty image is nothing to do; the checks come before the first access)
    assert L.r3dg_stage2_image_tail(None, 0, 8, None, *cam, *[None] * 8, *w, *[None] * 8) == 0
    assert L.r3dg_stage2_image_tail(None, 8, 8, None, *cam, *[1] * 7, None, *w, *[1] * 8) != 0          # no view matrix
    assert L.r3dg_stage2_image_tail(None, 8, 8, 1, *cam, *[1] * 7, None, *w, *[1] * 7, None) != 0       # no SSIM sum
    assert L.r3dg_stage2_image_tail(None, -1, 8, 1, *cam, *[1] * 7, None, *w, *[1] * 8) != 0


# ---- a whole iteration with the tail on and off -------------------------------------------------------------------------------------
def _iteration(tail_on):
    """One forward_backward of a small supervised-free stage-2 step (70 x 45: partial tiles on both axes) -> (loss, slab planes
    0..19, pseudo normals, surface points)."""
    from relightable3dgaussian_amd import synthetic as syn
    from relightable3dgaussian_amd.bench_core import GaussianParams, render_stage1
    from relightable3dgaussian_amd.fused_step import FusedStage2Step
    old = os.environ.get("R3DG_IMAGE_TAIL")
    os.environ["R3DG_IMAGE_TAIL"] = "1" if tail_on else "0"
    try:
        dev = torch.device("cuda", 0)
        scene = syn.make_scene(P=3000, seed=5, stage2=True, scale_log_mean=-3.0)
        cam = syn.orbit_cameras(4, width=70, height=45)[1].to(dev)
        bg = torch.ones(3, device=dev)
        params = GaussianParams(scene, dev, True)
        with torch.no_grad():
            gt = render_stage1(params, cam, bg)[2].clone() * 0.9
        step = FusedStage2Step(params, 8, lr=1e-3)
        seen = {}
        inner = step._image_loss

        def spy(v, fw):
            g, active = inner(v, fw)
            seen["g"], seen["active"] = g, list(active)
            return g, active
        step._image_loss = spy
        step.forward_backward(cam, bg, gt)
        torch.cuda.synchronize()
        outs = step.last_outs                      # the rasterizer's public outputs: 6 = pseudo normal, 7 = surface xyz
        from relightable3dgaussian_amd.fused_step import LAMBDA_DSSIM
        slack = 2.0 * LAMBDA_DSSIM * (step.w["l1"] + step.w["pbr"])
        return (float(step.loss()), seen["g"][:20].detach().cpu().clone(), sorted(set(seen["active"])),
                outs[6].detach().cpu().clone(), outs[7].detach().cpu().clone(), seen["g"].shape[0], slack)
    finally:
        if old is None:
            os.environ.pop("R3DG_IMAGE_TAIL", None)
        else:
            os.environ["R3DG_IMAGE_TAIL"] = old


def test_whole_iteration_with_the_tail_on_and_off():
    """Both paths run the same kernels up to the tail on the same inputs, so the two slabs are two evaluations of ONE function:
    each within the kernel-level bound of the exact value, hence within twice that bound of each other.  The bound per element is
    n 2^-24 x (the element's scale); without the float64 reference of a rendered scene at hand, |value| stands in for the scale
    where it is the smaller of the two (a tighter bound, never a wider one) plus the plane's largest |value| x 2^-24 x n for the
    elements whose addends cancel.  loss(): the sums' n, relative to |loss| + 2 lambda (w_l1 + w_pbr) -- the loss is
    lambda (w_l1 + w_pbr) plus the weighted sums, of which the two SSIM terms are negative and no larger than that constant."""
    loss_on, g_on, act_on, pn_on, sx_on, planes_on, slack = _iteration(True)
    loss_off, g_off, act_off, pn_off, sx_off, planes_off, _ = _iteration(False)
    assert planes_on == 20 and planes_off == 47 and act_on == act_off
    assert torch.equal(pn_on, pn_off) and torch.equal(sx_on, sx_off)
    n_loss = _n_sum(50 + 26, 21, 4 * _tiles(70, 45)) + _n_sum(50, 4, 3 * _tiles(70, 45))
    print("whole iteration 70x45  loss on %.9g off %.9g  rel %.2e  bound %.2e" % (
        loss_on, loss_off, abs(loss_on - loss_off) / (abs(loss_off) + slack), n_loss * gr.U32))
    assert abs(loss_on - loss_off) <= n_loss * gr.U32 * (abs(loss_off) + slack)
    # planes 0..3, and of the feature gradients 4 + k the ACTIVE maps k (the others are not written by either path): the tail's
    # count for the maps it writes, + 2 where the smoothness / supervision kernels behind it ADD to what it wrote (one rounding
    # each: dL_dopacity and the normal maps); the maps those kernels write alone come from identical inputs on both paths: n = 1
    n_plane = [N_DIMAGE] * 3 + [N_DOPACITY + 2] + [0] * 16
    for k in act_on:
        n_plane[4 + k] = float(N_DFEATURE[k, 0]) + (2 if k in (5, 6, 7) else 0) if k in (2, 3, 4, 5, 6, 7) else 1
    for p, n in enumerate(n_plane):
        if n == 0:
            continue
        a, b = _np(g_on[p]), _np(g_off[p])
        bound = 2.0 * n * gr.U32 * (np.minimum(np.abs(a), np.abs(b)) + np.abs(b).max()) + gr.TINY
        err = np.abs(a - b)
        print("whole iteration 70x45  plane %2d  n %3d  max err/bound %.3f" % (p, n, float((err / bound).max())))
        assert (err <= bound).all(), "plane %d: %d elements beyond twice the kernel-level bound" % (p, int((err > bound).sum()))
