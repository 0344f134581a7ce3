"""The tile backward's gradient records read in place (r3dg_rasterize_backward_split with record outputs, r3dg_stage2_unpack_gradients_records,
r3dg_stage2_activate_backward_with_records) against the scatter pass and the three kernels that read its arrays
(r3dg_gradient_records_scatter / r3dg_rasterize_backward_split without them, r3dg_stage2_unpack_gradients,
r3dg_stage2_activate_backward_with).  Given the same record contents each reader runs the same arithmetic on the same values
whichever place it loads them from, so every output is compared BIT FOR BIT.

The fixture is that of tests/test_sh_adam_in_backward_gpu.py: upstream pixel gradients that are non-zero in two 8x8 blocks only
(one wave of the tile kernel each, so a record element receives at most two non-zero terms and the tile sums are the same in every
run -- asserted first, on the records themselves), the camera at the scene's edge so that culled and live rows share a 256-row
block.  S = 16 feature columns, no depth gradient: the instances a stage-2 iteration with trained geometry selects.

How the two paths meet the same records: the geometry backward has no entry point that reads a COPY of the rows (it reads the
library's own, behind the fill, in one call), so path B is the records call itself followed by the two record readers on the
library's rows, and path A is the scatter pass on a copy of those rows followed by the array readers, with the classic backward
(whose own fill leaves, by the fixture, the same rows) for the geometry outputs.  The scatter's arrays are compared with the
classic backward's as well, which ties the copy to that fill."""
import os

import numpy as np
import pytest
import torch

from tests.helpers import fwd_args, make_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = (1, 255, 256, 257, 300)
W, H = 64, 48
LAYOUTS = {"pbr": [2, 3, 4], "pbr_normal": [2, 3, 4, 5, 6, 7], "depth_pbr_normal": [0, 2, 3, 4, 5, 6, 7]}
LR, LR_TAIL, BETAS, EPS = 2.5e-3, 1.25e-4, (0.9, 0.999), 1e-15
GEOMETRY = {0: "dL_dmeans2D", 3: "dL_dmeans3D", 5: "dL_dcov3D", 6: "dL_dsh", 7: "dL_dscales", 8: "dL_drotations"}
CHAIN = (("g_xyz", 3), ("g_scaling", 3), ("g_rotation", 4), ("g_opacity", 1), ("g_normal", 3), ("g_base", 3), ("g_rough", 1))
HE, WE = 3, 5


def _case(P, behind=False):
    case = make_case(P=P, W=W, H=H, S=16, seed=60 + P, eye=(1.0, 0.3, 0.5), scale_log_mean=-2.5)
    if behind:          # every Gaussian behind the camera (it looks from `eye` at the origin): nothing is rendered
        case["means3D"] = 0.1 * case["means3D"] + 2.0 * torch.tensor([1.0, 0.3, 0.5])
    return case


def _upstream(seed, active):
    """Pixel gradients (colour, opacity, 16 feature maps) that are zero outside two 8x8 blocks on the 8-pixel grid, and in every
    feature map outside `active` (None: all maps carry one)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for c in (3, 1, 16):
        t = torch.zeros(c, H, W)
        for y0, x0 in ((8, 16), (24, 40)):
            t[:, y0:y0 + 8, x0:x0 + 8] = torch.randn(c, 8, 8, generator=g)
        out.append(t)
    if active is not None:
        keep = torch.zeros(16, 1, 1)
        keep[active] = 1.0
        out[2] = out[2] * keep
    return [t.to(DEV) for t in out]


def _backward(a, out, ups, shs, active, **kw):
    from relightable3dgaussian_amd import rasterizer_ops
    return rasterizer_ops.rasterize_gaussians_backward(
        a[0], a[1], a[2], out[9], a[3], a[5], a[6], 1.0, a[8], a[9], a[10], a[11], a[12], ups[0], ups[1], torch.Tensor([]),
        ups[2], shs, a[18], a[19], out[10], out[0], out[11], out[12], True, False, active_features=active, **kw)


def _records():
    from relightable3dgaussian_amd import rasterizer_ops
    return rasterizer_ops.GradientRecords()


def _call(name, *args):
    from relightable3dgaussian_amd import _lib
    _lib.check(getattr(_lib.lib(), name)(_lib.current_stream(), *args), name)


def _optimizer(shs, P):
    from relightable3dgaussian_amd.fused_adam import FusedAdam
    g = torch.Generator().manual_seed(7 * P)
    opt = FusedAdam([dict(param=shs.clone(), lr=LR, lr_tail=LR_TAIL, period=48, split=3)], betas=BETAS, eps=EPS)
    opt.groups[0]["exp_avg"].copy_((0.01 * torch.randn(P, 16, 3, generator=g)).to(DEV))
    opt.groups[0]["exp_avg_sq"].copy_(((0.01 * torch.randn(P, 16, 3, generator=g)) ** 2).to(DEV))
    return opt, opt.groups[0]


class _Glue:
    """The inputs of the unpack and the activation chain rule that do not come from the rasterizer, and one run of either pair of
    entry points on them (every run gets fresh outputs and a fresh copy of the texture-gradient accumulator, which the chain rule
    consumes)."""

    def __init__(self, P, a):
        g = torch.Generator().manual_seed(900 + P)
        r = lambda *s: torch.randn(*s, generator=g).to(DEV)
        self.P, self.xyz, self.vm, self.campos = P, a[1], a[9].contiguous(), a[19].contiguous()
        self.scaling, self.rotation, self.opacity, self.normal = r(P, 3), r(P, 4), r(P, 1), r(P, 3)
        self.base, self.rough = r(P, 3), r(P, 1)
        self.shade_out = r(P, 19)
        self.d_base, self.d_rough, self.d_view = r(P, 3), r(P, 1), r(P, 3)
        self.env_raw, self.env, self.d_env = r(HE, WE, 3), r(HE, WE, 3).abs(), r(HE, WE, 3)

    def unpack(self, source, records):
        from relightable3dgaussian_amd import _abi
        P, nb = self.P, (self.P + 255) // 256
        out = dict(dL_dpbr=torch.full((P, 3), 7.0, device=DEV), dL_ddiffuse=torch.full((P, 3), 7.0, device=DEV),
                   block_absmax=torch.full((nb,), 7.0, device=DEV),
                   light_l1_sum=torch.zeros(_abi.constants["R3DG_SUM_SLOTS"], device=DEV))
        _call("r3dg_stage2_unpack_gradients_records" if records else "r3dg_stage2_unpack_gradients", P, *source,
              self.shade_out.data_ptr(), 0.37 / (3.0 * P), out["dL_dpbr"].data_ptr(), out["dL_ddiffuse"].data_ptr(),
              out["block_absmax"].data_ptr(), out["light_l1_sum"].data_ptr())
        if P > 256:            # (more than one block: the order of the blocks' atomics is not fixed)
            del out["light_l1_sum"]
        return out

    def chain(self, source, dL_dopacity, bw, records):
        P = self.P
        out = {k: torch.full((P, c), 7.0, device=DEV) for k, c in CHAIN}
        out["g_env_raw"] = torch.full((HE * WE * 3,), 7.0, device=DEV)
        out["dL_denv"] = self.d_env.clone()
        p = lambda t: t.data_ptr()
        head = (P, p(self.xyz), p(self.scaling), p(self.rotation), p(self.opacity), p(self.normal), p(self.base), p(self.rough),
                p(self.vm), p(self.campos))
        grads = (p(self.d_base), p(self.d_rough), p(self.d_view), p(bw[7]), p(bw[8])) + \
            (() if records else (p(dL_dopacity),)) + (p(bw[3]),)
        tail = tuple(p(out[k]) for k, _ in CHAIN) + (HE, WE, p(self.env_raw), p(self.env), p(out["dL_denv"]), 0.37,
                                                     p(out["g_env_raw"]), None, 1)
        _call("r3dg_stage2_activate_backward_with_records" if records else "r3dg_stage2_activate_backward_with",
              *head, *source, *grads, *tail)
        return out


def _same(tag, got, want):
    for k in want:
        assert got[k].shape == want[k].shape and torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), \
            "%s: %s differs (largest |difference| %.3e)" % (tag, k, float((got[k] - want[k]).abs().max()))


def _paths(P, active, behind=False):
    """Both paths on one fixture -> (path A's outputs, path B's outputs, the copies of the rows after the two fills, the
    library's rows after path B, the rasterizer's forward outputs)."""
    from r3dg_rasterization import _C
    case = _case(P, behind)
    a = fwd_args(case, DEV)
    out = _C.rasterize_gaussians(*a)
    ups = _upstream(P, active)
    glue = _Glue(P, a)
    A, B = {}, {}
    # ---- path B, and the fixture's promise: two fills leave the same rows (the first fill is ABANDONED -- its rows are never
    # zeroed -- so the second one also passes through the clearing of a buffer that was left dirty)
    rows1 = _records()
    bw_b = _backward(a, out, ups, a[17], active, gradient_records=rows1)
    assert rows1, "the library has no 16-float records for active_features=%r" % (active,)
    assert bw_b[1] is None and bw_b[2] is None and bw_b[4] is None
    copy1 = rows1.tensor().clone()
    opt_b, grp_b = _optimizer(a[17], P)
    rows = _records()
    bw_b_adam = _backward(a, out, ups, grp_b["param"], active, gradient_records=rows,
                          sh_adam=opt_b.fused_step_of(0, 1, 1.0, None))
    assert rows and rows.ptr == rows1.ptr and list(rows.layout) == list(rows1.layout)
    copy2 = rows.tensor().clone()
    B.update({GEOMETRY[i]: bw_b[i] for i in GEOMETRY})
    B.update({"adam " + GEOMETRY[i]: bw_b_adam[i] for i in GEOMETRY if i != 6})
    B.update({"sh " + k: grp_b[k] for k in ("param", "exp_avg", "exp_avg_sq")})
    B.update(glue.unpack((rows.ptr, rows.layout), True))
    B.update(glue.chain((rows.ptr, rows.layout), None, bw_b_adam, True))
    torch.cuda.synchronize()
    after = rows.tensor().clone()
    # ---- path A: the scatter pass on a copy of the rows, the classic backward, the array readers
    S = 16
    arr = dict(dL_dmeans2D_raw=torch.full((P, 3), 7.0, device=DEV), dL_dconic=torch.full((P, 4), 7.0, device=DEV),
               dL_dopacity=torch.full((P, 1), 7.0, device=DEV), dL_dcolors=torch.full((P, 3), 7.0, device=DEV),
               dL_dfeatures=torch.full((P, S), 7.0, device=DEV))
    scattered = copy1.clone()
    _call("r3dg_gradient_records_scatter", P, S, scattered.data_ptr(), rows.layout, *[t.data_ptr() for t in arr.values()])
    bw_a = _backward(a, out, ups, a[17], active)
    opt_a, grp_a = _optimizer(a[17], P)
    bw_a_adam = _backward(a, out, ups, grp_a["param"], active, sh_adam=opt_a.fused_step_of(0, 1, 1.0, None))
    A.update({GEOMETRY[i]: bw_a[i] for i in GEOMETRY})
    A.update({"adam " + GEOMETRY[i]: bw_a_adam[i] for i in GEOMETRY if i != 6})
    A.update({"sh " + k: grp_a[k] for k in ("param", "exp_avg", "exp_avg_sq")})
    A.update(glue.unpack((arr["dL_dfeatures"].data_ptr(),), False))
    A.update(glue.chain((arr["dL_dfeatures"].data_ptr(),), arr["dL_dopacity"], bw_a_adam, False))
    torch.cuda.synchronize()
    classic = dict(dL_dopacity=bw_a[2], dL_dcolors=bw_a[1], dL_dfeatures=bw_a[4])
    return A, B, (copy1, copy2), after, scattered, arr, classic, out


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("P", SIZES)
def test_readers_of_the_records_against_the_scatter_pass(P, layout):
    active = LAYOUTS[layout]
    A, B, (copy1, copy2), after, scattered, arr, classic, out = _paths(P, active)
    tag = "P=%d %s" % (P, layout)
    if P >= 255:
        live = int((out[9] > 0)[:256].sum())
        assert 0 < live < min(P, 256), "the first block needs culled and live rows"
    assert copy1.shape == (P, 16)
    assert torch.equal(copy1.view(torch.int32), copy2.view(torch.int32)), tag + ": the fixture's tile sums differ between two fills"
    if P > 1:
        assert float(copy1.abs().max()) > 0.0, tag + ": the tile kernel left nothing in the records"
    # the scatter pass alone = the classic backward's arrays; it hands the rows back as zeros
    _same(tag + " scatter vs classic backward", arr, classic)
    assert int(scattered.view(torch.int32).abs().max()) == 0, tag + ": the scatter pass left a non-zero record"
    # every output of the three readers
    assert sorted(A) == sorted(B)
    _same(tag, B, A)
    if P > 1:
        for k in ("dL_dmeans3D", "dL_dsh", "dL_dpbr", "g_opacity", "g_xyz"):
            assert float(A[k].abs().max()) > 0.0, tag + ": %s is all zeros, the comparison is empty" % k
        assert not torch.equal(A["sh param"], _case(P)["shs"].to(DEV))
    # the last reader zeroed the rows
    assert int(after.view(torch.int32).abs().max()) == 0, tag + ": the record rows are not all zeros behind the chain rule"


def test_identity_list_falls_back_to_the_scatter_pass():
    """All S = 16 channels live: 32-float records, which no reader takes in place.  The entry point says so without an error and
    the backward that was handed an (empty) GradientRecords is the classic one, array for array."""
    from r3dg_rasterization import _C
    P = 300
    a = fwd_args(_case(P), DEV)
    out = _C.rasterize_gaussians(*a)
    ups = _upstream(P, None)
    rows = _records()
    got = _backward(a, out, ups, a[17], None, gradient_records=rows)
    want = _backward(a, out, ups, a[17], None)
    torch.cuda.synchronize()
    assert not rows and rows.ptr is None
    for i in range(9):
        assert got[i] is not None and torch.equal(got[i].view(torch.int32), want[i].view(torch.int32)), "output %d differs" % i
    assert float(want[4].abs().max()) > 0.0


@pytest.mark.parametrize("P", (1, 300))
def test_nothing_rendered(P):
    """Every Gaussian behind the camera: no tile kernel runs, the rows are the zeros the buffer holds between calls, and the
    readers' outputs are those of the classic path (which fills its arrays with zeros)."""
    A, B, (copy1, copy2), after, _scattered, arr, classic, out = _paths(P, LAYOUTS["pbr_normal"], behind=True)
    assert out[0] == 0 and int((out[9] > 0).sum()) == 0
    assert int(copy1.view(torch.int32).abs().max()) == 0 and int(copy2.view(torch.int32).abs().max()) == 0
    assert int(after.view(torch.int32).abs().max()) == 0
    _same("R=0 scatter vs classic backward", arr, classic)
    _same("R=0", B, A)


def test_abandoned_fill_then_classic_backward():
    """A records fill whose readers never run leaves non-zero rows behind.  The classic backward that follows on the same stream
    finds the buffer marked dirty, clears it, and computes what it computes from a clean buffer."""
    from r3dg_rasterization import _C
    P, active = 300, LAYOUTS["pbr"]
    a = fwd_args(_case(P), DEV)
    out = _C.rasterize_gaussians(*a)
    ups = _upstream(P, active)
    want = _backward(a, out, ups, a[17], active)
    rows = _records()
    _backward(a, out, ups, a[17], active, gradient_records=rows)
    torch.cuda.synchronize()
    assert rows and float(rows.tensor().abs().max()) > 0.0
    got = _backward(a, out, ups, a[17], active)
    torch.cuda.synchronize()
    for i in range(9):
        assert torch.equal(got[i].view(torch.int32), want[i].view(torch.int32)), "output %d differs after an abandoned fill" % i
    assert int(rows.tensor().view(torch.int32).abs().max()) == 0, "the classic backward left its records non-zero"


# ---- whole iterations with the switch on and off ----------------------------------------------------------------------------------
def _two_steps(records_on):
    """Two consecutive FusedStage2Step.__call__ on the 70 x 45 scene of tests/test_image_tail_gpu.py's whole-iteration case ->
    (loss after the second step, {name: parameter tensor}, did the step read records in place)."""
    from relightable3dgaussian_amd import rasterizer_ops
    from relightable3dgaussian_amd import synthetic as syn
    from relightable3dgaussian_amd.bench_core import GaussianParams, render_stage1
    from relightable3dgaussian_amd.fused_step import LAMBDA_DSSIM, FusedStage2Step
    old = os.environ.get("R3DG_GRADIENT_RECORDS")
    os.environ["R3DG_GRADIENT_RECORDS"] = "1" if records_on else "0"
    used = []
    inner = rasterizer_ops.rasterize_gaussians_backward

    def spy(*args, **kw):
        res = inner(*args, **kw)
        used.append(bool(kw.get("gradient_records")))
        return res
    spy.sh_adam_supported, spy.gradient_records_supported = inner.sh_adam_supported, inner.gradient_records_supported
    rasterizer_ops.rasterize_gaussians_backward = spy
    try:
        dev = torch.device("cuda", 0)
        scene = syn.make_scene(P=3000, seed=5, stage2=True, scale_log_mean=-3.0)
        cam = syn.orbit_cameras(4, width=70, height=45)[1].to(dev)
        bg = torch.ones(3, device=dev)
        params = GaussianParams(scene, dev, True)
        with torch.no_grad():
            gt = render_stage1(params, cam, bg)[2].clone() * 0.9
        step = FusedStage2Step(params, 8, lr=1e-3)
        step(cam, bg, gt)
        step(cam, bg, gt)
        step.flush()
        torch.cuda.synchronize()
        state = {k: (step.incidents if k == "incidents" else getattr(step, k)).detach().cpu().clone() for k in step._opt_order}
        slack = 2.0 * LAMBDA_DSSIM * (step.w["l1"] + step.w["pbr"])
        return float(step.loss()), state, used, slack
    finally:
        rasterizer_ops.rasterize_gaussians_backward = inner
        if old is None:
            os.environ.pop("R3DG_GRADIENT_RECORDS", None)
        else:
            os.environ["R3DG_GRADIENT_RECORDS"] = old


def test_two_whole_iterations_with_the_switch_on_and_off():
    """Both settings run the same arithmetic on the same record contents; what differs between ANY two runs is the order of the
    tile backward's float atomics (and of the loss sums').  The bounds are those of tests/test_image_tail_gpu.py's whole-iteration
    case: the loss within n_loss 2^-24 (|loss| + 2 lambda (w_l1 + w_pbr)) with that test's n_loss; every parameter element within
    2 n 2^-24 (min(|a|, |b|) + max |b|) + tiny.  n for the parameters: a record channel is the sum of at most one addend per wave
    of the tile kernel (four per 16 x 16 tile, 5 x 3 tiles: 60 waves), whose order is free: n = 60 per step, 120 for the two.
    The second step is the one that reads records the first step's chain rule zeroed: rows left non-zero would double the
    gradients of the Gaussians in view, far outside the bound."""
    from tests import glue_reference as gr
    from tests.test_glue_kernels_gpu import _n_sum
    from tests.test_image_tail_gpu import _tiles
    loss_on, on, used_on, slack = _two_steps(True)
    loss_off, off, used_off, _ = _two_steps(False)
    assert used_on == [True, True] and used_off == [False, False], (used_on, used_off)
    n_loss = _n_sum(50 + 26, 21, 4 * _tiles(70, 45)) + _n_sum(50, 4, 3 * _tiles(70, 45))
    print("two iterations 70x45  loss on %.9g off %.9g  rel %.2e  bound %.2e" % (
        loss_on, loss_off, abs(loss_on - loss_off) / (abs(loss_off) + slack), n_loss * gr.U32))
    assert abs(loss_on - loss_off) <= n_loss * gr.U32 * (abs(loss_off) + slack)
    n = 2 * 4 * ((70 + 15) // 16) * ((45 + 15) // 16)          # (the rasterizer's 16 x 16 tiles, four waves each)
    assert sorted(on) == sorted(off)
    failed = []
    for k in sorted(on):
        a, b = on[k].numpy().astype(np.float64), off[k].numpy().astype(np.float64)
        bound = 2.0 * n * gr.U32 * (np.minimum(np.abs(a), np.abs(b)) + np.abs(b).max()) + gr.TINY
        err = np.abs(a - b)
        print("two iterations 70x45  %-12s n %3d  max err/bound %.3e" % (k, n, float((err / bound).max())))
        if not (err <= bound).all():
            failed.append("%s: %d elements beyond the bound" % (k, int((err > bound).sum())))
    assert not failed, failed
