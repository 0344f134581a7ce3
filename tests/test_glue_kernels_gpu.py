"""Every glue kernel of the two fused iterations (csrc/stage2_glue.hip, csrc/stage1_glue.hip) on its own, through the C ABI, against
its float64 restatement (tests/glue_reference.py) -- no element left out, no outlier fraction.  Inputs: tests/glue_cases.py (crafted
edge rows + seeded random rows; the distributions are in the builders' docstrings).  Every output is a view into a larger buffer
filled with a canary; the canaries must survive, and outputs the contract calls "not touched" must keep theirs.

TOLERANCE (measured against the reference, never the kernel; the convention of tests/test_neilf_dataset_gpu.py).  For each output,
d = max |ref32 - ref64| / scale with ref32 the same restatement in float32 on the CPU and `scale` the per-element sum of absolute
addends; every element must satisfy |kernel - ref64| <= max(2 d, n 2^-24) scale (+ 2^-126, the float32 format's underflow: a value
below it may come out as 0).  Where the reference is exactly 0 the kernel must be exactly 0; d must stay below 1e-5.  Each test prints
d, n and the measured largest err / bound per output (the MI355X table: profiles/r14_glue_parity.txt).

n = float32 roundings on the kernel's longest path to that output (E(x) = 4 + ceil(|x| log2 e) for __expf(x) / __logf: 4 for the
instruction pair plus the rounding of the scaled argument; S(x) = E(x) + 2 for sigmoidf_; both PER ELEMENT, never more than at the
case's largest |x|; srgb_pow = 8, the "~4 ulp" of glue_math.hpp):
  per-pixel x = F (1/opc) op + (1 - op) bg            6 (rcp, 3 mul, sub, add)
  srgb            x's 6 / 2.4 -> 3, srgb_pow 8, * 1.055, - 0.055                                        13
  dsrgb           x's 6 * 0.58 -> 4, srgb_pow 8, constant and its product 2                             14
  s2 dL_dfeature 2..4   dsrgb 14, (w sign + extra) * 3, * op * scale 2, scale 1                         20
  s2 dL_dfeature 5..7   dn = (Fn scale - pn) mk 4, 2 w dn mk 3, * scale 2                                10  (rounded up)
  s2 dL_dopacity  gx 17, r - bg + op F dscale (rcp of a square 2, 2 mul, 2 add) 6, * gx 1, six accumulations 6 -> 30; taken 32
  dL_dimage (both stages)  w * sign + extra                                                              2
  s1 dL_dfeature 0..2   e = __expf(-|G gt|): E(1) = 6 + the stencil's 8; 18 accumulated products 18 + 2; + the normal term and
                  its add 2 -> 36; * scale 2                                                              38
  s1 dL_dfeature 3 / 4  var 6, sqrt 1, max 0, 0.5 w / sd 3 -> dvar 10; * scale 2 -> 12; * -2 D (D: 2) 4 -> 16
  s1 dL_dopacity  the normal maps' 38 + Fn dscale 5 + five accumulations                                  48
  activations     scales E(raw); rotation / normal 6 (4 squares and adds -> sqrt halves, max, rcp, mul); opacity S(raw);
                  base colour / roughness S(raw) + 3; view direction 8 (the difference first); depth 5 (3 products, adds), depth^2 11;
                  texture softplus 6 (expf and log1pf are the library's, 1-2 ulp each)
  chain rule      g_scaling E(raw) + 1; g_opacity S(raw) + 4; g_base / g_rough S(raw) + 6 (sum, constant, s, 1 - s, products);
                  g_rotation / g_normal 24 (norm 3, rcp or quotient 1 + 3, dot 4, product, difference, * inv and its 4; rounded up);
                  g_xyz 28 (the view direction's 24, the depth columns' and the two adds)
  unpack dL_ddiffuse   (s0+s1+s2)/3 3, s - sm, * weight, + g                                              6
  texture g_raw   four differences * 2 inv (inv: 3) accumulated, * w_tv, + dL_denv, * softplus'           12 + S(raw)
  sums (atomics)  n = the addend's own + additions per thread + 8 (block reduction) + workgroups per slot (R3DG_SUM_SLOTS = 32 slots);
                  addends: |image - gt| 2, |srgb - gt| 14, dn^2 10, entropy 28 (E(13.8) = 24 + 4), sqrt(var) 8, edge 24
                  (stencil 8, |.| e 6 + 8, two products and an add), light 6, TV 8; the result is read as the sum over the slots."""
import math

import numpy as np
import pytest
import torch

from tests import glue_cases as gc
from tests import glue_reference as gr
from tests.helpers import report_elementwise

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = -7.5
PAD = 64                                  # floats of canary either side of an output (256 bytes: every vector access stays aligned)
SLOTS = gr.SUM_SLOTS
F64 = torch.float64
_REFS = {}
_KEEP = []


def _L():
    from relightable3dgaussian_amd import _lib
    return _lib


def _call(name, *args):
    lib = _L()
    lib.check(getattr(lib.lib(), name)(lib.current_stream(), *args), name)


def _p(t):
    return None if t is None else t.data_ptr()


def _dev(t):
    """`t` on the device, kept alive until the test ends (the kernels read it after this returns)."""
    if t is None:
        return None
    _KEEP.append(t.to(DEV).contiguous())
    return _KEEP[-1]


@pytest.fixture(autouse=True)
def _release_inputs():
    yield
    torch.cuda.synchronize()
    del _KEEP[:]


class Out:
    """A device output of `shape` inside a canary-filled buffer; `init` (a value) instead of the canary for accumulators."""

    def __init__(self, *shape, init=CANARY, dtype=torch.float32):
        n = int(np.prod(shape)) if shape else 1
        self.big = torch.full((n + 2 * PAD,), CANARY, device=DEV, dtype=dtype)
        self.t = self.big[PAD:PAD + n].view(*shape)
        if init != CANARY:
            self.t.fill_(init)

    def ptr(self):
        return self.t.data_ptr()

    def cpu(self):
        """The output on the host, after checking the canaries either side of it."""
        torch.cuda.synchronize()
        big = self.big.cpu()
        assert bool((big[:PAD] == CANARY).all()) and bool((big[-PAD:] == CANARY).all()), "canary overwritten"
        return big[PAD:-PAD].view(*self.t.shape)

    def untouched(self):
        return bool((self.cpu() == CANARY).all())


def _refs(key, fn, *args, **kw):
    """(ref64, ref32) of a restatement for a case: computed once, shared, never modified."""
    if key not in _REFS:
        _REFS[key] = (fn(*gr.widen(args, F64), **kw), fn(*args, **kw))
    return _REFS[key]


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64) if isinstance(t, torch.Tensor) else np.asarray(t, np.float64)


def _check(kernel, name, got, refs, n, index=None):
    """One output array of `kernel` against the rule of the module docstring; `index` selects a sub-array of the reference."""
    sel = (lambda a: a) if index is None else (lambda a: a[index])
    r64, s64 = (sel(_np(a)) for a in refs[0][name])
    r32 = sel(_np(refs[1][name][0]))
    got = _np(got).reshape(r64.shape)
    n = np.broadcast_to(np.asarray(n, np.float64), r64.shape)
    d, bound = gr.tolerance(r64, r32, s64, n)
    ok, msg = report_elementwise("%s %s" % (kernel, name), got, r64, bound)
    print("%-34s %-13s d %.2e  n %4d  %s" % (kernel, name, d, int(n.max()) if n.size else 0, msg.split("max err/bound", 1)[-1].strip()))
    assert d < 1e-5, "%s %s: badly conditioned case, d = %.3e" % (kernel, name, d)
    assert ok, msg
    zero = r64 == 0
    assert not (got[zero] != 0).any(), "%s %s: %d elements are exactly 0 in the reference and not in the kernel" % (
        kernel, name, int((got[zero] != 0).sum()))


def _n_sum(addend, per_thread, blocks):
    return addend + per_thread + 8 + math.ceil(blocks / SLOTS)


def _slot_sum(out, q=0):
    return out.cpu().double().reshape(-1, SLOTS)[q].sum()


# ---- stage 2, per pixel -------------------------------------------------------------------------------------------------------------
S2_SHAPES = [(1, 1), (5, 7), (51, 5), (257, 1)]
S2_LOSS_SHAPES = S2_SHAPES + [(3, 65537)]                        # 768 * 256 + 3 pixels: the 768-workgroup grid takes a second trip
_S2 = {}


def _s2_case(W, H):
    if (W, H) not in _S2:
        _S2[(W, H)] = gc.s2_pixels(W * H, seed=1000 + W * 7 + H)
    return _S2[(W, H)]


@pytest.mark.parametrize("w_normal", [0.0, 0.3])
@pytest.mark.parametrize("sparse", [0, 1])
@pytest.mark.parametrize("W,H", S2_LOSS_SHAPES)
def test_stage2_loss(W, H, sparse, w_normal):
    c = _s2_case(W, H)
    HW = W * H
    d = {k: _dev(c[k]) for k in ("image", "opacity", "feature", "pseudo", "n_contrib", "gt", "bg", "mask", "extra_dimage", "extra_dsrgb")}
    w_l1, w_pbr = 0.8, 0.6
    blocks = min((HW + 255) // 256, 768)
    trips = math.ceil(HW / (blocks * 256))
    for masked, extras in ((False, False), (True, True), (True, False), (False, True)):
        mask = c["mask"] if masked else None
        ei, es = (c["extra_dimage"], c["extra_dsrgb"]) if extras else (None, None)
        refs = _refs(("s2loss", W, H, sparse, w_normal, masked, extras), gr.stage2_loss, c["image"], c["opacity"], c["feature"],
                     c["pseudo"], c["n_contrib"], c["gt"], c["bg"], mask, w_l1, w_pbr, w_normal, ei, es, sparse=bool(sparse))
        gi, go, gf, sums = Out(3, HW), Out(HW), Out(16, HW), Out(3 * SLOTS, init=0.0)
        _call("r3dg_stage2_loss", W, H, _p(d["image"]), _p(d["opacity"]), _p(d["feature"]), _p(d["pseudo"]), _p(d["n_contrib"]),
              _p(d["gt"]), _p(d["bg"]), _p(d["mask"]) if masked else None, w_l1, w_pbr, w_normal,
              _p(d["extra_dimage"]) if extras else None, _p(d["extra_dsrgb"]) if extras else None, gi.ptr(), go.ptr(), gf.ptr(),
              sums.ptr(), sparse)
        tag = "s2_loss<%d> wn=%g m%d e%d %dx%d" % (sparse, w_normal, masked, extras, W, H)
        _check(tag, "dL_dimage", gi.cpu(), refs, 2)
        _check(tag, "dL_dopacity", go.cpu(), refs, 32)
        written = [2, 3, 4] + ([5, 6, 7] if (not sparse or w_normal != 0.0) else [])
        if not sparse:
            written = list(range(16))
        n_map = np.zeros((16, 1))
        n_map[2:5], n_map[5:8] = 20, 10
        got_f = gf.cpu()
        _check(tag, "dL_dfeature", got_f[written], refs, n_map[written], index=written)
        rest = [k for k in range(16) if k not in written]
        assert bool((got_f[rest] == CANARY).all()), "%s: a feature-gradient map outside the sparse set was written" % tag
        _check(tag, "sum_l1", _slot_sum(sums, 0), refs, _n_sum(2, 3 * trips, blocks))
        _check(tag, "sum_pbr", _slot_sum(sums, 1), refs, _n_sum(14, 3 * trips, blocks))
        if "sum_normal" in refs[0]:
            _check(tag, "sum_normal", _slot_sum(sums, 2), refs, _n_sum(10, 3 * trips, blocks))
        else:
            assert float(_slot_sum(sums, 2)) == 0.0


@pytest.mark.parametrize("W,H", S2_SHAPES)
def test_stage2_pbr_srgb(W, H):
    c = _s2_case(W, H)
    refs = _refs(("srgb", W, H), gr.stage2_pbr_srgb, c["opacity"], c["feature"], c["n_contrib"], c["bg"])
    d = {k: _dev(c[k]) for k in ("opacity", "feature", "n_contrib", "bg")}
    out = Out(3, W * H)
    _call("r3dg_stage2_pbr_srgb", W, H, _p(d["opacity"]), _p(d["feature"]), _p(d["n_contrib"]), _p(d["bg"]), out.ptr())
    _check("s2_pbr_srgb %dx%d" % (W, H), "srgb", out.cpu(), refs, 13)


def _pseudo_normal_oracle(opacity, depth, vm, fx, fy, cx, cy):
    from oracle import torch_rasterizer as trz
    H, W = depth.shape[-2:]
    n, xyz = trz.pseudo_normal(opacity.reshape(1, H, W), depth.reshape(1, H, W), vm.reshape(4, 4), fx, fy, cx, cy)
    return {"pseudo_normal": (n, torch.ones_like(n)), "surface_xyz": (xyz, xyz.abs())}


@pytest.mark.parametrize("W,H", [(1, 1), (63, 3), (64, 4), (65, 5), (130, 9)])
def test_stage2_normals_srgb(W, H):
    """The tile is 64 x 4.  sRGB half: the reference; pseudo-normal half: oracle.torch_rasterizer.pseudo_normal (forward.cu:398-491),
    the oracle path the rasterizer's own pass is tested against, in float64 (scale 1 for the unit normal, n = 24: the surface
    points 5, the stencils 6, the cross product 3, the norm 3, the division, the rotation 3, rounded up; surface point: n = 5, the
    focal length, two divisions, the difference and the product).  Depth: a tilted plane + 5 % noise, premultiplied by the case's
    opacity (the edge rows' 0, 9e-6, 1e-5 included)."""
    HW = W * H
    c = gc.s2_pixels(HW, seed=2000 + W)
    g = torch.Generator().manual_seed(W * 31 + H)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    op = c["opacity"].reshape(H, W)
    depth = (2.0 + 0.9 * xs / max(W, 2) + 0.7 * ys / max(H, 2)) * (1.0 + 0.05 * torch.rand(H, W, generator=g)) * op
    vm = gc.gaussians(1, seed=1)["viewmatrix"]
    tfx, tfy, cx, cy = 0.6, 0.45, 0.5 * W + 0.25, 0.5 * H - 0.5
    refs = _refs(("nsrgb", W, H), gr.stage2_pbr_srgb, c["opacity"], c["feature"], c["n_contrib"], c["bg"])
    refn = _refs(("pn", W, H), _pseudo_normal_oracle, op, depth, vm, W / (2.0 * tfx), H / (2.0 * tfy), cx, cy)
    d = {k: _dev(c[k]) for k in ("opacity", "feature", "n_contrib", "bg")}
    pn, sx, srgb = Out(3, HW), Out(3, HW), Out(3, HW)
    _call("r3dg_stage2_normals_srgb", W, H, _p(_dev(vm)), tfx, tfy, cx, cy, _p(d["opacity"]), _p(_dev(depth)), pn.ptr(), sx.ptr(),
          _p(d["feature"]), _p(d["n_contrib"]), _p(d["bg"]), srgb.ptr())
    tag = "s2_normals_srgb %dx%d" % (W, H)
    _check(tag, "srgb", srgb.cpu(), refs, 13)
    _check(tag, "surface_xyz", sx.cpu().reshape(3, H, W), refn, 5)
    _check(tag, "pseudo_normal", pn.cpu().reshape(3, H, W), refn, 24)


# ---- stage 1, per pixel -------------------------------------------------------------------------------------------------------------
S1_WEIGHTS = {"l1": (0.8, 0, 0, 0, 0), "entropy": (0, 0.1, 0, 0, 0), "normal": (0, 0, 0.3, 0, 0), "smooth": (0, 0, 0, 0.2, 0),
              "var": (0, 0, 0, 0, 0.05), "all": (0.8, 0.1, 0.3, 0.2, 0.05)}
S1_SHAPES = [(1, 1), (1, 9), (9, 1), (5, 7), (64, 33)]
S1_BIG = [(1031, 509), (1031, 1019)]                              # second trips of the loss kernel / of the edge pass
_S1 = {}


def _s1_case(W, H):
    if (W, H) not in _S1:
        _S1[(W, H)] = gc.s1_pixels(W, H, seed=3000 + W * 5 + H)
    return _S1[(W, H)]


def _run_stage1_loss(W, H, wname, masked):
    c = _s1_case(W, H)
    HW = W * H
    w = [float(v) for v in S1_WEIGHTS[wname]]
    mask = c["mask"] if masked else None
    refs = _refs(("s1loss", W, H, wname, masked), gr.stage1_loss, W, H, c["image"], c["opacity"], c["feature"], c["pseudo"],
                 c["n_contrib"], c["gt"], mask, *w, c["extra_dimage"])
    d = {k: _dev(c[k]) for k in ("image", "opacity", "feature", "pseudo", "n_contrib", "gt", "mask", "extra_dimage")}
    gi, go, gf, sums, scratch = Out(3, HW), Out(HW), Out(5, HW), Out(6 * SLOTS, init=0.0), Out(6, HW)
    _call("r3dg_stage1_loss", W, H, _p(d["image"]), _p(d["opacity"]), _p(d["feature"]), _p(d["pseudo"]), _p(d["n_contrib"]), _p(d["gt"]),
          _p(d["mask"]) if masked else None, *w, _p(d["extra_dimage"]), scratch.ptr(), gi.ptr(), go.ptr(), gf.ptr(), sums.ptr())
    tag = "s1_loss %s m%d %dx%d" % (wname, masked, W, H)
    blocks, eblocks = min((HW + 255) // 256, 2048), min((HW + 255) // 256, 4096)
    trips, etrips = math.ceil(HW / (blocks * 256)), math.ceil(HW / (eblocks * 256))
    _check(tag, "dL_dimage", gi.cpu(), refs, 2)
    _check(tag, "dL_dopacity", go.cpu(), refs, 48)
    _check(tag, "dL_dfeature", gf.cpu(), refs, np.array([38, 38, 38, 16, 12], np.float64)[:, None])
    _check(tag, "sum_l1", _slot_sum(sums, 0), refs, _n_sum(2, 3 * trips, blocks))
    _check(tag, "sum_normal", _slot_sum(sums, 1), refs, _n_sum(10, 3 * trips, blocks))
    _check(tag, "sum_entropy", _slot_sum(sums, 2), refs, _n_sum(28, 2 * trips, blocks))
    _check(tag, "sum_var", _slot_sum(sums, 5), refs, _n_sum(8, trips, blocks))
    if w[3] != 0.0:
        _check(tag, "sum_edge", _slot_sum(sums, 4), refs, _n_sum(24, 6 * etrips, eblocks))
        scratch.cpu()
    else:
        assert float(_slot_sum(sums, 4)) == 0.0 and scratch.untouched()
    assert float(_slot_sum(sums, 3)) == 0.0                      # the SSIM slot is not this kernel's


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("wname", list(S1_WEIGHTS))
@pytest.mark.parametrize("W,H", S1_SHAPES)
def test_stage1_loss(W, H, wname, masked):
    _run_stage1_loss(W, H, wname, masked)


def test_stage1_loss_second_trip_of_the_loss_kernel():
    _run_stage1_loss(*S1_BIG[0], "all", True)                     # 524 779 pixels > 2048 * 256


def test_stage1_loss_second_trip_of_the_edge_pass():
    _run_stage1_loss(*S1_BIG[1], "smooth", False)               # > 4096 * 256 pixels, w_normal_smooth != 0


# ---- per Gaussian ------------------------------------------------------------------------------------------------------------------
P_SIZES = [1, 63, 64, 65, 255, 256, 257, 1000]
RAW = ("xyz", "scaling_raw", "rotation_raw", "opacity_raw", "normal_raw", "base_raw", "rough_raw")
_G = {}


def _g_case(P):
    if P not in _G:
        _G[P] = gc.gaussians(P, seed=4000 + P)
    return _G[P]


def _activate_outs(P):
    return dict(scales=Out(P, 3), rot=Out(P, 4), opacity=Out(P), normal=Out(P, 3), base_color=Out(P, 3), roughness=Out(P),
                viewdirs=Out(P, 3), features=Out(P, 16))


def _n_activate(a):
    sb, sr = gr.n_sig(a["base_raw"].numpy()) + 3, gr.n_sig(a["rough_raw"].numpy()) + 3
    nf = np.zeros((a["P"], 16))
    nf[:, 0], nf[:, 1], nf[:, 5:8], nf[:, 8:11], nf[:, 11] = 5, 11, 6, sb, sr
    return dict(scales=gr.n_exp(a["scaling_raw"].numpy()), rot=6, opacity=gr.n_sig(a["opacity_raw"].numpy()), normal=6, base_color=sb,
                roughness=sr, viewdirs=8, features=nf)


def _check_activate(tag, a, outs, stage2, with_features):
    refs = _refs(("act", a["P"], stage2, with_features), gr.stage2_activate,
                 a if stage2 else dict(a, base_raw=None), with_features=with_features)
    n = _n_activate(a)
    for k in ("scales", "rot", "opacity", "normal") + (("base_color", "roughness", "viewdirs") if stage2 else ()):
        _check(tag, k, outs[k].cpu(), refs, n[k])
    if not stage2:
        assert outs["base_color"].untouched() and outs["roughness"].untouched() and outs["viewdirs"].untouched()
    if stage2 and with_features:
        cols = [0, 1, 5, 6, 7, 8, 9, 10, 11]
        got = outs["features"].cpu()
        _check(tag, "features", got[:, cols], refs, n["features"][:, cols], index=(slice(None), cols))
        assert bool((got[:, [2, 3, 4, 12, 13, 14, 15]] == CANARY).all())
        # value for value the activations' own outputs
        assert torch.equal(got[:, 5:8], outs["normal"].cpu()) and torch.equal(got[:, 8:11], outs["base_color"].cpu())
        assert torch.equal(got[:, 11], outs["roughness"].cpu())
    else:
        assert outs["features"].untouched()


def _activate_args(d, outs, stage2, with_features):
    return [d["P"]] + [_p(d[k]) if (stage2 or k not in ("base_raw", "rough_raw")) else None for k in RAW] + [_p(d["campos"])] + \
        [outs[k].ptr() for k in ("scales", "rot", "opacity", "normal", "base_color", "roughness", "viewdirs")] + \
        [_p(d["viewmatrix"]), outs["features"].ptr() if with_features else None]


def _g_dev(a):
    return {k: (_dev(v) if isinstance(v, torch.Tensor) else v) for k, v in a.items()}


@pytest.mark.parametrize("P", P_SIZES)
def test_stage2_activate(P):
    a = _g_case(P)
    d = _g_dev(a)
    for stage2, with_features in ((True, True), (True, False), (False, False)):
        outs = _activate_outs(P)
        _call("r3dg_stage2_activate", *_activate_args(d, outs, stage2, with_features))
        _check_activate("s2_activate P=%d s2=%d f=%d" % (P, stage2, with_features), a, outs, stage2, with_features)


@pytest.mark.parametrize("n_zero", [0, 1, 6 * SLOTS])
@pytest.mark.parametrize("n_env", [0, 1, 255, 1536, 2049 + 8 * 256])
def test_stage2_activate_with_side_jobs(n_env, n_zero):
    """The two side jobs behind P = 257 Gaussians (two main workgroups), P = 0 (side jobs alone), the stage-1 use
    (d_base_raw == NULL) and d_features == NULL; 2049 + 8 * 256 texture floats make the 8 side workgroups loop."""
    raw = gc.env_texture(max(n_env, 1), seed=5000 + n_env)[:n_env]
    refs = _refs(("softplus", n_env), gr.softplus_env, raw)
    d_raw = _dev(raw) if n_env else None
    for P, stage2, with_features in ((257, True, True), (257, False, False), (257, True, False), (0, True, False)):
        a = _g_case(257)
        d = dict(_g_dev(a), P=P)
        outs = _activate_outs(max(P, 1))
        env, zero = Out(max(n_env, 1)), Out(max(n_zero, 1) + 5, init=3.0)
        _call("r3dg_stage2_activate_with", *_activate_args(d, outs, stage2, with_features), n_env, _p(d_raw), env.ptr() if n_env else None,
              zero.ptr() if n_zero else None, n_zero)
        tag = "s2_activate_with P=%d s2=%d f=%d env=%d zero=%d" % (P, stage2, with_features, n_env, n_zero)
        if P:
            _check_activate(tag, a, outs, stage2, with_features)
        else:
            assert all(o.untouched() for o in outs.values())
        if n_env:
            _check(tag, "env", env.cpu(), refs, 6)
        else:
            assert env.untouched()
        z = zero.cpu()
        assert bool((z[:n_zero] == 0).all()) and bool((z[n_zero:] == 3.0).all()), tag


def _shading(P):
    key = ("shade", P)
    if key not in _G:
        g = torch.Generator().manual_seed(6000 + P)
        _G[key] = (gc.shade_rows(P, seed=6100 + P), torch.randn(P, 16, generator=g))
    return _G[key]


@pytest.mark.parametrize("P", P_SIZES)
def test_stage2_pack_features(P):
    a = _g_case(P)
    so, _ = _shading(P)
    act = gr.stage2_activate(a, with_features=False)
    normal, base, rough = (act[k][0].contiguous() for k in ("normal", "base_color", "roughness"))
    refs = _refs(("pack", P), gr.stage2_pack_features, a["xyz"], a["viewmatrix"], normal, base, rough, so)
    for with_sum in (True, False):
        feats, lsum = Out(P, 16), Out(SLOTS, init=0.0)
        _call("r3dg_stage2_pack_features", P, _p(_dev(a["xyz"])), _p(_dev(a["viewmatrix"])), _p(_dev(normal)), _p(_dev(base)),
              _p(_dev(rough)), _p(_dev(so)), feats.ptr(), lsum.ptr() if with_sum else None)
        tag = "s2_pack_features P=%d sum=%d" % (P, with_sum)
        got = feats.cpu()
        n = np.zeros((P, 16))
        n[:, 0], n[:, 1] = 5, 11
        _check(tag, "features", got, refs, n)
        assert torch.equal(got[:, 2:], refs[1]["features"][0][:, 2:]), tag + ": a copied column differs"
        if with_sum:
            _check(tag, "light_l1_sum", _slot_sum(lsum), refs, _n_sum(6, 3, (P + 255) // 256))
        else:
            assert float(_slot_sum(lsum)) == 0.0


@pytest.mark.parametrize("P", P_SIZES)
def test_stage2_unpack_gradients(P):
    """Rows 0 and 1 carry three equal / all-zero diffuse channels: the light gradient there is exactly the feature gradient, and the
    light sum is the value r3dg_stage2_pack_features adds (bit for bit: the same expression)."""
    so, gfeat = _shading(P)
    lw = 0.37
    refs = _refs(("unpack", P), gr.stage2_unpack_gradients, gfeat, so, lw)
    nb = (P + 255) // 256
    d_so, d_g = _dev(so), _dev(gfeat)
    for with_max, with_sum in ((True, True), (False, False)):
        pbr, dif, amax, lsum = Out(P, 3), Out(P, 3), Out(nb), Out(SLOTS, init=0.0)
        _call("r3dg_stage2_unpack_gradients", P, _p(d_g), _p(d_so), lw, pbr.ptr(), dif.ptr(), amax.ptr() if with_max else None,
              lsum.ptr() if with_sum else None)
        tag = "s2_unpack P=%d max=%d sum=%d" % (P, with_max, with_sum)
        assert torch.equal(pbr.cpu(), gfeat[:, 2:5]), tag
        got = dif.cpu()
        _check(tag, "dL_ddiffuse", got, refs, 6)
        assert torch.equal(got[:min(P, 2)], gfeat[:min(P, 2), 12:15]), tag + ": sign(0) must be 0"
        if with_sum:
            _check(tag, "light_l1_sum", _slot_sum(lsum), refs, _n_sum(6, 3, nb))
            a = _g_case(P)
            packed = Out(SLOTS, init=0.0)
            feats = Out(P, 16)
            z3 = _dev(torch.zeros(P, 3))
            _call("r3dg_stage2_pack_features", P, _p(_dev(a["xyz"])), _p(_dev(a["viewmatrix"])), _p(z3), _p(z3), _p(_dev(torch.zeros(P))),
                  _p(d_so), feats.ptr(), packed.ptr())
            assert torch.equal(packed.cpu(), lsum.cpu()), tag + ": the two entry points disagree on the light sum"
        else:
            assert float(_slot_sum(lsum)) == 0.0
        if with_max:
            rows = torch.cat([pbr.cpu(), got], 1).abs()
            want = torch.stack([rows[b * 256:(b + 1) * 256].max() for b in range(nb)])
            assert torch.equal(amax.cpu(), want), tag + ": block_absmax is not the true maximum"
        else:
            assert amax.untouched()


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), 3.2e38])
def test_stage2_unpack_gradients_flags_a_non_finite_block(bad):
    """A NaN, a +inf and a value above 3.0e38 in one row: +inf for that row's block alone, the true maximum for the others."""
    P = 1000
    so, gfeat = _shading(P)
    gfeat = gfeat.clone()
    gfeat[300, 3] = bad
    nb = (P + 255) // 256
    pbr, dif, amax = Out(P, 3), Out(P, 3), Out(nb)
    _call("r3dg_stage2_unpack_gradients", P, _p(_dev(gfeat)), _p(_dev(so)), 0.37, pbr.ptr(), dif.ptr(), amax.ptr(), None)
    rows = torch.cat([pbr.cpu(), dif.cpu()], 1).abs()
    want = torch.stack([rows[b * 256:(b + 1) * 256].max() for b in range(nb)])
    want[1] = float("inf")
    assert torch.equal(amax.cpu(), want), (amax.cpu(), want)
    assert torch.equal(pbr.cpu().view(torch.int32), gfeat[:, 2:5].contiguous().view(torch.int32))


BWD_OUT = (("g_xyz", 3), ("g_scaling", 3), ("g_rotation", 4), ("g_opacity", 1), ("g_normal", 3), ("g_base", 3), ("g_rough", 1))


def _n_backward(a):
    return dict(g_xyz=28, g_scaling=gr.n_exp(a["scaling_raw"].numpy()) + 1, g_rotation=24, g_opacity=gr.n_sig(a["opacity_raw"].numpy()) + 4,
                g_normal=24, g_base=gr.n_sig(a["base_raw"].numpy()) + 6, g_rough=gr.n_sig(a["rough_raw"].numpy()) + 6)


def _env_case(He, We):
    n = He * We * 3
    raw = gc.env_texture(n, seed=7000 + 10 * He + We)
    g = torch.Generator().manual_seed(7100 + 10 * He + We)
    return raw, torch.nn.functional.softplus(raw), torch.randn(n, generator=g)


def _check_env(tag, He, We, raw, env, d_env, w_tv, g_raw, dl, tv, consume):
    refs = _refs(("env", He, We), gr.env_backward, He, We, raw, env, d_env, w_tv)
    n = He * We * 3
    _check(tag, "g_raw", g_raw.cpu(), refs, 12 + gr.n_sig(raw.numpy()))
    after = dl.cpu()
    assert (bool((after == 0).all()) if consume else torch.equal(after, d_env)), tag + ": dL_denv after the call"
    if tv is not None:
        _check(tag, "tv_sum", _slot_sum(tv), refs, _n_sum(8, 2, (n + 255) // 256))


ENV_SHAPES = [(1, 1), (1, 8), (8, 1), (3, 5), (16, 32)]


@pytest.mark.parametrize("with_tv", [False, True])
@pytest.mark.parametrize("consume", [0, 1])
@pytest.mark.parametrize("He,We", ENV_SHAPES)
def test_stage2_env_backward(He, We, consume, with_tv):
    """(1,1), (1,8), (8,1): a direction with no differences has weight 0 (inv_v / inv_h)."""
    raw, env, d_env = _env_case(He, We)
    n = He * We * 3
    g_raw, dl, tv = Out(n), Out(n), Out(SLOTS, init=0.0)
    dl.t.copy_(d_env)
    _call("r3dg_stage2_env_backward", He, We, _p(_dev(raw)), _p(_dev(env)), dl.ptr(), 0.37, g_raw.ptr(), tv.ptr() if with_tv else None,
          consume)
    _check_env("s2_env_backward %dx%d c%d tv%d" % (He, We, consume, with_tv), He, We, raw, env, d_env, 0.37, g_raw, dl,
               tv if with_tv else None, consume)
    if not with_tv:
        assert float(_slot_sum(tv)) == 0.0


def _backward_args(d, up, outs, frozen):
    geo = (lambda k: None) if frozen else (lambda k: outs[k].ptr())
    return [d["P"]] + [_p(d[k]) for k in RAW] + [_p(d["viewmatrix"]), _p(d["campos"])] + \
        [_p(up[k]) for k in ("dL_dfeatures", "dL_dbase", "dL_drough", "dL_dviewdirs", "dL_dscales", "dL_drot", "dL_dopacity", "dL_dmeans3D")] + \
        [geo(k) for k in ("g_xyz", "g_scaling", "g_rotation", "g_opacity", "g_normal")] + [outs["g_base"].ptr(), outs["g_rough"].ptr()]


@pytest.mark.parametrize("P", P_SIZES)
def test_stage2_activate_backward(P):
    """The plain entry point, the frozen-geometry call (d_g_xyz == NULL: only g_base / g_rough are written) and the folded one with a
    (3,5) texture job behind the Gaussians' workgroups."""
    a = _g_case(P)
    up = gc.upstream(P, seed=8000 + P)
    d, dup = _g_dev(a), {k: _dev(v) for k, v in up.items()}
    n = _n_backward(a)
    for entry, frozen in (("r3dg_stage2_activate_backward", False), ("r3dg_stage2_activate_backward", True),
                          ("r3dg_stage2_activate_backward_with", False)):
        refs = _refs(("bwd2", P, frozen), gr.activate_backward, a, up, stage2=True, frozen=frozen)
        outs = {k: Out(P, c) if c > 1 else Out(P) for k, c in BWD_OUT}
        extra = []
        if entry.endswith("_with"):
            He, We = 3, 5
            raw, env, d_env = _env_case(He, We)
            g_raw, dl, tv = Out(He * We * 3), Out(He * We * 3), Out(SLOTS, init=0.0)
            dl.t.copy_(d_env)
            extra = [He, We, _p(_dev(raw)), _p(_dev(env)), dl.ptr(), 0.37, g_raw.ptr(), tv.ptr(), 1]
        _call(entry, *_backward_args(d, dup, outs, frozen), *extra)
        tag = "%s P=%d frozen=%d" % (entry[len("r3dg_stage2_"):], P, frozen)
        for k, _ in BWD_OUT:
            if k in refs[0]:
                _check(tag, k, outs[k].cpu(), refs, n[k])
            else:
                assert outs[k].untouched(), tag + ": %s was written with frozen geometry" % k
        if extra:
            _check_env(tag, He, We, raw, env, d_env, 0.37, g_raw, dl, tv, 1)


@pytest.mark.parametrize("tv", [False, True])
@pytest.mark.parametrize("consume", [0, 1])
@pytest.mark.parametrize("He,We", ENV_SHAPES)
def test_stage2_activate_backward_with_texture_job(He, We, consume, tv):
    """The texture job of the folded launch at every texture shape, behind P = 65 Gaussians and alone (P = 0)."""
    raw, env, d_env = _env_case(He, We)
    n = He * We * 3
    for P in (65, 0):
        a = _g_case(65)
        up = gc.upstream(65, seed=8065)
        d, dup = dict(_g_dev(a), P=P), {k: _dev(v) for k, v in up.items()}
        outs = {k: Out(65, c) if c > 1 else Out(65) for k, c in BWD_OUT}
        g_raw, dl, tvs = Out(n), Out(n), Out(SLOTS, init=0.0)
        dl.t.copy_(d_env)
        _call("r3dg_stage2_activate_backward_with", *_backward_args(d, dup, outs, False), He, We, _p(_dev(raw)), _p(_dev(env)), dl.ptr(),
              0.37, g_raw.ptr(), tvs.ptr() if tv else None, consume)
        tag = "activate_backward_with P=%d %dx%d c%d tv%d" % (P, He, We, consume, tv)
        _check_env(tag, He, We, raw, env, d_env, 0.37, g_raw, dl, tvs if tv else None, consume)
        if P:
            refs = _refs(("bwd2", 65, False), gr.activate_backward, a, up, stage2=True, frozen=False)
            nb = _n_backward(a)
            for k, _ in BWD_OUT:
                _check(tag, k, outs[k].cpu(), refs, nb[k])
        else:
            assert all(o.untouched() for o in outs.values())


# ---- stage 1, per Gaussian ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", P_SIZES)
def test_stage1_pack_features(P):
    a = _g_case(P)
    normal = gr.stage2_activate(dict(a, base_raw=None))["normal"][0].contiguous()
    refs = _refs(("pack1", P), gr.stage1_pack_features, a["xyz"], a["viewmatrix"], normal)
    feats = Out(P, 5)
    _call("r3dg_stage1_pack_features", P, _p(_dev(a["xyz"])), _p(_dev(a["viewmatrix"])), _p(_dev(normal)), feats.ptr())
    got = feats.cpu()
    n = np.zeros((P, 5))
    n[:, 3], n[:, 4] = 5, 11
    _check("s1_pack_features P=%d" % P, "features", got, refs, n)
    assert torch.equal(got[:, :3], normal)


@pytest.mark.parametrize("P", P_SIZES)
def test_stage1_activate_backward(P):
    a = _g_case(P)
    up = gc.upstream(P, seed=9000 + P, stage2=False)
    refs = _refs(("bwd1", P), gr.activate_backward, a, up, stage2=False)
    d, dup = _g_dev(a), {k: _dev(v) for k, v in up.items()}
    outs = {k: Out(P, c) if c > 1 else Out(P) for k, c in BWD_OUT[:5]}
    _call("r3dg_stage1_activate_backward", P, *[_p(d[k]) for k in RAW[:5]], _p(d["viewmatrix"]),
          *[_p(dup[k]) for k in ("dL_dfeatures", "dL_dscales", "dL_drot", "dL_dopacity", "dL_dmeans3D")],
          *[outs[k].ptr() for k, _ in BWD_OUT[:5]])
    n = _n_backward(a)
    for k, _ in BWD_OUT[:5]:
        _check("s1_activate_backward P=%d" % P, k, outs[k].cpu(), refs, 8 if k == "g_xyz" else n[k])
