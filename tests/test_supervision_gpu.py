"""csrc/supervision.hip on the GPU: the MVS depth / normal terms of stage 2, the depth smoothness and per-Gaussian terms of stage 1.

Each kernel against the reference's own calculate_loss (tests/golden/supervision_reference.npz, float64, written by
tests/golden/make_supervision_golden.py) and against the PyTorch restatement of train_step evaluated in float64 on generated
inputs; the fused iterations against their autograd counterparts.  Shapes: 29 x 37 images (narrower than a wave, neither side a
multiple of 8, five workgroups) and P = 3 * 256 + 37 Gaussians (four workgroups, a partial last wave); the fixture's P is 300.
Tolerances are those of tests/test_fused_step_gpu.py for r3dg_stage2_loss / r3dg_stage1_loss against PyTorch (loss 1e-5, gradients
2e-4 of the array's scale) and of tests/test_reference_pipeline_gpu.py for whole iterations (loss 1e-5, gradients 2e-3 of the scale
on every entry)."""
import os

import numpy as np
import pytest
import torch

from tests.helpers import report

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "supervision_reference.npz")
H, W = 29, 37
N = H * W
P_GEN = 256 * 3 + 37
W_DEPTH, W_NMVS = 0.7, 0.3                              # the fixture's lambdas
S1_LAMBDAS = dict(depth_smooth=0.4, point_entropy=0.6, orientation=0.8, scaling=0.5)


class _Chk:
    def __init__(self):
        self.msgs, self.ok = [], True

    def __call__(self, name, got, want, rtol, atol=0.0):
        want = torch.as_tensor(np.asarray(want.detach().cpu() if isinstance(want, torch.Tensor) else want)).reshape(got.shape)
        ok, msg = report(name, got, want, rtol, atol)
        self.msgs.append(msg)
        self.ok &= ok

    def done(self):
        print("\n".join(self.msgs))
        assert self.ok, "\n".join(self.msgs)


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def _fixture_case():
    f = np.load(GOLD)
    z = {k: f[k] for k in f.files}
    m = {k[4:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("map_")}
    q = {k[3:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("pt_")}
    return z, m, q


def _generated_maps(seed=23):
    """29 x 37 rasterizer outputs + supervision maps holding: n_contrib == 0, opacity < 1e-5, gt_depth == 0, mask and depth
    disagreeing both ways, rendered depth == gt_depth exactly (opacity a power of two: F / o and F * (1 / o) are one float)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)
    opacity = 0.05 + 0.95 * r(1, H, W)
    n_contrib = torch.randint(1, 9, (H, W), generator=g, dtype=torch.int32)
    n_contrib[r(H, W) < 0.1] = 0
    opacity[0, 7, 20:26], n_contrib[7, 20:26] = 4e-6, 3
    feat16 = torch.randn(16, H, W, generator=g) * opacity
    feat16[0] = (1.0 + 4.0 * r(H, W)) * opacity[0]
    gt_depth = 1.0 + 4.0 * r(1, H, W)
    gt_depth[r(1, H, W) < 0.3] = 0.0
    mask = (r(1, H, W) * 1.4 - 0.2).clamp(0, 1)                      # soft, zero on ~14 %
    mask[0, 2, 0:5], gt_depth[0, 2, 0:5] = 0.0, 3.0
    mask[0, 4, 0:5], gt_depth[0, 4, 0:5] = 0.6, 0.0
    for (y, x) in ((9, 9), (28, 36), (0, 0)):
        opacity[0, y, x], n_contrib[y, x], feat16[0, y, x], gt_depth[0, y, x], mask[0, y, x] = 0.25, 2, 0.75, 3.0, 1.0
    mvs = torch.nn.functional.normalize(torch.randn(3, H, W, generator=g), dim=0)
    gt = torch.nn.functional.avg_pool2d(r(3, H, W)[None], 3, 1, 1)[0].clamp(0, 1).contiguous()
    feat5 = torch.cat([feat16[5:8], feat16[0:1], feat16[1:2].abs()], 0)
    m = dict(opacity=opacity, n_contrib=n_contrib, feat16=feat16, feat5=feat5, gt_depth=gt_depth, mask=mask, mvs_normal=mvs, gt=gt)
    sel = (mask != 0) == (gt_depth > 0)
    dep = feat16[0:1] / opacity.clamp_min(1e-5) * (n_contrib > 0)[None]
    assert int((n_contrib == 0).sum()) > 0 and int((opacity < 1e-5).sum()) > 0 and int((gt_depth == 0).sum()) > 0
    assert int((~sel).sum()) >= 10 and int(((dep == gt_depth) & sel).sum()) >= 3
    return {k: v.contiguous() for k, v in m.items()}


def _generated_gaussians(P, seed=29):
    """weights == 0 and > 1, opacities at 1e-7 and 1 - 1e-7, normals facing away (n.d < 0), a Gaussian with three equal scales."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)
    weights = 2.5 * r(P, 1) ** 2
    weights[r(P, 1) < 0.2] = 0.0
    opac = 0.02 + 0.96 * r(P, 1)
    opac[0], opac[1], opac[P - 1], opac[P - 2] = 1e-7, 1.0 - 1e-7, 1e-7, 1.0 - 1e-7
    weights[0], weights[1], weights[P - 1], weights[P - 2], weights[2] = 0.7, 3.0, 1.8, 0.4, 0.0
    xyz = torch.randn(P, 3, generator=g)
    campos = torch.tensor([2.9, 1.1, 1.3])
    normal = torch.nn.functional.normalize(torch.randn(P, 3, generator=g), dim=-1)
    scales = torch.exp(-3.0 + 0.7 * torch.randn(P, 3, generator=g))
    scales[5] = 0.02
    q = dict(weights=weights, opac=opac, xyz=xyz, campos=campos, normal=normal, scales=scales)
    nd = (normal * torch.nn.functional.normalize(xyz - campos, dim=-1)).sum(-1)
    assert int((weights == 0).sum()) > 0 and int((weights > 1).sum()) > 0 and int((nd < 0).sum()) > 0 and int((nd > 0).sum()) > 0
    return {k: v.contiguous() for k, v in q.items()}


# ---- kernel drivers -----------------------------------------------------------------------------------------------------------
def _count(gt_depth, mask):
    from relightable3dgaussian_amd import _lib
    count = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().r3dg_supervision_count(_lib.current_stream(), W, H, gt_depth.data_ptr(), _lib.ptr(mask), count.data_ptr()),
               "supervision_count")
    return count


def _run_stage2(m, w_depth, w_nm, masked=True, accumulate=0, d_op=None, d_f=None, count=None):
    """-> (dL_dopacity, dL_dfeature [16,H,W], [depth sum, normal sum], count).  `w_nm` without its 1 / (3 N)."""
    from relightable3dgaussian_amd import _lib, fused_base
    d = {k: v.to(DEV) for k, v in m.items()}
    mask = d["mask"] if masked else None
    d_op = torch.zeros(1, H, W, device=DEV) if d_op is None else d_op.clone()
    d_f = torch.full((16, H, W), 7.0, device=DEV) if d_f is None else d_f.clone()
    sums = torch.zeros(2, fused_base.SUM_SLOTS, device=DEV)
    count = _count(d["gt_depth"], mask) if count is None else count
    _lib.check(_lib.lib().r3dg_stage2_supervision(
        _lib.current_stream(), W, H, d["opacity"].data_ptr(), d["feat16"].data_ptr(), d["n_contrib"].data_ptr(),
        d["gt_depth"].data_ptr(), d["mvs_normal"].data_ptr(), _lib.ptr(mask), count.data_ptr(), w_depth, w_nm / (3.0 * N),
        accumulate, d_op.data_ptr(), d_f.data_ptr(), sums.data_ptr()), "stage2_supervision")
    torch.cuda.synchronize()
    return d_op, d_f, sums.sum(1), count


def _run_depth_smooth(m, lam, d_op=None, d_f=None):
    from relightable3dgaussian_amd import _lib, fused_base
    d = {k: v.to(DEV) for k, v in m.items()}
    d_op = torch.zeros(1, H, W, device=DEV) if d_op is None else d_op.clone()
    d_f = torch.zeros(5, H, W, device=DEV) if d_f is None else d_f.clone()
    sums = torch.zeros(1, fused_base.SUM_SLOTS, device=DEV)
    edge = torch.empty(2, H, W, device=DEV)
    _lib.check(_lib.lib().r3dg_stage1_depth_smooth(
        _lib.current_stream(), W, H, d["opacity"].data_ptr(), d["feat5"].data_ptr(), d["n_contrib"].data_ptr(), d["gt"].data_ptr(),
        lam / (3.0 * N), edge.data_ptr(), d_op.data_ptr(), d_f.data_ptr(), sums.data_ptr()), "stage1_depth_smooth")
    torch.cuda.synchronize()
    return d_op, d_f, sums.sum(1)


def _run_gaussian_terms(q, w_pe, w_or, w_sc, base=None):
    """-> ({opac, normal (feature columns 0..2), scales, xyz: gradient}, the whole dL_dfeatures [P,5], the three sums).  Weights
    without their 1 / P."""
    from relightable3dgaussian_amd import _lib, fused_base
    d = {k: v.to(DEV) for k, v in q.items()}
    P = d["xyz"].shape[0]
    z = lambda *s: torch.zeros(*s, device=DEV)
    b = base or dict(opac=z(P, 1), feat=z(P, 5), scales=z(P, 3), xyz=z(P, 3))
    b = {k: v.clone() for k, v in b.items()}
    sums = torch.zeros(3, fused_base.SUM_SLOTS, device=DEV)
    _lib.check(_lib.lib().r3dg_stage1_gaussian_terms(
        _lib.current_stream(), P, d["weights"].data_ptr(), d["opac"].data_ptr(), d["normal"].data_ptr(), d["scales"].data_ptr(),
        d["xyz"].data_ptr(), d["campos"].data_ptr(), w_pe / P, w_or / P, w_sc / P, b["opac"].data_ptr(), b["feat"].data_ptr(),
        b["scales"].data_ptr(), b["xyz"].data_ptr(), sums.data_ptr()), "stage1_gaussian_terms")
    torch.cuda.synchronize()
    return dict(opac=b["opac"], normal=b["feat"][:, 0:3], scales=b["scales"], xyz=b["xyz"]), b["feat"], sums.sum(1)


# ---- float64 restatements (train_step's parity functions are dtype-agnostic) ---------------------------------------------------
def _ref_stage2(m, w_depth, w_nm, masked=True):
    from relightable3dgaussian_amd import train_step as ts
    d = lambda k: m[k].double()
    feature, opacity = d("feat16").requires_grad_(True), d("opacity").requires_grad_(True)
    feat = feature / opacity.clamp_min(1e-5) * (m["n_contrib"] > 0)[None]
    w = dict(ts.STAGE2_WEIGHTS, depth=w_depth, normal_mvs_depth=w_nm)
    loss = ts.stage2_supervision(feat, d("gt_depth"), d("mvs_normal"), d("mask") if masked else None, w)
    loss.backward()
    return float(loss), feature.grad, opacity.grad


def _ref_depth_smooth(m, lam):
    from relightable3dgaussian_amd import train_step as ts
    d = lambda k: m[k].double()
    feature, opacity = d("feat5").requires_grad_(True), d("opacity").requires_grad_(True)
    feat = feature / opacity.clamp_min(1e-5) * (m["n_contrib"] > 0)[None]
    loss = lam * ts.first_order_edge_aware_loss(feat[3:4], d("gt"))
    loss.backward()
    return float(loss), feature.grad, opacity.grad


def _ref_gaussian_terms(q, w_pe, w_or, w_sc):
    from relightable3dgaussian_amd import train_step as ts
    leaves = {k: q[k].double().requires_grad_(True) for k in ("opac", "normal", "scales", "xyz")}
    w = dict(ts.STAGE1_WEIGHTS, point_entropy=w_pe, orientation=w_or, scaling=w_sc, orientation_from_iter=0)
    # (iteration 1 of 4: the scaling schedule's factor is 1 - 0.99 = 0.01, undone here so that `w_sc` is the effective weight)
    w["scaling"] = w_sc / 0.01 if w_sc else 0.0
    loss = ts.stage1_gaussian_terms(w, q["weights"].double(), leaves["opac"], leaves["normal"], leaves["scales"], leaves["xyz"],
                                    q["campos"].double(), iteration=1, iterations=4)
    loss.backward()
    return float(loss), {k: (torch.zeros_like(v) if v.grad is None else v.grad) for k, v in leaves.items()}


# ---- case 1: every kernel against the fixture and against the float64 restatement ---------------------------------------------
@pytest.mark.parametrize("masked", [True, False], ids=["object_mask", "no_mask"])
def test_stage2_supervision_kernel_matches_the_reference_and_pytorch(masked):
    z, m_fix, _ = _fixture_case()
    chk = _Chk()
    # the fixture: each term alone (its gradients are stored per term) and both together
    tag = "depth" if masked else "depth_nomask"
    d_op, d_f, sums, count = _run_stage2(m_fix, W_DEPTH, 0.0, masked)
    n = int(count.item())
    assert n == int(z["count_masked" if masked else "count_nomask"])
    chk("fixture depth term", (W_DEPTH * sums[0:1] / n).cpu(), z["s2_%s_term" % tag].reshape(1), 1e-5)
    chk("fixture depth g_feature0", d_f[0], z["s2_%s_g_feature" % tag][0], 2e-4)
    chk("fixture depth g_opacity", d_op, z["s2_%s_g_opacity" % tag], 2e-4)
    assert bool((d_f[1:] == 7.0).all()) and float(sums[1]) == 0.0                  # nothing but map 0 is written
    if masked:
        d_op, d_f, sums, _ = _run_stage2(m_fix, 0.0, W_NMVS, masked)
        chk("fixture normal term", (W_NMVS * sums[1:2] / (3.0 * N)).cpu(), z["s2_normal_mvs_depth_term"].reshape(1), 1e-5)
        chk("fixture normal g_feature5..7", d_f[5:8], z["s2_normal_mvs_depth_g_feature"][5:8], 2e-4)
        chk("fixture normal g_opacity", d_op, z["s2_normal_mvs_depth_g_opacity"], 2e-4)
        assert bool((d_f[0:5] == 7.0).all()) and bool((d_f[8:] == 7.0).all()) and float(sums[0]) == 0.0
        d_op, d_f, sums, _ = _run_stage2(m_fix, W_DEPTH, W_NMVS, masked)
        both = lambda k: z["s2_depth_" + k] + z["s2_normal_mvs_depth_" + k]
        chk("fixture both g_feature", torch.cat([d_f[0:1], d_f[5:8]]), np.concatenate([both("g_feature")[0:1], both("g_feature")[5:8]]), 2e-4)
        chk("fixture both g_opacity", d_op, both("g_opacity"), 2e-4)
    # generated inputs against the float64 restatement
    m = _generated_maps()
    loss, g_f, g_op = _ref_stage2(m, W_DEPTH, W_NMVS, masked)
    d_op, d_f, sums, count = _run_stage2(m, W_DEPTH, W_NMVS, masked)
    value = W_DEPTH * sums[0:1] / int(count.item()) + W_NMVS * sums[1:2] / (3.0 * N)
    chk("pytorch loss", value.cpu(), np.array([loss]), 1e-5)
    chk("pytorch g_feature0", d_f[0], g_f[0], 2e-4)
    chk("pytorch g_feature5..7", d_f[5:8], g_f[5:8], 2e-4)
    chk("pytorch g_opacity", d_op, g_op, 2e-4)
    # sign(0) = 0: where the rendered depth equals the MVS depth exactly the depth term pulls on nothing
    dd = {k: v.to(DEV) for k, v in m.items()}
    dep = dd["feat16"][0:1] / dd["opacity"].clamp_min(1e-5) * (dd["n_contrib"] > 0)[None]
    d_op0, d_f0, _, _ = _run_stage2(m, W_DEPTH, 0.0, masked)
    eq = dep == dd["gt_depth"]
    assert int(eq.sum()) >= 3 and float(d_f0[0:1][eq].abs().max()) == 0.0 and float(d_op0[eq].abs().max()) == 0.0
    chk.done()


def test_stage1_depth_smooth_kernel_matches_the_reference_and_pytorch():
    z, m_fix, _ = _fixture_case()
    lam = S1_LAMBDAS["depth_smooth"]
    chk = _Chk()
    d_op, d_f, s = _run_depth_smooth(m_fix, lam)
    chk("fixture term", (lam * s / (3.0 * N)).cpu(), z["s1_depth_smooth_term"].reshape(1), 1e-5)
    chk("fixture g_feature3", d_f[3], z["s1_depth_smooth_g_feature"][3], 2e-4)
    chk("fixture g_opacity", d_op, z["s1_depth_smooth_g_opacity"], 2e-4)
    assert float(np.abs(np.delete(z["s1_depth_smooth_g_feature"], 3, 0)).max()) == 0.0
    m = _generated_maps(31)
    loss, g_f, g_op = _ref_depth_smooth(m, lam)
    base_op, base_f = torch.rand(1, H, W, device=DEV), torch.rand(5, H, W, device=DEV)
    d_op, d_f, s = _run_depth_smooth(m, lam, base_op, base_f)                     # ADDED to what r3dg_stage1_loss wrote
    chk("pytorch loss", (lam * s / (3.0 * N)).cpu(), np.array([loss]), 1e-5)
    chk("pytorch g_feature3", d_f[3] - base_f[3], g_f[3], 2e-4, 1e-7)             # (1e-7: rounding of the sum with the base, <= 1)
    chk("pytorch g_opacity", d_op - base_op, g_op, 2e-4, 1e-7)
    assert torch.equal(d_f[0:3], base_f[0:3]) and torch.equal(d_f[4], base_f[4])  # the other maps stay as they were
    chk.done()


@pytest.mark.parametrize("source", ["fixture", "generated"])
def test_stage1_gaussian_terms_kernel_matches_the_reference_and_pytorch(source):
    chk = _Chk()
    w_pe, w_or, w_sc = S1_LAMBDAS["point_entropy"], S1_LAMBDAS["orientation"], S1_LAMBDAS["scaling"]
    if source == "fixture":
        z, _, q = _fixture_case()
        P = q["xyz"].shape[0]
        from relightable3dgaussian_amd.train_step import scaling_weight
        w_sc_eff = scaling_weight(w_sc, int(z["iteration"]), int(z["iterations"]))
        for name, ws in (("point_entropy", (w_pe, 0.0, 0.0)), ("orientation", (0.0, w_or, 0.0)), ("scaling", (0.0, 0.0, w_sc_eff))):
            g, feat, s = _run_gaussian_terms(q, *ws)
            i = ("point_entropy", "orientation", "scaling").index(name)
            chk(name + " term", (ws[i] * s[i:i + 1] / P).cpu(), z["s1_%s_term" % name].reshape(1), 1e-5)
            assert float(s.sum()) == float(s[i])                                   # a term that is off adds nothing
            for k in ("opac", "normal", "scales", "xyz"):
                key = "s1_%s_g_%s" % (name, k)
                if key in z:
                    chk(key, g[k], z[key], 2e-4)
                else:
                    assert float(g[k].abs().max()) == 0.0, key
            assert float(feat[:, 3:].abs().max()) == 0.0
    else:
        q = _generated_gaussians(P_GEN)
        P = P_GEN
        loss, ref = _ref_gaussian_terms(q, w_pe, w_or, w_sc)
        g, feat, s = _run_gaussian_terms(q, w_pe, w_or, w_sc)
        chk("pytorch loss", ((w_pe * s[0:1] + w_or * s[1:2] + w_sc * s[2:3]) / P).cpu(), np.array([loss]), 1e-5)
        for k in ("opac", "normal", "scales", "xyz"):
            chk("pytorch g_" + k, g[k], ref[k], 2e-4)
        # ADDED to the rows the rasterizer backward wrote; feature columns 3, 4 are not touched
        base = dict(opac=torch.rand(P, 1, device=DEV), feat=torch.rand(P, 5, device=DEV), scales=torch.rand(P, 3, device=DEV),
                    xyz=torch.rand(P, 3, device=DEV))
        g2, feat2, _ = _run_gaussian_terms(q, w_pe, w_or, w_sc, base)
        assert torch.equal(feat2[:, 3:], base["feat"][:, 3:])
        for k, bk in (("opac", base["opac"]), ("normal", base["feat"][:, 0:3]), ("scales", base["scales"]), ("xyz", base["xyz"])):
            chk("added g_" + k, g2[k] - bk, g[k], 0.0, 2e-7)                       # (rounding of a sum of magnitude <= 2)
    chk.done()


# ---- case 2: the count ---------------------------------------------------------------------------------------------------------
def test_supervision_count_is_exact_and_an_empty_selection_gives_a_zero_depth_term():
    m = _generated_maps()
    for masked in (True, False):
        mask = m["mask"] if masked else torch.ones_like(m["mask"])
        want = int(((mask != 0) == (m["gt_depth"] > 0)).sum())
        got = int(_count(m["gt_depth"].to(DEV), m["mask"].to(DEV) if masked else None).item())
        assert got == want and 0 < want < N, (masked, got, want)
    # no pixel selected: depth everywhere, mask nowhere
    empty = dict(m, gt_depth=torch.full((1, H, W), 2.0), mask=torch.zeros(1, H, W))
    base_op = torch.rand(1, H, W, device=DEV)
    d_op, d_f, sums, count = _run_stage2(empty, W_DEPTH, 0.0, True, d_op=base_op)
    assert int(count.item()) == 0
    assert float(sums[0]) == 0.0 and float(d_f[0].abs().max()) == 0.0 and torch.equal(d_op, base_op)
    assert bool(torch.isfinite(d_f).all()) and bool(torch.isfinite(d_op).all())
    # both weights zero: the launcher returns without a launch (NULL buffers would fault otherwise) and writes nothing
    from relightable3dgaussian_amd import _lib
    assert _lib.lib().r3dg_stage2_supervision(_lib.current_stream(), W, H, None, None, None, None, None, None, None, 0.0, 0.0, 0,
                                              None, None, None) == 0


# ---- case 3: accumulation behind r3dg_stage2_loss / r3dg_stage2_smooth_fused ----------------------------------------------------
@pytest.mark.parametrize("normal,light_smooth,normal_mvs", [(a, b, c) for a in (0.0, 0.01) for b in (0.0, 1.0) for c in (0.0, W_NMVS)])
def test_normal_maps_and_opacity_gradient_accumulate_over_the_three_kernels(normal, light_smooth, normal_mvs):
    """Maps 5..7 = the sum of what r3dg_stage2_loss (normal term), r3dg_stage2_smooth_fused (light term) and
    r3dg_stage2_supervision (MVS normal term) contribute alone, dL_dopacity = the parent path's value + the new terms', for every
    combination -- with `accumulate_normal` chosen as FusedStage2Step._image_loss chooses it."""
    from relightable3dgaussian_amd import _lib, fused_base
    L, s = _lib.lib(), _lib.current_stream()
    m = _generated_maps(37)
    d = {k: v.to(DEV) for k, v in m.items()}
    g = torch.Generator().manual_seed(5)
    image, pseudo = torch.rand(3, H, W, generator=g).to(DEV), torch.nn.functional.normalize(torch.randn(3, H, W, generator=g), dim=0).to(DEV)
    bg = torch.tensor([1.0, 0.6, 0.3], device=DEV)

    def loss_kernel(w_normal):
        d_im, d_op, d_f = torch.empty(3, H, W, device=DEV), torch.empty(1, H, W, device=DEV), torch.zeros(16, H, W, device=DEV)
        sums = torch.zeros(10, fused_base.SUM_SLOTS, device=DEV)
        _lib.check(L.r3dg_stage2_loss(s, W, H, image.data_ptr(), d["opacity"].data_ptr(), d["feat16"].data_ptr(), pseudo.data_ptr(),
                                      d["n_contrib"].data_ptr(), d["gt"].data_ptr(), bg.data_ptr(), d["mask"].data_ptr(),
                                      0.8 / (3.0 * N), 0.8 / (3.0 * N), w_normal / (3.0 * N), None, None, d_im.data_ptr(),
                                      d_op.data_ptr(), d_f.data_ptr(), sums.data_ptr(), 1), "stage2_loss")
        return d_op, d_f

    def smooth(d_op, d_f, acc):
        sums = torch.zeros(3, fused_base.SUM_SLOTS, device=DEV)
        _lib.check(L.r3dg_stage2_smooth_fused(s, W, H, d["opacity"].data_ptr(), d["feat16"].data_ptr(), d["n_contrib"].data_ptr(),
                                              d["gt"].data_ptr(), d["mask"].data_ptr(), 0.0, 0.0, light_smooth / (3.0 * N), acc,
                                              d_op.data_ptr(), d_f.data_ptr(), sums.data_ptr()), "smooth_fused")

    # the chain of the iteration
    d_op, d_f = loss_kernel(normal)
    written = normal != 0.0
    if light_smooth != 0.0:
        smooth(d_op, d_f, 1 if written else 0)
        written = True
    parent_op = d_op.clone()
    d_op, d_f, _, _ = _run_stage2(m, W_DEPTH, normal_mvs, True, 1 if written else 0, d_op, d_f)
    # the separate contributions, each into buffers of its own
    a_op, a_f = loss_kernel(normal)
    parts = [a_f[5:8] if normal != 0.0 else torch.zeros(3, H, W, device=DEV)]
    if light_smooth != 0.0:
        b_op, b_f = torch.zeros(1, H, W, device=DEV), torch.zeros(16, H, W, device=DEV)
        smooth(b_op, b_f, 0)
        parts.append(b_f[5:8])
    c_op, c_f, _, _ = _run_stage2(m, W_DEPTH, normal_mvs, True, 0, torch.zeros(1, H, W, device=DEV), torch.zeros(16, H, W, device=DEV))
    if normal_mvs != 0.0:
        parts.append(c_f[5:8])
    want = sum(parts)
    chk = _Chk()
    # rounding of at most two float additions of terms of the arrays' scale (the kernels may fuse a product into the add)
    chk("maps 5..7", d_f[5:8], want, 3e-7, 1e-12)
    chk("map 0", d_f[0], c_f[0], 0.0, 0.0)
    chk("dL_dopacity", d_op, parent_op + c_op, 3e-7, 1e-12)
    chk("maps 2..4 untouched", d_f[2:5], a_f[2:5], 0.0, 0.0)
    chk.done()
    if normal == 0.0 and light_smooth == 0.0 and normal_mvs == 0.0:
        assert float(d_f[5:8].abs().max()) == 0.0


# ---- case 4: whole iterations against autograd ---------------------------------------------------------------------------------
def _scene(stage2, P=2000, seed=3):
    from relightable3dgaussian_amd import synthetic as syn
    from relightable3dgaussian_amd.bench_core import GaussianParams, render_stage1
    torch.manual_seed(1234)
    scene = syn.make_scene(P=P, seed=seed, stage2=stage2, scale_log_mean=-2.8)
    cam = syn.orbit_cameras(8, width=64, height=48)[1].to(DEV)
    bg = torch.tensor([1.0, 0.6, 0.3], device=DEV)
    params = GaussianParams(scene, DEV, stage2)
    with torch.no_grad():
        teacher = GaussianParams(syn.make_scene(P=P, seed=seed, stage2=False, scale_log_mean=-2.8), DEV, False)
        teacher.features_dc.add_(0.2 * torch.randn_like(teacher.features_dc))
        outs = render_stage1(teacher, cam, bg)
        gt = outs[2].clone()
        # an "MVS" depth map and normals: the teacher's rendered depth and normals, perturbed, with rejected pixels
        valid = outs[1] > 0
        feat = outs[5] / outs[3].clamp_min(1e-5) * valid
        g = torch.Generator().manual_seed(9)
        gt_depth = (feat[3:4] * (1.0 + 0.1 * torch.randn(1, 48, 64, generator=g).to(DEV))).clamp_min(0.0)
        gt_depth[(torch.rand(1, 48, 64, generator=g) < 0.2).to(DEV)] = 0.0
        mvs = torch.nn.functional.normalize(feat[0:3] + 0.2 * torch.randn(3, 48, 64, generator=g).to(DEV), dim=0).contiguous()
        yy, xx = torch.meshgrid(torch.linspace(-1, 1, 48), torch.linspace(-1, 1, 64), indexing="ij")
        mask = (1.3 - 1.5 * (xx * xx + yy * yy).sqrt()).clamp(0, 1)[None].contiguous().to(DEV)
    return scene, params, cam, bg, gt, gt_depth.contiguous(), mvs, mask


def test_fused_stage2_iteration_with_the_mvs_terms_matches_autograd():
    from relightable3dgaussian_amd.fused_step import FusedStage2Step
    from relightable3dgaussian_amd.train_step import Stage2Step
    scene, params, cam, bg, gt, gt_depth, mvs, mask = _scene(True)
    K = 16
    w = dict(depth=W_DEPTH, normal_mvs_depth=W_NMVS)
    ref = Stage2Step(params, scene, DEV, K, loss_weights=w)
    fused = FusedStage2Step(params, K, loss_weights=w)
    assert not fused.frozen_geometry
    fused.visibility, fused.incident_dirs, fused.incident_areas = ref.visibility, ref.incident_dirs, ref.incident_areas
    loss_ref, outs_ref = ref(cam, bg, gt, mask, gt_depth=gt_depth, mvs_normal=mvs)
    loss_ref.backward()
    outs = fused.forward_backward(cam, bg, gt, image_mask=mask, gt_depth=gt_depth, mvs_normal=mvs)
    torch.cuda.synchronize()
    assert outs[0] == outs_ref[0]
    assert fused.last_active_features == [0, 2, 3, 4, 5, 6, 7]
    chk = _Chk()
    chk("loss", fused.loss().reshape(1), loss_ref.detach().reshape(1), 1e-5)
    sel = ((mask != 0) == (gt_depth > 0))
    assert 0 < int(sel.sum()) == int(fused._sup_count_cur.item()) < 48 * 64
    # the new terms are a real share of the objective and of the gradients compared below
    terms = fused.sums.sum(1)[10:12].cpu().numpy() * np.array([W_DEPTH / int(sel.sum()), W_NMVS / (3.0 * 48 * 64)])
    assert terms.min() > 1e-3 * float(loss_ref), terms
    g = fused.grads
    for k in ("xyz", "normal", "scaling", "rotation", "opacity", "base_color", "roughness", "env"):
        chk("g_" + k, g[k], getattr(params, k).grad, 2e-3, 1e-9)
    chk("g_shs", g["shs"], torch.cat([params.features_dc.grad, params.features_rest.grad], 1), 2e-3, 1e-9)
    chk("g_incidents", g["incidents"], torch.cat([params.incidents_dc.grad, params.incidents_rest.grad], 1), 2e-3, 1e-9)
    chk.done()
    # a missing map is an error, not a silently dropped term
    with pytest.raises(RuntimeError):
        fused.forward_backward(cam, bg, gt, image_mask=mask)
    with pytest.raises(RuntimeError):
        fused.forward_backward(cam, bg, gt, image_mask=mask, gt_depth=gt_depth)


def test_fused_stage1_iteration_with_the_four_new_terms_matches_autograd():
    from relightable3dgaussian_amd.bench_core import render_stage1
    from relightable3dgaussian_amd.fused_step import FusedStage1Step
    from relightable3dgaussian_amd.train_step import stage1_loss
    # (the scene: one on which the two paths agree entry for entry with every new weight at 0 -- checked below.  On some seeds a
    # few Gaussians' borderline alpha >= 1/255 decisions differ between the two activation paths whatever the objective, which
    # is what the outlier allowance of tests/test_fused_step_gpu.py::test_fused_stage1_matches_autograd is for)
    scene, params, cam, bg, gt, _, _, mask = _scene(False, seed=5)
    it, its = 6000, 30_000
    outs_ref = render_stage1(params, cam, bg)
    stage1_loss(outs_ref, gt, mask, None, it).backward()
    parent = FusedStage1Step(params)
    parent.iteration = it
    parent.forward_backward(cam, bg, gt, mask)
    base = _Chk()
    for k in ("xyz", "normal", "scaling", "rotation", "opacity"):
        base("parent path g_" + k, parent.grads[k], getattr(params, k).grad, 2e-3, 1e-9)
        getattr(params, k).grad = None
    params.features_dc.grad = params.features_rest.grad = None
    base.done()
    outs_ref = render_stage1(params, cam, bg)
    gaussians = dict(opacity=params.get_opacity(), normal=params.get_normal(), scales=params.get_scaling(), xyz=params.xyz,
                     campos=cam.camera_center)
    loss_ref = stage1_loss(outs_ref, gt, mask, S1_LAMBDAS, it, gaussians=gaussians, iterations=its)
    plain = stage1_loss(outs_ref, gt, mask, None, it)
    loss_ref.backward()
    fused = FusedStage1Step(params, loss_weights=S1_LAMBDAS, iterations=its)
    fused.iteration = it
    outs = fused.forward_backward(cam, bg, gt, mask)
    torch.cuda.synchronize()
    assert outs[0] == outs_ref[0]
    assert float(loss_ref - plain) > 1e-3 * float(plain)                           # the new terms are a real share of the objective
    chk = _Chk()
    chk("loss", fused.loss().reshape(1), loss_ref.detach().reshape(1), 1e-5)
    g = fused.grads
    for k in ("xyz", "normal", "scaling", "rotation", "opacity"):
        chk("g_" + k, g[k], getattr(params, k).grad, 2e-3, 1e-9)
    chk("g_shs", g["shs"], torch.cat([params.features_dc.grad, params.features_rest.grad], 1), 2e-3, 1e-9)
    chk.done()
    # before the gate opens the orientation term is off in both (render.py:191)
    fused.iteration = 5000
    fused.forward_backward(cam, bg, gt, mask)
    off = stage1_loss(outs_ref, gt, mask, S1_LAMBDAS, 5000, gaussians=gaussians, iterations=its)
    ok, msg = report("loss at the gate", fused.loss().reshape(1), off.detach().reshape(1), 1e-5, 0.0)
    assert ok, msg


# ---- case 5: no behaviour change with the weights at zero -----------------------------------------------------------------------
def _same(name, grad_a, grad_b, param_a, param_b, msgs):
    """A gradient group of two steps: bit for bit, or -- where float atomics order its sums (the rasterizer backward's
    per-Gaussian records, the shading backward), so that two runs of ONE step object differ as well -- the bound README.md states
    for two runs of one build: the group's parameters after the iteration's Adam update within 1e-7 of their scale."""
    if torch.equal(grad_a, grad_b):
        msgs.append("%-16s gradient bit for bit" % name)
        return True
    gd = float((grad_a - grad_b).abs().max()) / max(float(grad_b.abs().max()), 1e-30)
    pd = float((param_a - param_b).abs().max()) / max(float(param_b.abs().max()), 1e-30)
    msgs.append("%-16s gradient differs by %.2e of its scale (float atomics); parameters after Adam by %.2e of theirs" % (name, gd, pd))
    return pd <= 1e-7


def test_zero_weights_change_nothing():
    """A step built with the new keys at 0 (with and without the maps) against one built without them: the same launches (the
    recording-library test of tests/test_supervision_cpu.py pins that), so the forward outputs and loss() agree bit for bit and
    every gradient group either bit for bit or within README's run-to-run bound (_same)."""
    from relightable3dgaussian_amd.fused_step import FusedStage1Step, FusedStage2Step
    scene, params, cam, bg, gt, gt_depth, mvs, mask = _scene(True)
    msgs, ok = [], True
    runs = []
    for weights, maps in ((None, {}), (dict(depth=0.0, normal_mvs_depth=0.0), dict(gt_depth=gt_depth, mvs_normal=mvs)),
                          (dict(depth=0.0, normal_mvs_depth=0.0), {})):
        step = FusedStage2Step(params, 16, loss_weights=weights, lr=1e-3)
        if runs:
            step.visibility, step.incident_dirs, step.incident_areas = runs[0][0].visibility, runs[0][0].incident_dirs, runs[0][0].incident_areas
        assert step.sums.shape[0] == 10
        outs = step.forward_backward(cam, bg, gt, image_mask=mask, **maps)
        torch.cuda.synchronize()
        grads = {k: v.clone() for k, v in step.grads.items()}
        loss = step.loss().clone()
        step.optimizer_step()
        torch.cuda.synchronize()
        runs.append((step, outs, grads, loss))
    base = runs[0]
    for i, (step, outs, grads, loss) in enumerate(runs[1:], 1):
        assert torch.equal(outs[2], base[1][2]) and torch.equal(outs[5], base[1][5]) and torch.equal(loss, base[3])
        for k in grads:
            ok &= _same("s2[%d] %s" % (i, k), grads[k], base[2][k], getattr(step, k), getattr(base[0], k), msgs)
    scene, params, cam, bg, gt, _, _, mask = _scene(False, seed=4)
    runs = []
    for weights in (None, dict(depth_smooth=0.0, point_entropy=0.0, orientation=0.0, scaling=0.0)):
        step = FusedStage1Step(params, loss_weights=weights, **({} if weights is None else dict(iterations=1000)))
        step.iteration = 6000
        assert step.sums.shape[0] == 6
        outs = step.forward_backward(cam, bg, gt, mask)
        torch.cuda.synchronize()
        grads, loss = {k: v.clone() for k, v in step.grads.items()}, step.loss().clone()
        step.optimizer_step()
        torch.cuda.synchronize()
        runs.append((outs, grads, loss, step))
    assert torch.equal(runs[1][0][2], runs[0][0][2]) and torch.equal(runs[1][2], runs[0][2])
    for k in runs[0][1]:
        ok &= _same("s1 %s" % k, runs[1][1][k], runs[0][1][k], getattr(runs[1][3], k), getattr(runs[0][3], k), msgs)
    print("\n".join(msgs))
    assert ok, "\n".join(msgs)


# ---- case 6: two runs on the same inputs ------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_integers_and_the_same_sums_within_rounding():
    """Built: gradients are per-thread read-modify-writes (no atomics: identical bits), the count is integer atomics (identical),
    the float sums are one atomic add per workgroup / wave into R3DG_SUM_SLOTS slots, summed by the host in slot order -- not a
    fixed order once a slot takes more than one add, so the sums are compared within rounding: 64 eps of the sum of magnitudes
    (every term here is non-negative: of the sum itself), a slot never takes more adds than that at these sizes."""
    m, q = _generated_maps(), _generated_gaussians(P_GEN)
    a = _run_stage2(m, W_DEPTH, W_NMVS)
    b = _run_stage2(m, W_DEPTH, W_NMVS)
    assert int(a[3].item()) == int(b[3].item())
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert bool(((a[2] - b[2]).abs() <= 64 * 1.2e-7 * a[2].abs()).all()), (a[2], b[2])
    ga, fa, sa = _run_gaussian_terms(q, 0.6, 0.8, 0.5)
    gb, fb, sb = _run_gaussian_terms(q, 0.6, 0.8, 0.5)
    assert torch.equal(fa, fb) and all(torch.equal(ga[k], gb[k]) for k in ga)
    assert bool(((sa - sb).abs() <= 64 * 1.2e-7 * sa.abs()).all()), (sa, sb)
