"""r3dg_rasterize_backward_split with sh_adam: the per-Gaussian geometry backward that applies the SH colour group's Adam itself
(csrc/rasterizer_preprocess_bwd.hip, preprocess_backward_kernel<true, true>) against the two launches it replaces in a whole
single-GPU iteration -- the same entry without it, then r3dg_adam_step on the one group.  Both kernels compile the same update
statements (csrc/adam_update.hpp) with the same flags, so parameters and moments are compared BIT FOR BIT, and so is every other
output of the backward.

The fixture: the tile pass in front of the kernel under test adds its per-wave sums with float atomics, so its result depends on
their order as soon as three non-zero terms meet in one element.  The upstream pixel gradients are therefore non-zero in two 8x8
pixel blocks only -- one wave of the tile kernel each (its lanes are an 8x8 block of its tile) -- so that an element receives at
most two non-zero terms (a + b == b + a) and otherwise zeros: the tile sums, and with them everything behind, are the same in
every run, which the test asserts before it compares the two paths.  The camera stands at the edge of the scene, so about half of the
Gaussians are culled (checked on the CPU oracle below: both kinds of row in one 256-row block); culled rows take part with a zero
gradient and their (non-zero) moments decay."""
import pytest
import torch

from tests.helpers import fwd_args, make_case

DEV = "cuda"
SIZES = (1, 255, 256, 257, 300)
W, H = 64, 48
LR, LR_TAIL, BETAS, EPS = 2.5e-3, 1.25e-4, (0.9, 0.999), 1e-15


def _case(P):
    return make_case(P=P, W=W, H=H, S=5, seed=60 + P, eye=(1.0, 0.3, 0.5), scale_log_mean=-2.5)


def _upstream(seed):
    """Pixel gradients (colour, opacity, depth, feature) that are zero outside two 8x8 blocks on the 8-pixel grid."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for c in (3, 1, 1, 5):
        t = torch.zeros(c, H, W)
        for y0, x0 in ((8, 16), (24, 40)):
            t[:, y0:y0 + 8, x0:x0 + 8] = torch.randn(c, 8, 8, generator=g)
        out.append(t)
    return out


@pytest.mark.parametrize("P", [p for p in SIZES if p > 1])
def test_fixture_has_culled_and_live_rows_in_one_block(P):
    """(CPU) the oracle's forward on the fixture: the first 256-row block holds culled AND live Gaussians, roughly half each."""
    from oracle import rasterizer as orc
    radii = torch.as_tensor(orc.rasterize_gaussians(*fwd_args(_case(P))[:-3])[9])[:256]
    live = int((radii > 0).sum())
    assert 0.2 * radii.numel() < live < 0.8 * radii.numel(), (live, radii.numel())


def _backward(case, a, out, ups, shs, **kw):
    from relightable3dgaussian_amd import rasterizer_ops
    return rasterizer_ops.rasterize_gaussians_backward(
        a[0], a[1], a[2], out[9], a[3], a[5], a[6], 1.0, a[8], a[9], a[10], a[11], a[12], ups[0], ups[1], ups[2], ups[3], shs,
        a[18], a[19], out[10], out[0], out[11], out[12], True, False, **kw)


GEOMETRY = {0: "dL_dmeans2D", 1: "dL_dcolors", 2: "dL_dopacity", 3: "dL_dmeans3D", 4: "dL_dfeatures", 5: "dL_dcov3D",
            7: "dL_dscales", 8: "dL_drotations"}


@pytest.mark.gpu
@pytest.mark.parametrize("P", SIZES)
def test_backward_with_the_sh_adam_inside_equals_backward_then_adam(P):
    """Steps 1, 2 and 3 (three different bias corrections) from the same parameters and non-zero moments, lr != lr_tail: after
    every step shs, exp_avg and exp_avg_sq are bitwise equal and so is every geometry output of the backward; the fused call
    does not touch its dL_dsh buffer.  With the skip flag set, parameters and moments are bitwise unchanged and the geometry
    outputs are still those of the unfused call."""
    from r3dg_rasterization import _C
    from relightable3dgaussian_amd import rasterizer_ops
    from relightable3dgaussian_amd.fused_adam import FusedAdam
    assert rasterizer_ops.rasterize_gaussians_backward.sh_adam_supported(16)
    case = _case(P)
    a = fwd_args(case, DEV)
    out = _C.rasterize_gaussians(*a)
    ups = [t.to(DEV) for t in _upstream(P)]
    live = out[9] > 0
    if P >= 255:
        assert 0 < int(live[:256].sum()) < min(P, 256), "the first block needs culled and live rows"
    g = torch.Generator().manual_seed(7 * P)
    m0 = (0.01 * torch.randn(P, 16, 3, generator=g)).to(DEV)
    v0 = ((0.01 * torch.randn(P, 16, 3, generator=g)) ** 2).to(DEV)

    def optimizer():
        opt = FusedAdam([dict(param=a[17].clone(), lr=LR, lr_tail=LR_TAIL, period=48, split=3)], betas=BETAS, eps=EPS)
        opt.groups[0]["exp_avg"].copy_(m0)
        opt.groups[0]["exp_avg_sq"].copy_(v0)
        return opt, opt.groups[0]
    opt_u, grp_u = optimizer()
    opt_f, grp_f = optimizer()
    sentinel = torch.full((P, 16, 3), 12345.0, device=DEV)
    for step in (1, 2, 3):
        bw_u = _backward(case, a, out, ups, grp_u["param"])
        again = _backward(case, a, out, ups, grp_u["param"])
        torch.cuda.synchronize()
        for i in range(9):
            assert torch.equal(bw_u[i], again[i]), "the fixture's tile sums differ between two runs (output %d)" % i
        if step == 1 and P > 1:
            assert int((bw_u[6][live].abs().amax((1, 2)) > 0).sum()) >= 2, "no live Gaussian carries an SH gradient"
            assert float(bw_u[6][~live].abs().max()) == 0.0
        opt_u.step([bw_u[6]])
        dsh = sentinel.clone()
        bw_f = _backward(case, a, out, ups, grp_f["param"], dL_dsh_out=dsh,
                         sh_adam=opt_f.fused_step_of(0, opt_f.step_count + 1, 1.0, None))
        opt_f.begin_step()
        torch.cuda.synchronize()
        assert opt_f.step_count == opt_u.step_count == step
        assert torch.equal(dsh, sentinel), "the fused backward wrote dL_dsh"
        for i, name in GEOMETRY.items():
            assert torch.equal(bw_f[i], bw_u[i]), "step %d: %s differs" % (step, name)
        for k in ("param", "exp_avg", "exp_avg_sq"):
            diff = (grp_f[k] - grp_u[k]).abs().max().item()
            assert torch.equal(grp_f[k], grp_u[k]), "step %d: %s differs by up to %.3e" % (step, k, diff)
        assert not torch.equal(grp_u["param"], a[17])
    # the two rates: the dc columns moved 20 times as far as the rest columns (same distribution of moments and gradients)
    moved = (grp_f["param"] - a[17]).abs().reshape(P, 48)
    if P > 1:
        assert float(moved[:, :3].median()) > 5 * float(moved[:, 3:].median()) > 0
    # a dropped view: no update, the geometry gradients as ever
    before = {k: grp_f[k].clone() for k in ("param", "exp_avg", "exp_avg_sq")}
    bw_u = _backward(case, a, out, ups, grp_f["param"])
    flag = torch.ones(1, device=DEV)
    bw_s = _backward(case, a, out, ups, grp_f["param"], sh_adam=opt_f.fused_step_of(0, 4, 1.0, flag))
    torch.cuda.synchronize()
    for k, t in before.items():
        assert torch.equal(grp_f[k], t), "a dropped view moved %s" % k
    for i, name in GEOMETRY.items():
        assert torch.equal(bw_s[i], bw_u[i]), "dropped view: %s differs" % name
