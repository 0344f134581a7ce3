"""The visibility bake on the device: the trace over hemisphere rays the kernel generates (r3dg_bvh_trace_hemisphere), the fit
kernel (r3dg_visibility_sh_fit), visibility_bake.VisibilityBaker / bake_visibility, against tests/golden/visibility_bake_reference.npz
(the reference's own Python on the CPU: see tests/test_visibility_bake_cpu.py for the fixture, the bound 4 x spread and the
knife-edge mask).

What is exact and what is not: every traced ray is bit-identical to the existing trace given the origin and direction the kernel
generated; the fit gives the same bits run to run and however its iterations are chunked; against the reference's float64 loop it
is held to the bound the reference's own float32 run sets."""
import numpy as np
import pytest
import torch

from tests.test_visibility_bake_cpu import fixture

pytestmark = pytest.mark.gpu
DEV = "cuda"
_SCENE = {}


def _scene(P=None):
    """The fixture's activated Gaussians (the first P of them) with tree and packed records, built once per P."""
    from relightable3dgaussian_amd import bvh, bvh_ops
    f = fixture()
    P = f["xyz"].shape[0] if P is None else P
    if P not in _SCENE:
        d = {k: f[k][:P].to(DEV).contiguous() for k in ("xyz", "scales", "rotations", "opacity", "normal")}
        tracer = bvh.RayTracer.from_device_leaves(d["xyz"], d["scales"], d["rotations"])
        op = d["opacity"][:, 0].contiguous()
        records = bvh_ops.trace_records(tracer.tree, tracer.aabb, d["xyz"], tracer.covs_inv, op, d["normal"])
        _SCENE[P] = dict(d=d, tracer=tracer, op=op, records=records)
    return _SCENE[P]


@pytest.mark.parametrize("P,T", [(333, 5), (2, 3), (1, 4)])
def test_hemisphere_trace_equals_the_array_trace_on_its_own_rays(P, T):
    """(333, 5): P no multiple of 64, a ray count that is no multiple of 8 (the per-XCD queue split) across several 256-ray blocks."""
    from relightable3dgaussian_amd import bvh_ops
    f, c = fixture(), _scene(P)
    d, tracer = c["d"], c["tracer"]
    raw = f["draws"][:T, :P].to(DEV).contiguous()
    vis = torch.full((T, P), -7.0, device=DEV)
    cnt = torch.full((T, P), -7, dtype=torch.int32, device=DEV)
    dirs = torch.full((T, P, 3), float("nan"), device=DEV)
    overflow = bvh_ops.trace_hemisphere(c["records"], tracer.tree, raw, vis, dirs, contributes=cnt)
    torch.cuda.synchronize()
    assert (vis != -7.0).all() and (cnt != -7).all() and torch.isfinite(dirs).all(), "a row was not written"
    # the existing trace over the same records, fed the directions the kernel wrote and the origins mean + d * 0.05
    res = tracer.trace_visibility(d["xyz"][None].expand_as(dirs), dirs, d["xyz"], tracer.covs_inv, c["op"], d["normal"])
    torch.cuda.synchronize()
    assert torch.equal(vis.view(torch.int32), res["visibility"][..., 0].view(torch.int32)), "visibility differs"
    assert torch.equal(cnt, res["contribute"][..., 0]), "hit counts differ"
    assert int(overflow) == int(bvh_ops.trace_bvh_opacity.last_overflow)
    # directions: F.normalize + flip of the draws (one square root and one division per unit vector: a few ulp)
    want = f["dirs"][:T, :P].to(DEV)
    worst = float((dirs - want).abs().max())
    dot = float((dirs * d["normal"][None]).sum(-1).min())
    print("P=%d T=%d  max |direction - normalize/flip| %.3e  min d.n %.3e  visible %.3f  overflow %d" % (
        P, T, worst, dot, float((vis > 0).float().mean()), int(overflow)))
    assert worst <= 1e-6 and dot >= -1e-6
    # two calls over two parts of the leaf slots fill the same buffers as one call; rows outside a range keep the sentinel
    h = P // 2
    vis2, dirs2 = torch.full((T, P), -7.0, device=DEV), torch.full((T, P, 3), -7.0, device=DEV)
    bvh_ops.trace_hemisphere(c["records"], tracer.tree, raw, vis2, dirs2, 0, h)
    torch.cuda.synchronize()
    outside = torch.ones(P, dtype=torch.bool, device=DEV)
    outside[tracer.tree[P - 1:, 3].long()[:h]] = False
    assert (vis2[:, outside] == -7.0).all() and (dirs2[:, outside] == -7.0).all(), "rows of leaves outside the range were written"
    assert (vis2[:, ~outside] != -7.0).all()
    bvh_ops.trace_hemisphere(c["records"], tracer.tree, raw, vis2, dirs2, h, P)
    torch.cuda.synchronize()
    assert torch.equal(vis2.view(torch.int32), vis.view(torch.int32)) and torch.equal(dirs2.view(torch.int32), dirs.view(torch.int32))


def test_hemisphere_trace_launches_nothing_for_nothing():
    from relightable3dgaussian_amd import _lib, bvh_ops
    L = _lib.lib()
    c = _scene(2)
    raw = fixture()["draws"][:3, :2].to(DEV).contiguous()
    vis, dirs = torch.full((3, 2), -7.0, device=DEV), torch.full((3, 2, 3), -7.0, device=DEV)
    bvh_ops.trace_hemisphere(c["records"], c["tracer"].tree, raw, vis, dirs, 1, 1)                 # empty range
    for lo, hi in ((-1, 1), (2, 1), (0, 3)):
        with pytest.raises(RuntimeError, match="bad leaf range"):
            bvh_ops.trace_hemisphere(c["records"], c["tracer"].tree, raw, vis, dirs, lo, hi)
    # P == 0 and T == 0 at the C ABI: status 0 without reading a pointer
    assert L.r3dg_bvh_trace_hemisphere(_lib.current_stream(), 0, 5, None, None, None, 0, 0, 0.05, None, None, None, None) == 0
    assert L.r3dg_bvh_trace_hemisphere(_lib.current_stream(), 2, 0, None, None, None, 0, 2, 0.05, None, None, None, None) == 0
    assert L.r3dg_visibility_sh_fit(_lib.current_stream(), 0, 5, 0, None, None, 0.01, 0.9, 0.999, 1e-8, None, None, None, None) == 0
    assert L.r3dg_visibility_sh_fit_loss_rows(0) == 0 and L.r3dg_visibility_sh_fit_loss_rows(333) >= 1
    torch.cuda.synchronize()
    assert (vis == -7.0).all() and (dirs == -7.0).all()


def _fit(dirs, vis, chunks, want_loss=True):
    """r3dg_visibility_sh_fit over dirs [T,P,3] / vis [T,P] (on the device) from zero state, in calls of the given sizes ->
    (coeffs, exp_avg, exp_avg_sq, losses[T])."""
    from relightable3dgaussian_amd import _lib
    L, f = _lib.lib(), fixture()
    T, P = vis.shape
    assert sum(chunks) == T
    state = [torch.zeros(P, 16, device=DEV) for _ in range(3)]
    rows = int(L.r3dg_visibility_sh_fit_loss_rows(P))
    losses = torch.empty(T, device=DEV)
    t0 = 0
    for n in chunks:
        part = torch.full((rows, n), float("nan"), device=DEV) if want_loss else None
        _lib.check(L.r3dg_visibility_sh_fit(_lib.current_stream(), P, n, t0, dirs[t0:t0 + n].contiguous().data_ptr(),
                                            vis[t0:t0 + n].contiguous().data_ptr(), f["lr"], float(f["betas"][0]),
                                            float(f["betas"][1]), f["eps"], *[s.data_ptr() for s in state],
                                            _lib.ptr(part)), "visibility_sh_fit")
        torch.cuda.synchronize()                                   # (the chunk's temporaries are alive until here)
        if want_loss:
            losses[t0:t0 + n] = part.sum(0) / P
        t0 += n
    return state[0], state[1], state[2], losses


def test_fit_kernel_against_the_reference_loop():
    """Fed the fixture's directions and visibility: the trace plays no part."""
    f = fixture()
    dirs, vis = f["dirs"].to(DEV), f["visibility"].to(DEV)
    T, P = vis.shape
    c, m, v, losses = _fit(dirs, vis, [32, 32, 32])
    again = _fit(dirs, vis, [32, 32, 32])
    other = _fit(dirs, vis, [20, 20, 20, 20, 16])
    whole = _fit(dirs, vis, [96], want_loss=False)
    for tag, s in (("a second run", again), ("chunks of 20", other), ("one call without the loss", whole)):
        for name, a, b in zip(("coeffs", "exp_avg", "exp_avg_sq"), (c, m, v), s):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "%s: %s differs" % (tag, name)
    assert torch.equal(losses.view(torch.int32), again[3].view(torch.int32)) and torch.equal(losses.view(torch.int32),
                                                                                              other[3].view(torch.int32))
    c1 = _fit(dirs[:1], vis[:1], [1])[0]
    e1 = float((c1.cpu().double() - f["coeffs_unmodified_1"].double()).abs().max())
    keep = f["keep"]
    err = {k: float((a.cpu().double() - f[k + "64"])[keep].abs().max()) for k, a in (("coeffs", c), ("exp_avg", m), ("exp_avg_sq", v))}
    rel = float(((losses.cpu().double() - f["losses64"]).abs() / f["losses64"]).max())
    print("one step vs the unmodified method %.3e; %d steps vs the float64 loop %s; bound %.3e (%d knife-edge left out); "
          "losses: max relative error %.3e (allowed %.3e)" % (e1, T, err, f["bound"], int((~keep).sum()), rel, P * 2.0 ** -23))
    assert torch.isfinite(c).all()
    assert e1 <= f["bound"]
    assert max(err.values()) <= f["bound"]
    assert rel <= P * 2.0 ** -23


def test_baker_end_to_end_against_the_reference_loop():
    """Trace and fit together over the fixture's draws.  Left out: a Gaussian one of whose rays differs from the fixture's (CPU
    oracle) visibility by more than 1e-5 -- it grazed a box or the 0.9 threshold, as in tests/test_visibility_refresh_gpu.py -- and
    the knife-edge ones; together at most 3 % of P."""
    from relightable3dgaussian_amd import bvh_ops, visibility_bake as vb
    f, c = fixture(), _scene()
    d = c["d"]
    T, P = f["visibility"].shape
    raw = f["draws"].to(DEV)
    baker = vb.VisibilityBaker(d["xyz"], d["scales"], d["rotations"], d["opacity"], d["normal"], lr=f["lr"],
                               betas=tuple(f["betas"].tolist()), eps=f["eps"], chunk=40)
    losses = baker.run(T, raw_dirs=raw)
    assert losses.shape == (T,) and losses.is_cuda and baker.steps == T
    vis, dirs = torch.empty(T, P, device=DEV), torch.empty(T, P, 3, device=DEV)
    bvh_ops.trace_hemisphere(baker.tracer._records, baker.tracer.tree, raw, vis, dirs)
    torch.cuda.synchronize()
    moved = ((vis.cpu() - f["visibility"]).abs() > 1e-5).any(0)
    left_out = moved | f["knife_edge"]
    dc, rest = baker.coefficients()
    assert dc.shape == (P, 1, 1) and rest.shape == (P, 15, 1)
    got = torch.cat((dc, rest), 1)[:, :, 0].cpu().double()
    err = float((got - f["coeffs64"])[~left_out].abs().max())
    print("end to end: %d Gaussians with a moved ray + %d knife-edge = %d of %d left out (cap %d); max |c - c64| %.3e (bound %.3e); "
          "loss %.4f -> %.4f" % (int(moved.sum()), int(f["knife_edge"].sum()), int(left_out.sum()), P, int(0.03 * P), err,
                                 f["bound"], float(losses[0]), float(losses[-1])))
    assert int(left_out.sum()) <= 0.03 * P
    assert err <= f["bound"]
    # the state travels: a second baker continues from the first one's state after 40 iterations, to the same bits
    a = vb.VisibilityBaker(d["xyz"], d["scales"], d["rotations"], d["opacity"], d["normal"], lr=f["lr"], chunk=64, tracer=baker.tracer)
    a.run(40, raw_dirs=raw[:40].contiguous())
    b = vb.VisibilityBaker(d["xyz"], d["scales"], d["rotations"], d["opacity"], d["normal"], lr=f["lr"], chunk=7, tracer=baker.tracer)
    b.load_state(a.state())
    b.run(T - 40, raw_dirs=raw[40:].contiguous())
    assert b.steps == T and torch.equal(b.coeffs.view(torch.int32), baker.coeffs.view(torch.int32))


def test_own_draws_bake_visibility_and_the_contract_op():
    import types
    from relightable3dgaussian_amd import shading_ops as so, visibility_bake as vb
    f, c = fixture(), _scene()
    d = c["d"]
    P = d["xyz"].shape[0]
    runs = []
    for _ in range(2):
        baker = vb.VisibilityBaker(d["xyz"], d["scales"], d["rotations"], d["opacity"], d["normal"], chunk=48)
        losses = baker.run(64, generator=torch.Generator(device=DEV).manual_seed(11))
        runs.append((baker.coeffs.clone(), losses))
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32)), "the same seed gives other coefficients"
    assert torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32))
    first, last = float(runs[0][1][0]), float(runs[0][1][-8:].mean())
    print("own draws: loss %.4f at the first iteration, %.4f over the last 8 of 64" % (first, last))
    assert last < first
    # bake_visibility fills both groups of a restored model in place (raw parameters: the fixture's)
    raw = {k: f["raw_" + k].to(DEV) for k in ("xyz", "normal", "scaling", "rotation", "opacity")}
    restored = types.SimpleNamespace(visibility_dc=torch.zeros(P, 1, 1, device=DEV), visibility_rest=torch.zeros(P, 15, 1, device=DEV),
                                     **raw)
    dc0, rest0 = restored.visibility_dc, restored.visibility_rest
    losses = vb.bake_visibility(restored, iterations=32, chunk=32, generator=torch.Generator(device=DEV).manual_seed(11))
    assert losses.shape == (32,) and restored.visibility_dc is dc0 and restored.visibility_rest is rest0
    assert float(dc0.abs().max()) > 0 and float(rest0.abs().max()) > 0 and torch.isfinite(rest0).all()
    as_dict = dict(raw)
    vb.bake_visibility(as_dict, iterations=32, chunk=32, generator=torch.Generator(device=DEV).manual_seed(11))
    assert torch.equal(as_dict["visibility_dc"], dc0) and torch.equal(as_dict["visibility_rest"], rest0)
    # the contract op takes the two groups joined, and saturated coefficients are visibility == 1 / == 0 to it
    g = torch.Generator().manual_seed(3)
    nrm = torch.nn.functional.normalize(torch.randn(P, 3, generator=g), dim=-1)
    inp = [torch.rand(P, 3, generator=g), 0.05 + 0.9 * torch.rand(P, 1, generator=g), torch.rand(P, 1, generator=g), nrm,
           torch.nn.functional.normalize(nrm + 0.8 * torch.randn(P, 3, generator=g), dim=-1), 0.3 * torch.randn(P, 16, 3, generator=g),
           0.3 * torch.randn(1, 16, 3, generator=g)]
    inp = [t.to(DEV) for t in inp]
    shade = lambda vis_shs: so.render_equation_forward(*inp, vis_shs, 24, False)
    baked = shade(torch.cat((dc0, rest0), 1))
    assert all(torch.isfinite(t).all() for t in baked)

    def constant(dc_value):
        v = torch.zeros(P, 16, 1, device=DEV)
        v[:, 0] = dc_value
        return v
    one, one_far = shade(constant(2.0)), shade(constant(40.0))            # 0.5 + C0 * 2 = 1.06: clamps to 1
    zero, zero_far = shade(constant(-2.0)), shade(constant(-40.0))
    torch.cuda.synchronize()
    assert torch.equal(one[0], one_far[0]) and torch.equal(one[2], one_far[2])
    assert torch.equal(zero[0], zero_far[0]) and torch.equal(zero[2], zero_far[2])
    assert not torch.equal(one[0], zero[0])
    # and what the op clamps is what the bake trained: sh_visibility of the same coefficients
    want = vb.sh_visibility(torch.cat((dc0, rest0), 1)[:, None, :, 0], baked[1])
    assert want.shape == (P, 24) and float(want.min()) >= 0.0 and float(want.max()) <= 1.0
    assert np.isfinite(float(want.mean()))
