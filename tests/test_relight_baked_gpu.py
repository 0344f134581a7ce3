"""RelightRenderer(baked_visibility=True): the two kernels that turn the baked visibility SH into visibility on the ray set --
r3dg_visibility_sh_expand against visibility_bake.sh_visibility in torch, r3dg_shade_build_transport_baked against the existing
builders fed that torch visibility -- and the renderer they serve against a default renderer holding the expanded visibility,
under a fixed light, a turning light and the radiance cache.  Cases, environment maps (last column = first: the seam argument of
tests/test_relight_device_visibility_gpu.py's header applies here too), helpers and bounds are that file's.

Coefficients are 0.6 randn(P,16): on the ray sets of the cases with P >= 257 the value before the clamp falls below 0, inside
[0,1] and above 1 for about 23 % / 54 % / 23 % of the samples; every such case asserts >= 15 % in each region, so no branch of
the clamp can be forgotten unnoticed."""
import math

import pytest
import torch

from tests.helpers import CACHED_PATTERN, SPLIT_PATTERN, assert_frame_matches_glue, report, turning_light_frames
from tests.test_relight_device_visibility_gpu import (TWO_PI, _COLUMNS, _IMAGES, _builder_case, _compare_frames, _envmap,  # noqa: F401
                                                      _params, _rotation, _two_kernel_path)

pytestmark = pytest.mark.gpu
DEV = "cuda"
_SHAPES = [(1, 4, 8), (3, 5, 8), (257, 7, 16), (3000, 16, 32), (3000, 100, 32)]                # P, K, He
_BAKED = {}


def _coeffs(P, seed):
    return (0.6 * torch.randn(P, 16, generator=torch.Generator().manual_seed(seed))).to(DEV)


def _baked_case(P, K, M, He):
    """The builder case of the device-visibility tests (normals, ray table, both direction sets, incident light, map) with baked
    coefficients and their torch visibility on either direction set; computed once, never modified."""
    from relightable3dgaussian_amd.visibility_bake import sh_basis, sh_visibility
    if (P, K, M, He) not in _BAKED:
        c = dict(_builder_case(P, K, M, He))
        c["coeffs"] = _coeffs(P, 7000 + P + K)
        c["raw"] = (c["coeffs"][:, None, :] * sh_basis(c["dirs_trace"])).sum(-1) + 0.5               # before the clamp
        c["vis_trace"] = sh_visibility(c["coeffs"][:, None, :], c["dirs_trace"])[..., None].contiguous()
        c["vis_torch"] = sh_visibility(c["coeffs"][:, None, :], c["dirs_torch"])[..., None].contiguous()
        _BAKED[(P, K, M, He)] = c
    return _BAKED[(P, K, M, He)]


def _assert_all_clamp_regions(c, P):
    if P >= 257:
        raw = c["raw"]
        parts = [float((raw < 0).float().mean()), float(((raw >= 0) & (raw <= 1)).float().mean()), float((raw > 1).float().mean())]
        print("before the clamp: below 0 %.3f, inside %.3f, above 1 %.3f" % tuple(parts))
        assert min(parts) >= 0.15, parts


# ---- 1. the expansion against torch ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,K,He", _SHAPES)
def test_expand_matches_torch(P, K, He):
    """A = sh_visibility on the directions the trace kernel generates (trace_bundles(dirs_out=)), A' = the same on
    fibonacci_sphere_sampling's; D_ref = max|A - A'| is what direction rounding costs this formula between two existing
    evaluations.  The kernel must sit within max(2 D_ref, 1e-5) of A: the floor is the fp32 rounding of a 16-term sum of O(1)
    terms, 16 * 2^-23 * sum|v_i Y_i| <~ 1e-5 for these inputs."""
    from relightable3dgaussian_amd import shading_ops as so
    c = _baked_case(P, K, 16, He)
    _assert_all_clamp_regions(c, P)
    out = torch.full((P, K, 1), float("nan"), device=DEV)
    got = so.expand_visibility(c["normal"], c["coeffs"], c["zs"], out)
    assert got is out
    assert bool(torch.isfinite(out).all()) and float(out.min()) >= 0.0 and float(out.max()) <= 1.0
    fresh = so.expand_visibility(c["normal"], c["coeffs"][..., None], c["zs"])                    # [P,16,1] is taken too
    assert tuple(fresh.shape) == (P, K, 1) and torch.equal(fresh, out)
    d_ref = float((c["vis_trace"] - c["vis_torch"]).abs().max())
    err = float((out - c["vis_trace"]).abs().max())
    bound = max(2.0 * d_ref, 1e-5)
    print("P=%d K=%d  D_ref %.3e  kernel: max|got - A| %.3e  (bound %.3e)" % (P, K, d_ref, err, bound))
    assert err <= bound, (err, bound)


# ---- 2. the baked builder against the existing builders fed the torch visibility ----------------------------------------------------
@pytest.mark.parametrize("with_transform", [False, True])
@pytest.mark.parametrize("M", [16, 4])
@pytest.mark.parametrize("P,K,He", _SHAPES)
def test_baked_builder_matches_the_existing_builder(P, K, He, M, with_transform):
    """A = build_transport_rayset fed the torch visibility on the trace's directions; A' = build_taps + build_transport fed the
    torch visibility on fibonacci_sphere_sampling's.  Records and the 13 constants each within max(2 D_ref max|A|, 2e-5 max|A| +
    1e-6) of A, the bound of test_builder_matches_the_two_kernel_path by its argument.  M = 4: the visibility basis stays the
    full 16 while the local light sees its own 4 coefficients.  With the rotation: the visibility must not turn with the light."""
    from relightable3dgaussian_amd import shading_ops as so
    c = _baked_case(P, K, M, He)
    _assert_all_clamp_regions(c, P)
    tr = _rotation() if with_transform else None
    a_rec, a_consts = so.build_transport_rayset(c["normal"], c["incidents"], c["vis_trace"], c["zs"], TWO_PI, c["env"], tr)
    b_rec, b_consts = _two_kernel_path(dict(c, vis=c["vis_torch"]), c["dirs_torch"], tr)
    transport = torch.full((P, K, 3), float("nan"), device=DEV)
    consts = torch.full((P, 16), float("nan"), device=DEV)
    got_t, got_c = so.build_transport_baked(c["normal"], c["incidents"], c["coeffs"], c["zs"], TWO_PI, c["env"], tr, transport, consts)
    assert got_t is transport and got_c is consts                       # the buffers passed in are the ones returned
    assert bool(torch.isfinite(transport).all()) and bool(torch.isfinite(consts).all())
    assert bool((consts[:, 13:] == 0).all())
    fresh_t, fresh_c = so.build_transport_baked(c["normal"], c["incidents"], c["coeffs"], c["zs"], TWO_PI, c["env"], tr)
    assert tuple(fresh_t.shape) == (P, K, 3) and tuple(fresh_c.shape) == (P, 16)
    assert torch.equal(fresh_t, transport) and torch.equal(fresh_c, consts)
    for name, got, a, b in (("records", transport, a_rec, b_rec.reshape(P, K, 3)),
                            ("consts", consts[:, :13], a_consts[:, :13], b_consts[:, :13])):
        scale = float(a.abs().max())
        d_ref = float((a - b).abs().max()) / scale
        err = float((got - a).abs().max())
        bound = max(2.0 * d_ref * scale, 2e-5 * scale + 1e-6)
        print("P=%d K=%d M=%d He=%d transform=%s  %-7s D_ref %.3e  baked builder: max|got - A| / max|A| %.3e  (bound %.3e, max|A| %.3g)"
              % (P, K, M, He, with_transform, name, d_ref, err / scale, bound / scale, scale))
        assert err <= bound, (name, err, bound)
    mean_vis = so.expand_visibility(c["normal"], c["coeffs"], c["zs"]).mean(1)[:, 0]
    err = float((consts[:, 12] - mean_vis).abs().max())
    print("constant 12 against the row mean of the expansion: max|diff| %.3e" % err)
    assert err <= 1e-6


# ---- 3.-5. the renderer against a default renderer holding the expanded visibility -----------------------------------------------------
_PAIRS = {}


def _params_with_coeffs(P=3000, seed=5, single=False):
    p = _params(P=P, seed=seed)
    coeffs = _coeffs(P, 9000 + P)
    if single:
        p.visibility_sh = coeffs
    else:
        p.visibility_dc, p.visibility_rest = coeffs[:, :1, None].contiguous(), coeffs[:, 1:, None].contiguous()
    return p


def _pair(K):
    """b: the baked renderer; a: a default renderer (transport cache, regenerated directions) whose visibility is the expansion of
    b's coefficient snapshot and whose directions are update_visibility_device(want_dirs=True)'s for that snapshot."""
    from relightable3dgaussian_amd import relight, sampling, shading_ops as so
    from relightable3dgaussian_amd.train_step import update_visibility_device
    if K not in _PAIRS:
        env = _envmap(32)
        b = relight.RelightRenderer(_params_with_coeffs(), env, K, baked_visibility=True)
        assert b.tracer is None and b.incident_dirs is None and b.incident_areas is None and b.visibility is None
        assert b._uniform_area == TWO_PI and tuple(b.visibility_sh.shape) == (b.P, 16)
        zs = sampling.fibonacci_z_samples(K, DEV)[0].t().contiguous()
        vis = so.expand_visibility(b.a_normal, b.visibility_sh, zs)
        _, dirs, _ = update_visibility_device(b.xyz, b.a_scales, b.a_rot, b.a_opacity, b.a_normal, K, want_dirs=True)
        a = relight.RelightRenderer(_params(), env, K)
        a.visibility, a.incident_dirs = vis, dirs
        _PAIRS[K] = (a, b)
    return _PAIRS[K]


@pytest.mark.parametrize("K", [16, 100])
def test_baked_renderer_frames_equal_the_default_renderer_on_the_expanded_visibility(K):
    a, b = _pair(K)
    _compare_frames(a, b)
    assert b.visibility is None and b.tracer is None and b.incident_dirs is None and b.incident_areas is None
    assert b._taps.dtype == torch.float32 and tuple(b._taps.shape) == (b.P, K, 3)


@pytest.mark.parametrize("K", [20, 18])
def test_turning_light_on_a_baked_renderer(K):
    """The six-rotation sequence of test_turning_light_in_device_mode: the same cached / split pattern and every frame within
    that test's bounds of frame_reference(exact_activations=True).  K = 20: the split cache is built from a transient expansion
    and no [P,K] visibility (nor a direction tensor) is resident before frame_reference.  K = 18, outside
    shading_ops.split_supported: the general kernel runs on the materialised visibility and directions."""
    from relightable3dgaussian_amd import relight, shading_ops as so, synthetic as syn
    b = relight.RelightRenderer(_params_with_coeffs(P=3001, single=True), _envmap(32), K, baked_visibility=True)
    cam = syn.orbit_cameras(8, width=96, height=96)[2].to(DEV)
    bg = torch.zeros(3, device=DEV)

    def per_frame(tr, got):
        assert bool(torch.isfinite(b.shade_out).all())
    trs, cached, split, frames = turning_light_frames(b, cam, bg, per_frame)
    splits = so.split_supported(K, b.M, 32, 64, b._uniform_area)
    assert splits == (K == 20)
    assert cached == CACHED_PATTERN, cached
    assert split == (SPLIT_PATTERN if splits else [False] * 6), split
    assert b.tracer is None and b.incident_areas is None
    if splits:
        assert b.visibility is None and b.incident_dirs is None              # (checked before frame_reference, which fills both)
    else:
        assert tuple(b.visibility.shape) == (b.P, 18, 1) and tuple(b.incident_dirs.shape) == (b.P, 18, 3)
    for tr, got in zip(trs, frames):
        assert_frame_matches_glue(b, cam, bg, tr, got)
    assert tuple(b.visibility.shape) == (b.P, K, 1) and tuple(b.incident_dirs.shape) == (b.P, K, 3)


def test_radiance_cache_on_a_baked_renderer():
    from relightable3dgaussian_amd import relight
    a, b = _pair(16)
    c = relight.RelightRenderer(_params_with_coeffs(), _envmap(32), 16, cache="radiance", baked_visibility=True)
    assert c.visibility is None and c.incident_dirs is None and c.tracer is None
    _compare_frames(a, c)
    assert tuple(c.visibility.shape) == (c.P, 16, 1) and tuple(c.incident_dirs.shape) == (c.P, 16, 3)    # materialised, and kept
    held = c.visibility
    _compare_frames(a, c, cameras=(4,))
    assert c.visibility is held


def test_capture_map_and_base_color_scale_on_a_baked_renderer():
    """The "visibility" capture map and base_color_scale go through unchanged code: the map of the baked renderer equals the
    default renderer's on the expanded visibility, and the scale multiplies the albedo of both alike."""
    from relightable3dgaussian_amd import relight, synthetic as syn
    a, b = _pair(16)
    cam = syn.orbit_cameras(8, width=96, height=80)[4].to(DEV)
    bg = torch.zeros(3, device=DEV)
    fa, fb = a.frame(cam, bg, outputs=("visibility",)), b.frame(cam, bg, outputs=("visibility",))
    ok, msg = report("visibility", fb["visibility"], fa["visibility"], 2e-4, 1e-6)
    assert ok, msg
    assert float(fb["visibility"].max()) > 0.2
    scaled = relight.RelightRenderer(_params_with_coeffs(), _envmap(32), 16, baked_visibility=True, base_color_scale=[0.5, 1.0, 2.0])
    scaled.frame(cam, bg)
    assert torch.equal(scaled.a_base, b.a_base * torch.tensor([0.5, 1.0, 2.0], device=DEV))


# ---- 6. memory ----------------------------------------------------------------------------------------------------------------------
def test_baked_mode_never_holds_a_visibility_tensor():
    """Peak allocation growth over construction + one frame, P = 5000, K = 64, measured as
    test_device_mode_never_holds_the_direction_and_area_tensors measures it: the baked renderer must stay at least 4 P K bytes
    under device_visibility -- the [P,K] visibility alone is that much and never exists (nor do the tree and the trace records)."""
    from relightable3dgaussian_amd import relight, synthetic as syn
    P, K = 5000, 64
    params, env = _params_with_coeffs(P=P), _envmap(32)
    cam = syn.orbit_cameras(8, width=96, height=80)[1].to(DEV)
    bg = torch.zeros(3, device=DEV)
    modes = {"default": {}, "device_visibility": dict(device_visibility=True), "baked": dict(baked_visibility=True)}
    growth = {}
    for name in list(modes) * 2:                                        # (the first round also warms every allocation-free path)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        r = relight.RelightRenderer(params, env, K, **modes[name])
        r.frame(cam, bg)
        torch.cuda.synchronize()
        growth[name] = torch.cuda.max_memory_allocated() - base
        del r
    print("P=%d K=%d  peak growth over construction + one frame: default %d B, device_visibility %d B, baked %d B, 4 P K = %d B"
          % (P, K, growth["default"], growth["device_visibility"], growth["baked"], 4 * P * K))
    assert growth["baked"] <= growth["device_visibility"] - 4 * P * K, growth


# ---- 7. errors ----------------------------------------------------------------------------------------------------------------------
def test_errors():
    from relightable3dgaussian_amd import relight, shading_ops as so
    env = _envmap(8)
    with pytest.raises(RuntimeError):
        relight.RelightRenderer(_params(P=64), env, 8, baked_visibility=True)                                # no coefficients
    with pytest.raises(RuntimeError):
        relight.RelightRenderer(_params_with_coeffs(P=64), env, 8, baked_visibility=True, regenerate_dirs=False)
    with pytest.raises(RuntimeError):
        relight.RelightRenderer(_params_with_coeffs(P=64), env, 8, baked_visibility=True, device_visibility=True)
    P, K = 5, 4
    f = lambda *s: torch.rand(*s, device=DEV)
    n, zs, v = torch.nn.functional.normalize(f(P, 3) - 0.5, dim=-1), f(K, 3), f(P, 16) - 0.5
    so.build_transport_baked(n, f(P, 16, 3), v, zs, TWO_PI, env)
    so.expand_visibility(n, v, zs)
    for bad in (dict(normals=n.cpu()), dict(visibility_sh=v.cpu()), dict(visibility_sh=f(P, 9)), dict(visibility_sh=v.double()),
                dict(zsamples=zs.cpu())):
        kw = dict(dict(normals=n, visibility_sh=v, zsamples=zs), **bad)
        with pytest.raises(RuntimeError):
            so.expand_visibility(**kw)
        with pytest.raises(RuntimeError):
            so.build_transport_baked(kw["normals"], f(P, 16, 3), kw["visibility_sh"], kw["zsamples"], TWO_PI, env)
    with pytest.raises(RuntimeError):
        so.expand_visibility(n, v, zs, out=torch.empty(P, K + 1, 1, device=DEV))
    with pytest.raises(RuntimeError):
        so.build_transport_baked(n, f(P, 5, 3), v, zs, TWO_PI, env)                                            # M = 5: the library refuses
    with pytest.raises(RuntimeError):
        so.build_transport_baked(n, f(P, 16, 3), v, zs, TWO_PI, env, transport=torch.empty(P, K, 2, device=DEV))
