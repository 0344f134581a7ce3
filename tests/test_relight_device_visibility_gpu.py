"""RelightRenderer(device_visibility=True): the transport cache built straight from the ray set
(r3dg_shade_build_transport_rayset) against the two-kernel path it replaces, and the renderer it serves against the default
one -- with the trace taken out of the comparison -- under a fixed light, a turning light and the radiance cache.

Every environment map here is 3 rand^2 with its last column equal to its first: the lat-long lookup is discontinuous at
theta = +-pi (zero padding on either side) and sample 0 of every bundle is the normal itself, so Gaussians with n_y = 0, n_x < 0
put a sample exactly on that seam, where the sign of a zero -- which differs between units compiled under different
floating-point flags -- picks the side.  With equal end columns either side reads the same radiance; no sample is excluded."""
import math

import pytest
import torch

from tests.helpers import CACHED_PATTERN, SPLIT_PATTERN, assert_frame_matches_glue, report, turning_light_frames
from tests.test_visibility_refresh_gpu import _trace_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
TWO_PI = 2.0 * math.pi


def _envmap(He, seed=11):
    env = 3.0 * torch.rand(He, 2 * He, 3, generator=torch.Generator().manual_seed(seed)) ** 2
    env[:, -1] = env[:, 0]
    return env.to(DEV).contiguous()


def _rotation(seed=2):
    return torch.linalg.qr(torch.randn(3, 3, generator=torch.Generator().manual_seed(seed))).Q.to(DEV).contiguous()


# ---- 1. the builder against r3dg_shade_build_taps + r3dg_shade_build_transport -------------------------------------------------
_CASES = {}


def _builder_case(P, K, M, He):
    """Inputs of one case and the directions of its ray set from the two existing sources (never modified)."""
    from relightable3dgaussian_amd import bvh, bvh_ops, sampling
    if (P, K, M, He) not in _CASES:
        d = _trace_case(P, K, seed=P % 7)
        g = torch.Generator().manual_seed(1000 + P + K)
        tracer = bvh.RayTracer.from_device_leaves(d["xyz"], d["scales"], d["rotations"])
        records = bvh_ops.trace_records(tracer.tree, tracer.aabb, d["xyz"], tracer.covs_inv, d["opacity"][:, 0].contiguous(),
                                        d["normal"])
        zs = sampling.fibonacci_z_samples(K, DEV)[0].t().contiguous()
        dirs = torch.full((P, K, 3), float("nan"), device=DEV)
        bvh_ops.trace_bundles(records, tracer.tree, zs, torch.empty(P, K, device=DEV), 0, P, dirs_out=dirs)
        _CASES[(P, K, M, He)] = dict(
            normal=d["normal"], zs=zs, dirs_trace=dirs, dirs_torch=sampling.fibonacci_sphere_sampling(d["normal"], K)[0],
            incidents=(0.5 * torch.randn(P, M, 3, generator=g)).to(DEV), vis=torch.rand(P, K, 1, generator=g).to(DEV),
            env=_envmap(He, seed=11 + He))
    return _CASES[(P, K, M, He)]


def _two_kernel_path(c, dirs, tr):
    from relightable3dgaussian_amd import shading_ops as so
    He, We = c["env"].shape[0], c["env"].shape[1]
    rec = so.build_taps(dirs, He, We, tr, radiance_of=c["env"])
    consts = so.build_transport(c["normal"], c["incidents"], c["vis"], dirs, None, TWO_PI, rec)
    return rec.view(torch.float32), consts


@pytest.mark.parametrize("with_transform", [False, True])
@pytest.mark.parametrize("P,K,M,He", [(1, 4, 16, 8), (3, 5, 4, 8), (257, 7, 16, 16), (3000, 16, 16, 32), (3000, 100, 16, 32)])
def test_builder_matches_the_two_kernel_path(P, K, M, He, with_transform):
    """Reference A: build_taps(radiance_of=env) + build_transport(uniform_area = 2 pi) on the directions the trace kernel
    generated (bvh_ops.trace_bundles(dirs_out=)); A': the same on sampling.fibonacci_sphere_sampling's.  D_ref = max|A - A'| /
    max|A| is what direction rounding costs this formula on this scene between two existing evaluations; the new builder, a
    third evaluation under other floating-point flags, must sit within max(2 D_ref max|A|, 2e-5 max|A| + 1e-6) of A (the
    e_kernel <= 2 e_torch pattern of tests/test_visibility_refresh_gpu.py), records and constants each by their own D_ref.
    K = 5, 7, 100: not a multiple of 4 or of 64; the first normals of every case are +z, -z, 0.7 degrees off -z and unnormalised
    inputs (_trace_case).  Measured (profiles/r08_relight_setup.txt): D_ref 0 - 2.1e-5, the builder within 2.5e-6 in every case."""
    from relightable3dgaussian_amd import shading_ops as so
    c = _builder_case(P, K, M, He)
    tr = _rotation() if with_transform else None
    a_rec, a_consts = _two_kernel_path(c, c["dirs_trace"], tr)
    b_rec, b_consts = _two_kernel_path(c, c["dirs_torch"], tr)
    transport = torch.full((P, K, 3), float("nan"), device=DEV)
    consts = torch.full((P, 16), float("nan"), device=DEV)
    got_t, got_c = so.build_transport_rayset(c["normal"], c["incidents"], c["vis"], c["zs"], TWO_PI, c["env"], tr, transport, consts)
    assert got_t is transport and got_c is consts                       # the buffers passed in are reused
    assert bool(torch.isfinite(transport).all()) and bool(torch.isfinite(consts).all())      # every row written, finite
    assert bool((consts[:, 13:] == 0).all())
    fresh_t, fresh_c = so.build_transport_rayset(c["normal"], c["incidents"], c["vis"], c["zs"], TWO_PI, c["env"], tr)
    assert tuple(fresh_t.shape) == (P, K, 3) and tuple(fresh_c.shape) == (P, 16)
    assert torch.equal(fresh_t, transport) and torch.equal(fresh_c, consts)
    for name, got, a, b in (("records", transport, a_rec, b_rec), ("consts", consts[:, :13], a_consts[:, :13], b_consts[:, :13])):
        scale = float(a.abs().max())
        d_ref = float((a - b).abs().max()) / scale
        err = float((got - a).abs().max())
        bound = max(2.0 * d_ref * scale, 2e-5 * scale + 1e-6)
        print("P=%d K=%d M=%d He=%d transform=%s  %-7s D_ref %.3e  new builder: max|got - A| / max|A| %.3e  (bound %.3e, max|A| %.3g)"
              % (P, K, M, He, with_transform, name, d_ref, err / scale, bound / scale, scale))
        assert err <= bound, (name, err, bound)


# ---- 2.-4. the renderer, with the trace taken out of the comparison ---------------------------------------------------------------
_PAIRS = {}


def _params(P=3000, seed=5):
    from relightable3dgaussian_amd import synthetic as syn
    from relightable3dgaussian_amd.bench_core import GaussianParams
    return GaussianParams(syn.make_scene(P=P, seed=seed, stage2=True, scale_log_mean=-3.0), DEV, True)


def _pair(K):
    """b: the device-mode renderer; a: a default renderer (transport cache, regenerated directions) holding b's visibility and
    the directions update_visibility_device(want_dirs=True) returns for b's snapshot -- the same rays, kept as a tensor."""
    from relightable3dgaussian_amd import relight
    from relightable3dgaussian_amd.train_step import update_visibility_device
    if K not in _PAIRS:
        env = _envmap(32)
        b = relight.RelightRenderer(_params(), env, K, device_visibility=True)
        vis, dirs, _ = update_visibility_device(b.xyz, b.a_scales, b.a_rot, b.a_opacity, b.a_normal, K, want_dirs=True)
        a = relight.RelightRenderer(_params(), env, K)
        a.visibility, a.incident_dirs = b.visibility, dirs
        _PAIRS[K] = (a, b, vis, dirs)
    return _PAIRS[K]


# the bounds tests/test_relight_gpu.py::test_transport_cache_frames_equal_radiance_cache_frames holds between cached and
# regenerated directions: 2e-4 on the columns that carry the GGX lobe, 2e-5 on the view-independent ones, 4e-4 behind the sRGB curve
_COLUMNS = ((0, 3, "pbr", 2e-4), (3, 6, "diffuse_light", 2e-5), (6, 9, "specular", 2e-4), (9, 18, "lights", 2e-5), (18, 19, "vis", 2e-5))
_IMAGES = (("feature", 2e-4, 1e-6), ("pbr_env", 0.0, 4e-4))


def _compare_frames(a, b, cameras=(1, 4, 6)):
    from relightable3dgaussian_amd import synthetic as syn
    bg = torch.zeros(3, device=DEV)
    for i in cameras:
        cam = syn.orbit_cameras(8, width=96, height=80)[i].to(DEV)
        fa = a.frame(cam, bg)
        sa = a.shade_out.clone()
        fb = b.frame(cam, bg)
        assert fa["num_rendered"] == fb["num_rendered"]
        for c0, c1, name, tol in _COLUMNS:
            ok, msg = report(name, b.shade_out[:, c0:c1], sa[:, c0:c1], tol, 1e-6)
            assert ok, msg
        for k, rtol, atol in _IMAGES:
            ok, msg = report(k, fb[k], fa[k], rtol, atol)
            assert ok, msg


@pytest.mark.parametrize("K", [16, 100])
def test_device_renderer_frames_equal_the_default_renderer_on_the_same_rays(K):
    a, b, vis, dirs = _pair(K)
    assert torch.equal(b.visibility, vis)
    _compare_frames(a, b)
    assert b.incident_dirs is None and b.incident_areas is None
    assert b._taps.dtype == torch.float32 and tuple(b._taps.shape) == (b.P, K, 3)


@pytest.mark.parametrize("K", [20, 18])
def test_turning_light_in_device_mode(K):
    """The six-rotation sequence of tests/test_relight_gpu.py's turning-light test on a device-mode renderer: the same cached /
    split pattern and every frame within that test's bounds of frame_reference(exact_activations=True).  K = 20: no direction
    tensor appears.  K = 18, outside shading_ops.split_supported: the general kernel runs and materialises the directions."""
    from relightable3dgaussian_amd import relight, shading_ops as so, synthetic as syn
    b = relight.RelightRenderer(_params(P=3001), _envmap(32), K, device_visibility=True)
    cam = syn.orbit_cameras(8, width=96, height=96)[2].to(DEV)
    bg = torch.zeros(3, device=DEV)

    def per_frame(tr, got):
        assert bool(torch.isfinite(b.shade_out).all())
    trs, cached, split, frames = turning_light_frames(b, cam, bg, per_frame)
    splits = so.split_supported(K, b.M, 32, 64, b._uniform_area)
    assert splits == (K == 20)
    assert cached == CACHED_PATTERN, cached
    assert split == (SPLIT_PATTERN if splits else [False] * 6), split
    if splits:
        assert b.incident_dirs is None and b.incident_areas is None          # (checked before frame_reference, which fills it)
    else:
        assert b.incident_dirs is not None and tuple(b.incident_dirs.shape) == (b.P, 18, 3) and b.incident_areas is None
    for tr, got in zip(trs, frames):
        assert_frame_matches_glue(b, cam, bg, tr, got)
    assert tuple(b.incident_dirs.shape) == (b.P, K, 3)                      # frame_reference materialised them on the renderer


def test_radiance_cache_in_device_mode_holds_directions_from_construction():
    from relightable3dgaussian_amd import relight
    a, b, vis, dirs = _pair(16)
    c = relight.RelightRenderer(_params(), _envmap(32), 16, cache="radiance", device_visibility=True)
    assert tuple(c.incident_dirs.shape) == (c.P, 16, 3) and c.incident_areas is None
    assert torch.equal(c.visibility, vis) and torch.equal(c.incident_dirs, dirs)
    held = c.incident_dirs
    _compare_frames(a, c)
    assert c.incident_dirs is held


# ---- 5. memory ----------------------------------------------------------------------------------------------------------------------
def test_device_mode_never_holds_the_direction_and_area_tensors():
    """Peak allocation growth over construction + one frame, P = 5000, K = 64: device mode must stay at least 16 P K bytes under
    the default -- directions (12 B) and areas (4 B) per sample never exist; the 12-byte records are common to both."""
    from relightable3dgaussian_amd import relight, synthetic as syn
    P, K = 5000, 64
    params, env = _params(P=P), _envmap(32)
    cam = syn.orbit_cameras(8, width=96, height=80)[1].to(DEV)
    bg = torch.zeros(3, device=DEV)
    growth = {}
    for device_visibility in (False, True, False, True):               # (the first round also warms every allocation-free path)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        r = relight.RelightRenderer(params, env, K, device_visibility=device_visibility)
        r.frame(cam, bg)
        torch.cuda.synchronize()
        growth[device_visibility] = torch.cuda.max_memory_allocated() - base
        del r
    print("P=%d K=%d  peak growth over construction + one frame: default %d B, device_visibility %d B, saved %d B, 16 P K = %d B"
          % (P, K, growth[False], growth[True], growth[False] - growth[True], 16 * P * K))
    assert growth[True] <= growth[False] - 16 * P * K, growth


# ---- 6. errors ----------------------------------------------------------------------------------------------------------------------
def test_errors():
    from relightable3dgaussian_amd import relight, shading_ops as so
    with pytest.raises(RuntimeError):
        relight.RelightRenderer(_params(P=64), _envmap(8), 8, device_visibility=True, regenerate_dirs=False)
    P, K = 5, 4
    f = lambda *s: torch.rand(*s, device=DEV)
    n, vis, zs, env = torch.nn.functional.normalize(f(P, 3) - 0.5, dim=-1), f(P, K, 1), f(K, 3), _envmap(8)
    so.build_transport_rayset(n, f(P, 16, 3), vis, zs, TWO_PI, env)
    with pytest.raises(RuntimeError):
        so.build_transport_rayset(n.cpu(), f(P, 16, 3), vis, zs, TWO_PI, env)
    with pytest.raises(RuntimeError):
        so.build_transport_rayset(n, f(P, 5, 3), vis, zs, TWO_PI, env)
    with pytest.raises(RuntimeError):
        so.build_transport_rayset(n, f(P, 16, 3), vis, zs, TWO_PI, env, transport=torch.empty(P, K, 2, device=DEV))
