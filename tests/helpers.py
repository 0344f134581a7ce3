"""Shared helpers for the parity tests (oracle <-> HIP)."""
import numpy as np
import torch

from relightable3dgaussian_amd import synthetic as syn


def to_np(t):
    if isinstance(t, torch.Tensor):
        return t.detach().cpu().numpy()
    return np.asarray(t)


def report(name, got, ref, rtol, atol):
    """Returns (ok, message): |got-ref| <= atol + rtol*max|ref| elementwise (scale-relative tolerance: sums of
    float atomics are compared against the double-accumulated oracle, so the natural scale is the array's)."""
    got = to_np(got).astype(np.float64)
    ref = to_np(ref).astype(np.float64)
    assert got.shape == ref.shape, "%s: shape %s vs %s" % (name, got.shape, ref.shape)
    if ref.size == 0:
        return True, "%s: empty" % name
    scale = np.abs(ref).max()
    err = np.abs(got - ref)
    bound = atol + rtol * scale
    bad = err > bound
    msg = "%-14s max|err| %.3e  scale %.3e  rel %.2e  bad %d/%d (bound %.2e)" % (
        name, err.max(), scale, err.max() / max(scale, 1e-30), bad.sum(), ref.size, bound)
    if not np.isfinite(got).all():
        return False, msg + "  NON-FINITE values in result"
    return not bad.any(), msg


U32 = 2.0 ** -24          # one fp32 rounding (half an ulp, relative)

# The constants in front of the two element bounds (tests/test_gradient_bounds_cpu.py measures both and asserts that they
# are 4 x its measured maxima, rounded up):
#   tile pass:            |err| <= TILE_BOUND_C * 2^-24 * E      (E: oracle.rasterizer ... want_bounds)
#   per-Gaussian stage:   |err| <= STAGE_BOUND_C * sigma          (sigma: oracle.rasterizer.per_gaussian_sigma)
TILE_BOUND_C = 4.0
STAGE_BOUND_C = 8300.0


def report_elementwise(name, got, ref, bound):
    """Returns (ok, message): every element within ITS OWN bound, |got - ref| <= bound (an array of ref's shape), and finite.
    The message names the largest err / bound, where it occurs, and the median ratio (over elements with a non-zero bound;
    an element whose bound is zero has to be exact)."""
    got = to_np(got).astype(np.float64)
    ref = to_np(ref).astype(np.float64)
    bound = np.broadcast_to(np.asarray(bound, np.float64), ref.shape)
    assert got.shape == ref.shape, "%s: shape %s vs %s" % (name, got.shape, ref.shape)
    if ref.size == 0:
        return True, "%s: empty" % name
    finite = np.isfinite(got).all()
    err = np.abs(np.where(np.isfinite(got), got, 0.0) - ref)
    bad = err > bound
    nz = bound > 0
    ratio = np.zeros_like(err)
    ratio[nz] = err[nz] / bound[nz]
    ratio[~nz & (err > 0)] = np.inf
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    msg = "%-14s max err/bound %.3e at %s (err %.3e, ref %.3e)  median %.2e  bad %d/%d  zero-bound elements %d" % (
        name, ratio[at], tuple(int(i) for i in at), err[at], ref[at], float(np.median(ratio[nz])) if nz.any() else 0.0,
        bad.sum(), ref.size, (~nz).sum())
    if not finite:
        return False, msg + "  NON-FINITE values in result"
    return not bad.any(), msg


def make_case(P=3000, W=128, H=128, S=5, seed=1, scale_log_mean=-3.0, eye=(3.2, 1.0, 1.5), use_colors=False,
              use_cov=False, bg=(1.0, 0.5, 0.2), sh_degree=3, scale_modifier=1.0, sh_shift=0.0, fovy_scale=1.0,
              principal_point=None):
    """A seeded scene + camera + feature block; everything as CPU fp32 torch tensors (dict).
    `sh_shift` is added to every DC coefficient (negative: more colour channels clamp); `fovy_scale` multiplies tan(fovy/2)
    (focal_x != focal_y); `principal_point` = (cx / W, cy / H) moves the principal point off the centre."""
    sc = syn.make_scene(P=P, seed=seed, scale_log_mean=scale_log_mean)
    cam = syn.look_at_camera(eye, width=W, height=H)
    if fovy_scale != 1.0:
        import math
        fovy = 2 * math.atan(cam.tanfovy * fovy_scale)
        proj = syn._projection(0.01, 100.0, cam.FoVx, fovy).transpose(0, 1)
        full = (cam.world_view_transform.unsqueeze(0).bmm(proj.unsqueeze(0))).squeeze(0).contiguous()
        cam = cam._replace(FoVy=fovy, tanfovy=math.tan(fovy * 0.5), full_proj_transform=full)
    if principal_point is not None:
        cam = cam._replace(cx=principal_point[0] * W, cy=principal_point[1] * H)
    if sh_shift != 0.0:
        sc["shs"] = sc["shs"].clone()
        sc["shs"][:, 0] += sh_shift
    g = torch.Generator().manual_seed(seed + 100)
    feat = torch.rand(P, S, generator=g) if S > 0 else torch.zeros(P, 0)
    case = dict(P=P, W=W, H=H, S=S, bg=torch.tensor(bg, dtype=torch.float32), means3D=sc["xyz"], features=feat,
                opacity=sc["opacity"], scales=sc["scales"], rotations=sc["rotations"], shs=sc["shs"],
                degree=sh_degree, cam=cam, colors=None, cov3D=None, scale_modifier=scale_modifier)
    if use_colors:
        case["colors"] = torch.rand(P, 3, generator=g)
        case["shs"] = None
    if use_cov:
        from oracle import torch_rasterizer as trz
        case["cov3D"] = trz.cov3d_from_scale_rot(sc["scales"], 1.0, sc["rotations"]).contiguous()
        case["scales"] = None
        case["rotations"] = None
    return case


def case_from_scene(sc, W=128, H=128, S=5, seed=1, eye=(3.2, 1.0, 1.5), bg=(1.0, 0.5, 0.2), sh_degree=3):
    """make_case for a GIVEN scene (synthetic.make_scene's format; e.g. relightable3dgaussian_amd.trained_scene)."""
    P = sc["xyz"].shape[0]
    g = torch.Generator().manual_seed(seed + 100)
    feat = torch.rand(P, S, generator=g) if S > 0 else torch.zeros(P, 0)
    cpu = lambda t: t.detach().cpu().contiguous()
    return dict(P=P, W=W, H=H, S=S, bg=torch.tensor(bg, dtype=torch.float32), means3D=cpu(sc["xyz"]), features=feat,
                opacity=cpu(sc["opacity"]), scales=cpu(sc["scales"]), rotations=cpu(sc["rotations"]), shs=cpu(sc["shs"]),
                degree=sh_degree, cam=syn.look_at_camera(eye, width=W, height=H), colors=None, cov3D=None)


def fwd_args(case, device=None, debug=False):
    """Positional args of `_C.rasterize_gaussians` for a case (optionals as empty CPU tensors, like the reference)."""
    cam = case["cam"]
    empty = torch.Tensor([])

    def dv(t):
        if t is None:
            return empty
        return t.to(device) if device is not None else t
    return (dv(case["bg"]), dv(case["means3D"]), dv(case["features"]), dv(case["colors"]), dv(case["opacity"]),
            dv(case["scales"]), dv(case["rotations"]), case.get("scale_modifier", 1.0), dv(case["cov3D"]),
            dv(cam.world_view_transform),
            dv(cam.full_proj_transform), cam.tanfovx, cam.tanfovy, cam.cx, cam.cy, case["H"], case["W"],
            dv(case["shs"]), case["degree"], dv(cam.camera_center), False, True, debug)


# ---- the element-wise gradient bounds (tests/test_gradient_bounds_cpu.py, tests/test_rasterizer_gpu.py) ----------------------
# Cases added for the element-wise checks: what the parity cases above leave out of the argument space.
ELEMENTWISE_CASES = {
    "scale_mod_0.6": dict(S=5, seed=41, scale_modifier=0.6),
    "scale_mod_1.7": dict(S=5, seed=42, scale_modifier=1.7),
    "scale_mod_1.7_cov": dict(S=4, seed=43, use_cov=True, scale_modifier=1.7),
    "sh_degree_0": dict(S=3, seed=44, sh_degree=0),
    "sh_degree_1": dict(S=3, seed=45, sh_degree=1),
    "sh_degree_2": dict(S=3, seed=46, sh_degree=2),
    "camera_inside": dict(S=5, seed=47, eye=(0.2, 0.1, 0.0)),
    "black_bg": dict(S=5, seed=48, bg=(0.0, 0.0, 0.0)),
    "sh_negative": dict(S=5, seed=49, sh_shift=-1.2),
    "aniso_fov_ragged": dict(S=5, seed=50, W=200, H=120, fovy_scale=1.3),
    "deep_list": dict(S=5, seed=51, P=4000, scale_log_mean=-2.5, W=48, H=40),
}
# The backward parity cases of tests/test_rasterizer_gpu.py (test_backward_parity, test_backward_no_geometry_flag)
BWD_CASES = {
    "S5": dict(S=5),
    "S0": dict(S=0, seed=21),
    "S16": dict(S=16, seed=22),
    "S24": dict(S=24, seed=23, P=1500),
    "S33": dict(S=33, seed=24, P=1000),
    "colors_precomp": dict(S=3, use_colors=True, seed=25),
    "cov_precomp": dict(S=4, use_cov=True, seed=26),
    "ragged_image": dict(S=5, W=200, H=120, seed=27),
    "big_splats": dict(S=5, scale_log_mean=-1.5, P=800, seed=28),
}
NO_GEOMETRY_CASE = dict(S=5, seed=31)
TILE_ARRAYS = ("mean2D", "conic", "opacity", "colors", "feature")
STAGE_ARRAYS = ("means3D", "cov3D", "sh", "scales", "rot")


def upstream(case, seed=123):
    """Seeded upstream gradients (colour, opacity, depth, feature) of a case, CPU fp32."""
    H, W, S = case["H"], case["W"], case["S"]
    g = torch.Generator().manual_seed(seed)
    gC, gO, gD = torch.randn(3, H, W, generator=g), torch.randn(1, H, W, generator=g), torch.randn(1, H, W, generator=g)
    return gC, gO, gD, torch.randn(S, H, W, generator=g)


def oracle_backward(case, fwd_ref, ups, backward_geometry=True, **kw):
    """oracle.rasterizer.rasterize_gaussians_backward of a case on the oracle forward `fwd_ref` (keyword arguments passed on)."""
    from oracle import rasterizer as orc
    c = fwd_args(case)
    return orc.rasterize_gaussians_backward(c[0], c[1], c[2], fwd_ref[9], c[3], c[5], c[6], c[7], c[8], c[9], c[10], c[11],
                                            c[12], ups[0], ups[1], ups[2], ups[3], c[17], c[18], c[19], fwd_ref[-1],
                                            backward_geometry, **kw)


def stage_args(case, fwd_ref, d_mean2D, d_conic, d_colors):
    """Arguments of oracle.rasterizer.per_gaussian_backward_f64 / per_gaussian_sigma for a case and given tile-pass sums (the
    sums as the per-Gaussian kernel sees them: fp32)."""
    c = fwd_args(case)
    st = fwd_ref[-1]
    f32 = lambda a: to_np(a).astype(np.float32)
    return (c[1], c[5], c[6], c[7], c[8], c[17], c[18], c[9], c[10], c[11], c[12], c[19], case["W"], case["H"], fwd_ref[9],
            st["clamped"], f32(d_mean2D).reshape(-1, 3), f32(d_conic).reshape(-1, 4), f32(d_colors).reshape(-1, 3))


# ---- the recording library of the relight CPU tests (tests/test_host_mirrors_cpu.py, tests/test_relight_device_visibility_cpu.py,
# tests/test_relight_baked_cpu.py, tests/test_relight_call_sequences_cpu.py) and of tests/test_fused_samples_call_sequences_cpu.py:
# the host side of a renderer or a step with every C-ABI entry point replaced by a recorder, so that nothing runs on a GPU -----------------------------------------------------------------
class DeviceTensor(torch.Tensor):            # a CPU tensor that claims to be a device tensor
    is_cuda = property(lambda self: True)


def dt(t):
    return t.as_subclass(DeviceTensor)


class Recorder:
    """Stands for the loaded library: every entry point appends (name, args) -- or what `convert(name, args)` makes of them --
    to `calls` and returns 0 (or `returns[name]`).  `wanted` collects the `want_weights` of every rasterizer front end the fake
    below stood in for."""

    def __init__(self, convert=None, returns=None):
        self.calls, self.wanted, self.convert = [], [], convert or (lambda name, args: (name, args))
        self.returns = returns or {}

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append(self.convert(name, args))
            return self.returns.get(name, 0)
        return fn

    def names(self):
        return [c[0] for c in self.calls]

    def args_of(self, name):
        return [c[1] for c in self.calls if c[0] == name]


class FakePending:
    """What rasterizer_ops.rasterize_gaussians_begin returns, for a 4x4 frame of P Gaussians of which 3 are rendered."""

    def __init__(self, P):
        self.P = P

    def finish(self, ordering_stream=None):
        z = torch.zeros
        return (3, z(1), z(3, 4, 4), z(1, 4, 4), z(1, 4, 4), z(28, 4, 4), z(3, 4, 4), z(3, 4, 4), None, z(self.P))


def recording_library(monkeypatch, P, convert=None, returns=None):
    """Puts a Recorder in the place of the library for the rest of the test and makes the host code around it run on CPU
    tensors (the renderer's own buffers are CPU tensors here); the rasterizer front end returns a FakePending."""
    import contextlib
    from relightable3dgaussian_amd import _lib, rasterizer_ops, shading_ops
    rec = Recorder(convert, returns)
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(_lib, "current_stream", lambda: 0)
    monkeypatch.setattr(shading_ops, "_c", lambda t: t.contiguous())
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(rasterizer_ops, "rasterize_gaussians_begin",
                        lambda *a, want_weights=True, **k: rec.wanted.append(want_weights) or FakePending(P))
    return rec


def relight_model(P, **extra):
    """The raw parameters RelightRenderer reads, all zero; `xyz` claims to be on a device."""
    import types
    z = torch.zeros
    return types.SimpleNamespace(xyz=dt(z(P, 3)), normal=z(P, 3), scaling=z(P, 3), rotation=z(P, 4), opacity=z(P, 1),
                                 base_color=z(P, 3), roughness=z(P, 1), shs=z(P, 16, 3), incidents=z(P, 16, 3), **extra)


def relight_camera():
    import types
    return types.SimpleNamespace(image_height=4, image_width=4, world_view_transform=torch.eye(4), full_proj_transform=torch.eye(4),
                                 camera_center=torch.zeros(3), tanfovx=0.5, tanfovy=0.5, cx=2.0, cy=2.0)


def z_rotation_by(a, device=None):
    """A light rotation: `a` radians about z."""
    import math
    return torch.tensor([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]], device=device)


def z_rotation(i):
    """The light rotation of step i of a turning light in the recording-library tests: 0.3 i radians about z, on the host."""
    return z_rotation_by(0.3 * i)


# ---- the turning-light sequence of the relight GPU tests (tests/test_relight_gpu.py, tests/test_relight_device_visibility_gpu.py,
# tests/test_relight_baked_gpu.py) -------------------------------------------------------------------------------------------------
CACHED_PATTERN = [True, False, False, False, True, True]        # the first change still builds; a light that stops is cached again
SPLIT_PATTERN = [False, True, True, True, True, True]           # built at the second consecutive change, kept


def turning_light_frames(r, cam, bg, per_frame=None):
    """Six frames of renderer `r` under a light on the device that turns four times and then stops (the last rotation three times
    over), each into a NaN-filled shade_out.  -> (rotations, cached, split, frames): per frame whether the lookup cache was
    live after it, whether a split cache was, and copies of the "feature" and "pbr_env" images.  `per_frame(tr, got)` runs
    after each frame, while shade_out still holds it."""
    trs = [z_rotation_by(a, device=cam.world_view_transform.device) for a in (0.1, 0.7, 1.3, 1.9)]
    trs += [trs[-1], trs[-1]]
    cached, split, frames = [], [], []
    for tr in trs:
        r.shade_out.fill_(float("nan"))
        got = r.frame(cam, bg, env_transform=tr, outputs=("pbr_env",))
        cached.append(r._taps_key == r._light_key)
        split.append(bool(r._split))
        frames.append({k: got[k].clone() for k in ("feature", "pbr_env")})
        if per_frame is not None:
            per_frame(tr, got)
    return trs, cached, split, frames


def assert_frame_matches_glue(r, cam, bg, tr, got):
    """`got` against relight.frame_reference(exact_activations=True) under the light `tr`, which shades with the general HIP op:
    two fp32 evaluations of the ill-conditioned GGX term."""
    from relightable3dgaussian_amd import relight
    want = relight.frame_reference(r, cam, bg, env_transform=tr, exact_activations=True)
    for k, rtol, atol in (("feature", 1e-3, 1e-6), ("pbr_env", 0.0, 4e-4)):
        ok, msg = report(k, got[k], want[k], rtol, atol)
        assert ok, msg
