"""The MVS depth / normal supervision and the per-Gaussian terms (csrc/supervision.hip) without a GPU: the PyTorch parity
functions of train_step against the reference's own calculate_loss (tests/golden/supervision_reference.npz, written by
tests/golden/make_supervision_golden.py: float64, every term alone), the weight keys, the header, and the host logic of the two
fused iterations with a recording library."""
import contextlib
import os
import types

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "supervision_reference.npz")
S1_BASE = dict(l1=1.0, mask_entropy=0.0, normal_render_depth=0.0, normal_smooth=0.0, depth_var=0.0)


@pytest.fixture(scope="module")
def z():
    f = np.load(GOLD)
    return {k: f[k] for k in f.files}


def _close(name, got, want, rtol):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = np.abs(want).max()
    assert scale > 0, name + ": the fixture's array is all zero"
    err = np.abs(got - want).max()
    assert err <= rtol * scale, "%s: max|err| %.3e, scale %.3e" % (name, err, scale)


def test_new_weight_keys_exist_and_default_to_zero():
    from relightable3dgaussian_amd import train_loop, train_step as ts
    for k in ("depth", "normal_mvs_depth"):
        assert ts.STAGE2_WEIGHTS[k] == 0.0 and ts.STAGE2_WEIGHTS_SYN4[k] == 0.0
    for k in ("depth_smooth", "point_entropy", "orientation", "scaling"):
        assert ts.STAGE1_WEIGHTS[k] == 0.0
    assert ts.STAGE1_WEIGHTS["orientation_from_iter"] == 5000
    sch = train_loop.Schedule()
    assert (sch.lambda_depth_smooth, sch.lambda_point_entropy, sch.lambda_orientation, sch.lambda_scaling) == (0.0,) * 4
    assert sch.lambda_orientation_from_iter == 5000
    # the schedules of render.py:191 and :218
    assert ts.scaling_weight(0.5, 0, 30000) == 0.5 and abs(ts.scaling_weight(0.5, 30000, 30000) - 0.005) < 1e-12
    assert abs(ts.scaling_weight(0.5, 6000, 30000) - (0.5 - 0.99 * 0.5 * 0.8)) < 1e-12


def test_header_declares_the_four_entry_points():
    from relightable3dgaussian_amd import _abi
    import ctypes as C
    want = {"r3dg_supervision_count": 6, "r3dg_stage2_supervision": 16, "r3dg_stage1_depth_smooth": 12,
            "r3dg_stage1_gaussian_terms": 16}
    for name, n in want.items():
        assert name in _abi.prototypes, name
        res, args = _abi.prototypes[name]
        assert res is C.c_int and len(args) == n, (name, len(args))
    # device pointers (the count included: it never visits the host), three float weights + the flag
    res, args = _abi.prototypes["r3dg_stage2_supervision"]
    assert args[9] is C.c_void_p and args[10] is C.c_float and args[11] is C.c_float and args[12] is C.c_int
    assert _abi.prototypes["r3dg_supervision_count"][1][5] is C.c_void_p


def test_stage2_parity_terms_reproduce_the_reference(z):
    from relightable3dgaussian_amd import train_step as ts
    t = lambda k: torch.from_numpy(z[k]).double()
    mask_c = (torch.from_numpy(z["map_n_contrib"]) > 0)[None]
    for name, masked in (("depth", True), ("normal_mvs_depth", True), ("depth_nomask", False)):
        key = "depth" if name == "depth_nomask" else name
        w = dict(ts.STAGE2_WEIGHTS, **{key: float(z["s2_%s_lambda" % key])})
        feature, opacity = t("map_feat16").requires_grad_(True), t("map_opacity").requires_grad_(True)
        feat = feature / opacity.clamp_min(1e-5) * mask_c
        loss = ts.stage2_supervision(feat, t("map_gt_depth"), t("map_mvs_normal"), t("map_mask") if masked else None, w)
        loss.backward()
        _close(name + " term", loss.detach().reshape(1), z["s2_%s_term" % name].reshape(1), 1e-12)
        _close(name + " g_feature", feature.grad, z["s2_%s_g_feature" % name], 1e-12)
        _close(name + " g_opacity", opacity.grad, z["s2_%s_g_opacity" % name], 1e-12)
    assert abs(float(z["s2_depth_tb"]) * 0.7 - float(z["s2_depth_term"])) < 1e-12
    # the selection the count kernel restates
    sel = (z["map_mask"] != 0) == (z["map_gt_depth"] > 0)
    assert int(sel.sum()) == int(z["count_masked"]) and 0 < int(z["count_masked"]) < sel.size
    assert int((z["map_gt_depth"] > 0).sum()) == int(z["count_nomask"]) != int(z["count_masked"])
    with pytest.raises(RuntimeError):
        ts.stage2_supervision(feat.detach(), None, None, None, dict(ts.STAGE2_WEIGHTS, depth=1.0))
    with pytest.raises(RuntimeError):
        ts.stage2_supervision(feat.detach(), t("map_gt_depth"), None, None, dict(ts.STAGE2_WEIGHTS, normal_mvs_depth=1.0))


def _stage1_case(z, dtype):
    t = lambda k: torch.from_numpy(z[k]).to(dtype)
    leaves = dict(feature=t("map_feat5"), opacity=t("map_opacity"), opac=t("pt_opac"), normal=t("pt_normal"), xyz=t("pt_xyz"),
                  scales=t("pt_scales"))
    for v in leaves.values():
        v.requires_grad_(True)
    gt = t("map_gt")
    n_contrib = torch.from_numpy(z["map_n_contrib"])
    # the rasterizer's ten outputs as stage1_loss reads them (the image equals the target: the L1 / SSIM part vanishes)
    outs = (0, n_contrib, gt, leaves["opacity"], None, leaves["feature"], None, None, t("pt_weights"), None)
    gaussians = dict(opacity=leaves["opac"], normal=leaves["normal"], scales=leaves["scales"], xyz=leaves["xyz"],
                     campos=t("pt_campos"))
    return leaves, outs, gt, gaussians


@pytest.mark.parametrize("name", ["depth_smooth", "point_entropy", "orientation", "scaling"])
def test_stage1_loss_reproduces_the_reference(z, name):
    """train_step.stage1_loss (float32, as it runs) with ONE of the new terms on against the reference's float64 value and
    gradients: 1e-5 of the scale -- float32 rounding of sums over at most 3 x 29 x 37 elements."""
    from relightable3dgaussian_amd import train_step as ts
    leaves, outs, gt, gaussians = _stage1_case(z, torch.float32)
    w = dict(S1_BASE, **{name: float(z["s1_%s_lambda" % name])})
    it, its = int(z["iteration"]), int(z["iterations"])
    assert it > int(z["orientation_from_iter"]) == ts.STAGE1_WEIGHTS["orientation_from_iter"]
    loss = ts.stage1_loss(outs, gt, None, w, it, gaussians=gaussians, iterations=its)
    loss.backward()
    _close(name + " term", loss.detach().reshape(1), z["s1_%s_term" % name].reshape(1), 1e-5)
    seen = 0
    for k, v in leaves.items():
        key = "s1_%s_g_%s" % (name, k)
        if key in z:
            _close(key, v.grad, z[key], 1e-5)
            seen += 1
        else:
            assert v.grad is None or float(v.grad.abs().max()) == 0.0, key
    assert seen == {"depth_smooth": 2, "point_entropy": 1, "orientation": 2, "scaling": 1}[name]
    if name == "orientation":           # gated: at iteration == orientation_from_iter the term is still off (render.py:191)
        off = ts.stage1_loss(outs, gt, None, w, 5000, gaussians=gaussians, iterations=its)
        assert abs(float(off)) < 1e-6
    if name != "depth_smooth":
        with pytest.raises(RuntimeError):
            ts.stage1_loss(outs, gt, None, w, it)


# ---- host logic of the fused iterations with every C-ABI entry point replaced by a recorder (nothing runs on a GPU) -------------
class _Recorder:
    def __init__(self, calls):
        self.calls = calls

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 1 if name == "r3dg_bounded_forward_supported" else 0
        return fn


P_, K_, H_, W_ = 6, 8, 4, 4


def _patch(monkeypatch, S):
    from relightable3dgaussian_amd import _lib, fused_step, rasterizer_ops, shading_ops
    calls, active = [], []
    z_ = torch.zeros
    monkeypatch.setattr(_lib, "lib", lambda: _Recorder(calls))
    monkeypatch.setattr(_lib, "current_stream", lambda: 0)
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "stream", lambda s: contextlib.nullcontext())

    class FakeStream:
        cuda_stream = 0

        def wait_stream(self, other):
            pass
    monkeypatch.setattr(torch.cuda, "Stream", lambda device=None: FakeStream())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: FakeStream())
    monkeypatch.setattr(fused_step, "update_visibility", lambda *a, **k: (torch.ones(P_, K_, 1), torch.ones(P_, K_, 3),
                                                                          torch.full((P_, K_, 1), 2.0), None))
    monkeypatch.setattr(shading_ops, "build_taps", lambda dirs, He, We, *a, **k: z_(P_ * K_ * 3))
    monkeypatch.setattr(shading_ops, "_c", lambda t: t.contiguous())

    class Pending:
        def finish(self, ordering_stream=None):
            return (17, z_(H_, W_, dtype=torch.int32), z_(3, H_, W_), z_(1, H_, W_), z_(1, H_, W_), z_(S, H_, W_), z_(3, H_, W_),
                    z_(3, H_, W_), z_(P_, 1), z_(P_, dtype=torch.int32), z_(64, dtype=torch.uint8), z_(8, dtype=torch.uint8),
                    z_(8, dtype=torch.uint8))
    monkeypatch.setattr(rasterizer_ops, "rasterize_gaussians_begin", lambda *a, **k: Pending())

    def backward(*a, **k):
        active.append(tuple(k["active_features"]))
        calls.append(("rasterize_backward", a))
        return (z_(P_, 3), z_(P_, 3), z_(P_, 1), z_(P_, 3), z_(P_, S), z_(P_, 6), z_(P_, 16, 3), z_(P_, 3), z_(P_, 4))
    monkeypatch.setattr(rasterizer_ops, "rasterize_gaussians_backward", backward)
    monkeypatch.setattr(rasterizer_ops, "rasterize_gaussians_backward_features",
                        lambda P, S_, H, W, gF, geom, R, binning, img, debug=False, active_features=None:
                        active.append(tuple(active_features)) or z_(P_, 16))
    monkeypatch.setattr(rasterizer_ops, "num_rendered_of", lambda geom, P: torch.tensor(17))
    params = types.SimpleNamespace(xyz=z_(P_, 3), normal=z_(P_, 3), scaling=z_(P_, 3), rotation=z_(P_, 4), opacity=z_(P_, 1),
                                   features_dc=z_(P_, 1, 3), features_rest=z_(P_, 15, 3), base_color=z_(P_, 3),
                                   roughness=z_(P_, 1), incidents_dc=z_(P_, 1, 3), incidents_rest=z_(P_, 15, 3),
                                   env=z_(1, 16, 32, 3))
    cam = types.SimpleNamespace(image_height=H_, image_width=W_, world_view_transform=torch.eye(4),
                                full_proj_transform=torch.eye(4), camera_center=z_(3), tanfovx=0.5, tanfovy=0.5, cx=2.0, cy=2.0)
    return calls, active, params, cam


@pytest.mark.parametrize("normal,light_smooth,normal_mvs", [(a, b, c) for a in (0.0, 0.01) for b in (0.0, 1.0) for c in (0.0, 0.3)])
def test_fused_stage2_host_logic_launches_and_accumulates_in_every_combination(monkeypatch, normal, light_smooth, normal_mvs):
    """`accumulate_normal` and the active feature maps for every combination of the three terms that write the normal maps'
    gradient, with the depth term on: the supervision kernel runs last and adds to maps 5..7 exactly when a kernel before it
    wrote them; the count is launched once per (depth map, mask) pair."""
    from relightable3dgaussian_amd import fused_step
    calls, active, params, cam = _patch(monkeypatch, 16)
    w = dict(normal=normal, light_smooth=light_smooth, normal_mvs_depth=normal_mvs, depth=0.7)
    step = fused_step.FusedStage2Step(params, K_, loss_weights=w)
    assert step.sums.shape[0] == 12
    calls.clear()
    gt, bg = torch.zeros(3, H_, W_), torch.ones(3)
    with pytest.raises(RuntimeError):
        step.forward_backward(cam, bg, gt)                                   # the depth map is missing
    depth, mvs, mask = torch.ones(1, H_, W_), torch.ones(3, H_, W_), torch.ones(1, H_, W_)
    if normal_mvs != 0.0:
        with pytest.raises(RuntimeError):
            step.forward_backward(cam, bg, gt, gt_depth=depth)               # ... or the normals
    calls.clear()
    del active[:]
    for _ in range(2):
        step(cam, bg, gt, image_mask=mask, gt_depth=depth, mvs_normal=mvs)
    names = [c[0] for c in calls]
    assert names.count("r3dg_supervision_count") == 1 and names.count("r3dg_stage2_supervision") == 2
    one = [n for n in names if n in ("r3dg_stage2_loss", "r3dg_stage2_smooth_fused", "r3dg_supervision_count",
                                     "r3dg_stage2_supervision", "rasterize_backward")]
    want = ["r3dg_stage2_loss"] + (["r3dg_stage2_smooth_fused"] if light_smooth else []) + [
        "r3dg_supervision_count", "r3dg_stage2_supervision", "rasterize_backward"]
    assert one[:len(want)] == want
    sup = [c[1] for c in calls if c[0] == "r3dg_stage2_supervision"][0]
    cnt = [c[1] for c in calls if c[0] == "r3dg_supervision_count"][0]
    N = H_ * W_
    assert sup[6] == depth.data_ptr() and sup[8] == mask.data_ptr() and sup[9] == cnt[5] and sup[10] == 0.7
    assert sup[7] == (mvs.data_ptr() if normal_mvs else None) and abs(sup[11] - normal_mvs / (3.0 * N)) < 1e-9
    assert sup[12] == (1 if (normal != 0.0 or light_smooth != 0.0) else 0)
    assert sup[15] == step.sums[10].data_ptr()
    loss_args = [c[1] for c in calls if c[0] == "r3dg_stage2_loss"][0]
    assert sup[13] == loss_args[17] and sup[14] == loss_args[18]             # the buffers r3dg_stage2_loss wrote
    normals_on = normal != 0.0 or light_smooth != 0.0 or normal_mvs != 0.0
    want = [0, 2, 3, 4] + ([5, 6, 7] if normals_on else []) + ([12, 13, 14] if light_smooth else [])
    assert active == [tuple(want)] * 2
    # a new depth map (or an edited one) is counted again
    step(cam, bg, gt, image_mask=mask, gt_depth=depth.clone(), mvs_normal=mvs)
    depth.add_(1.0)
    step(cam, bg, gt, image_mask=mask, gt_depth=depth, mvs_normal=mvs)
    assert [c[0] for c in calls].count("r3dg_supervision_count") == 3


def test_fused_stage2_frozen_geometry_keeps_the_mvs_terms_out_of_the_backward(monkeypatch):
    from relightable3dgaussian_amd import fused_step
    calls, active, params, cam = _patch(monkeypatch, 16)
    lrs = dict(xyz=0.0, normal=0.0, scaling=0.0, rotation=0.0, opacity=0.0, shs=0.0, shs_rest=0.0)
    step = fused_step.FusedStage2Step(params, K_, lrs=lrs, loss_weights=dict(depth=0.7, normal_mvs_depth=0.3))
    assert step.frozen_geometry
    step(cam, torch.ones(3), torch.zeros(3, H_, W_), gt_depth=torch.ones(1, H_, W_), mvs_normal=torch.ones(3, H_, W_))
    assert active == [(2, 3, 4)]                                             # the terms only show in loss()
    assert [c[0] for c in calls].count("r3dg_stage2_supervision") == 1


def test_fused_steps_with_default_weights_launch_and_allocate_nothing_new(monkeypatch):
    from relightable3dgaussian_amd import fused_step
    calls, active, params, cam = _patch(monkeypatch, 16)
    step = fused_step.FusedStage2Step(params, K_)
    assert step.sums.shape[0] == 10 and not step._supervised
    step(cam, torch.ones(3), torch.zeros(3, H_, W_), gt_depth=torch.ones(1, H_, W_), mvs_normal=torch.ones(3, H_, W_))
    assert active == [(2, 3, 4)]
    calls2, active2, params, cam = _patch(monkeypatch, 5)
    s1 = fused_step.FusedStage1Step(params)
    assert s1.sums.shape[0] == 6 and s1.iterations == 30_000
    s1(cam, torch.ones(3), torch.zeros(3, H_, W_))
    assert active2 == [(0, 1, 2, 3, 4)]
    new = {"r3dg_supervision_count", "r3dg_stage2_supervision", "r3dg_stage1_depth_smooth", "r3dg_stage1_gaussian_terms"}
    assert not new & {c[0] for c in calls + calls2}


def test_fused_stage1_host_logic(monkeypatch):
    """Depth smoothness behind r3dg_stage1_loss with map 3 active; the per-Gaussian kernel between the rasterizer backward and
    the activation chain rule, with the orientation gate and the scaling schedule in its weights."""
    from relightable3dgaussian_amd import fused_step, train_step as ts
    calls, active, params, cam = _patch(monkeypatch, 5)
    w = dict(depth_var=0.0, depth_smooth=0.4, point_entropy=0.6, orientation=0.8, scaling=0.5)
    step = fused_step.FusedStage1Step(params, loss_weights=w, iterations=20_000)
    assert step.sums.shape[0] == 10
    step.iteration = 4999                       # __call__ advances it to 5000: the orientation term is still off
    step(cam, torch.ones(3), torch.zeros(3, H_, W_))
    step(cam, torch.ones(3), torch.zeros(3, H_, W_))
    names = [c[0] for c in calls if c[0] in ("r3dg_stage1_loss", "r3dg_stage1_depth_smooth", "rasterize_backward",
                                             "r3dg_stage1_gaussian_terms", "r3dg_stage1_activate_backward")]
    assert names == ["r3dg_stage1_loss", "r3dg_stage1_depth_smooth", "rasterize_backward", "r3dg_stage1_gaussian_terms",
                     "r3dg_stage1_activate_backward"] * 2
    assert active == [(0, 1, 2, 3)] * 2
    ds = [c[1] for c in calls if c[0] == "r3dg_stage1_depth_smooth"][0]
    loss_args = [c[1] for c in calls if c[0] == "r3dg_stage1_loss"][0]
    assert abs(ds[7] - 0.4 / (3.0 * H_ * W_)) < 1e-9 and ds[9] == loss_args[18] and ds[10] == loss_args[19]
    assert ds[11] == step.sums[6].data_ptr()
    g0, g1 = [c[1] for c in calls if c[0] == "r3dg_stage1_gaussian_terms"]
    assert abs(g0[8] - 0.6 / P_) < 1e-9 and g0[9] == 0.0 and abs(g1[9] - 0.8 / P_) < 1e-9
    assert abs(g1[10] - ts.scaling_weight(0.5, 5001, 20_000) / P_) < 1e-12
    assert g1[15] == step.sums[7].data_ptr()
    ab = [c[1] for c in calls if c[0] == "r3dg_stage1_activate_backward"][1]
    assert (g1[11], g1[12], g1[13], g1[14]) == (ab[11], ab[8], ab[9], ab[12])      # dL_dopacity, dL_dfeatures, dL_dscales, dL_dmeans3D


def test_train_loop_passes_the_schedule_fields_through(monkeypatch):
    from relightable3dgaussian_amd import train_loop
    seen = {}

    class Stop(Exception):
        pass

    def fake(init, **kw):
        seen.update(kw)
        raise Stop
    monkeypatch.setattr(train_loop, "FusedStage1Step", fake)
    sch = train_loop.Schedule(iterations=7000, lambda_scaling=0.5, lambda_orientation=0.8, lambda_orientation_from_iter=100)
    with pytest.raises(Stop):
        train_loop.train_stage1(None, [], [], None, extent=1.0, schedule=sch, loss_weights=dict(normal_smooth=0.02))
    assert seen["iterations"] == 7000
    assert seen["loss_weights"] == dict(scaling=0.5, orientation=0.8, orientation_from_iter=100, normal_smooth=0.02)
    seen.clear()
    with pytest.raises(Stop):
        train_loop.train_stage1(None, [], [], None, extent=1.0)
    assert "iterations" not in seen and seen["loss_weights"] is None
