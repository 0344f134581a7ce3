"""The Python side of the whole single-GPU iteration whose geometry backward applies the SH colour group's Adam
(FusedStage2Step._fuses_sh_adam), with recorders in place of the library and the rasterizer -- nothing runs on a GPU: which calls
carry the group's update, with which step count, and when the separate launch comes back."""
import contextlib
import ctypes
import types

import torch

from tests.helpers import Recorder

P, K, H, W = 6, 8, 4, 4


def _step_with_recorders(monkeypatch, backward_can_fuse=True, **step_kw):
    from relightable3dgaussian_amd import _lib, fused_adam, fused_step, rasterizer_ops, shading_ops
    rec = Recorder(returns={"r3dg_bounded_forward_supported": 1})
    z = torch.zeros
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(_lib, "current_stream", lambda: 0)
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "stream", lambda s: contextlib.nullcontext())

    class FakeStream:
        cuda_stream = 0

        def wait_stream(self, other):
            pass
    monkeypatch.setattr(torch.cuda, "Stream", lambda device=None: FakeStream())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: FakeStream())
    monkeypatch.setattr(fused_step, "update_visibility", lambda *a, **k: (torch.ones(P, K, 1), torch.ones(P, K, 3),
                                                                          torch.full((P, K, 1), 2.0), None))
    monkeypatch.setattr(shading_ops, "build_taps", lambda dirs, He, We, *a, **k: z(P * K * 3))
    monkeypatch.setattr(shading_ops, "_c", lambda t: t.contiguous())

    class Pending:
        def finish(self, ordering_stream=None):
            return (17, z(H, W, dtype=torch.int32), z(3, H, W), z(1, H, W), z(1, H, W), z(16, H, W), z(3, H, W), z(3, H, W),
                    z(P, 1), z(P, dtype=torch.int32), z(64, dtype=torch.uint8), z(8, dtype=torch.uint8), z(8, dtype=torch.uint8))
    monkeypatch.setattr(rasterizer_ops, "rasterize_gaussians_begin", lambda *a, **k: Pending())
    backwards = []

    def backward(*a, **k):
        sh_adam = k.get("sh_adam")
        if sh_adam is not None:         # (the descriptor is only valid during the call: read it now)
            desc = fused_adam.AdamGroup.from_address(sh_adam[0])
            sh_adam = (dict(param=desc.param, grad=desc.grad, exp_avg=desc.exp_avg, n=desc.n, lr=desc.lr, lr_tail=desc.lr_tail,
                            period=desc.period, split=desc.split),) + tuple(sh_adam[1:])
        backwards.append(sh_adam)
        rec.calls.append(("raster.backward", ()))
        return (z(P, 3), z(P, 3), z(P, 1), z(P, 3), z(P, 16), z(P, 6), z(P, 16, 3), z(P, 3), z(P, 4))
    if backward_can_fuse:
        backward.sh_adam_supported = lambda M: M == 16
    monkeypatch.setattr(rasterizer_ops, "rasterize_gaussians_backward", backward)
    monkeypatch.setattr(rasterizer_ops, "num_rendered_of", lambda geom, P_: torch.tensor(17))
    params = types.SimpleNamespace(xyz=z(P, 3), normal=z(P, 3), scaling=z(P, 3), rotation=z(P, 4), opacity=z(P, 1),
                                   features_dc=z(P, 1, 3), features_rest=z(P, 15, 3), base_color=z(P, 3), roughness=z(P, 1),
                                   incidents_dc=z(P, 1, 3), incidents_rest=z(P, 15, 3), env=z(1, 16, 32, 3))
    cam = types.SimpleNamespace(image_height=H, image_width=W, world_view_transform=torch.eye(4), full_proj_transform=torch.eye(4),
                                camera_center=z(3), tanfovx=0.5, tanfovy=0.5, cx=2.0, cy=2.0)
    step = fused_step.FusedStage2Step(params, K, **step_kw)
    del rec.calls[:]
    return step, rec, backwards, (cam, torch.ones(3), z(3, H, W))


def _adam_launches(rec):
    return [a[1] for a in rec.args_of("r3dg_adam_step")]          # the group count of every launch


def test_whole_iterations_hand_the_sh_group_to_the_geometry_backward(monkeypatch):
    step, rec, backwards, view = _step_with_recorders(monkeypatch)
    sh = step._opt_order.index("shs")
    grp = step.opt.groups[sh]
    for it in (1, 2, 3):
        step(*view)
        desc, beta1, beta2, eps, count, scale, skip = backwards[-1]
        # the group IS the SH tensor with its two rates by column; no gradient buffer is named; the iteration's own step count
        # (begun after the call, in _schedule_early) and its own slot of the overflow-flag ring
        f32 = lambda x: ctypes.c_float(x).value
        assert desc == dict(param=step.shs.data_ptr(), grad=None, exp_avg=grp["exp_avg"].data_ptr(), n=48 * P, lr=f32(grp["lr"]),
                            lr_tail=f32(grp["lr_tail"]), period=48, split=3)
        assert (beta1, beta2, eps, scale) == (0.9, 0.999, 1e-15, 1.0) and count == it == step.opt.step_count
        assert skip == step._skip_cur.data_ptr()
    # ONE Adam launch per iteration, the nine other groups, behind the backward; none for the SH group
    assert _adam_launches(rec) == [9, 9, 9]
    names = rec.names()
    assert names.index("raster.backward") < names.index("r3dg_adam_step")
    # the A/B switch restores the separate early launch: the group alone, then the other nine
    monkeypatch.setenv("R3DG_SH_ADAM_IN_BACKWARD", "0")
    del rec.calls[:]
    step(*view)
    assert backwards[-1] is None and _adam_launches(rec) == [1, 9]
    monkeypatch.delenv("R3DG_SH_ADAM_IN_BACKWARD")
    # without the early Adam (above a million Gaussians; R3DG_EARLY_ADAM overrides the size rule) the group is still updated in
    # the backward: the one late launch carries the other nine
    monkeypatch.setenv("R3DG_EARLY_ADAM", "0")
    del rec.calls[:]
    step(*view)
    assert backwards[-1] is not None and backwards[-1][4] == step.opt.step_count == 5 and _adam_launches(rec) == [9]
    monkeypatch.delenv("R3DG_EARLY_ADAM")
    # a bare forward_backward + optimizer_step: callers read grads["shs"], so the backward writes it and Adam reads it
    del rec.calls[:]
    step.forward_backward(*view)
    step.optimizer_step()
    assert backwards[-1] is None and _adam_launches(rec) == [10] and step.opt.step_count == 6


def test_the_separate_launch_stays_where_the_backward_cannot_or_need_not_fuse(monkeypatch):
    # a backward without the capability (a wrapper, an older build)
    step, rec, backwards, view = _step_with_recorders(monkeypatch, backward_can_fuse=False)
    step(*view)
    assert backwards == [None] and _adam_launches(rec) == [1, 9] and not step._fuses_sh_adam()
    # a frozen SH group: nothing to apply
    step, rec, backwards, view = _step_with_recorders(monkeypatch, lrs=dict(shs=0.0, shs_rest=0.0))
    step(*view)
    assert backwards == [None] and _adam_launches(rec) == [9] and not step._fuses_sh_adam()
