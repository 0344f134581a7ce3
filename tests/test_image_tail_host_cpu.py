"""The Python side of the fused image tail (FusedStage2Step._image_loss): with a recording library that ANSWERS 1 to
r3dg_stage2_image_tail_supported -- the recorders of tests/test_host_mirrors_cpu.py answer 0 and keep describing the four-launch
path -- one iteration calls r3dg_stage2_image_tail once, in the place of the four launches, on planes 0, 3, 4 of a twenty-plane
slab; R3DG_IMAGE_TAIL=0 brings the four calls back.  Nothing runs on a GPU."""
import contextlib
import types

import pytest
import torch

FOUR = ("r3dg_stage2_normals_srgb", "r3dg_ssim_forward_pair", "r3dg_ssim_backward_pair", "r3dg_stage2_loss")
TAIL = "r3dg_stage2_image_tail"
P, K, H, W = 6, 8, 4, 4
z = torch.zeros


@pytest.fixture
def recorded(monkeypatch):
    """-> (calls, make_step, camera): FusedStage2Step on CPU tensors over a library that records every call."""
    from relightable3dgaussian_amd import _lib, fused_step, rasterizer_ops, shading_ops
    calls = []
    yes = {"r3dg_bounded_forward_supported", "r3dg_stage2_image_tail_supported"}

    class Recorder:
        def __getattr__(self, name):
            def fn(*args):
                calls.append((name, args))
                return 1 if name in yes else 0
            return fn

    class FakeStream:
        cuda_stream = 0

        def wait_stream(self, other):
            pass

    class Pending:
        def finish(self, ordering_stream=None):
            return (17, z(H, W, dtype=torch.int32), z(3, H, W), z(1, H, W), z(1, H, W), z(16, H, W), z(3, H, W), z(3, H, W),
                    z(P, 1), z(P, dtype=torch.int32), z(64, dtype=torch.uint8), z(8, dtype=torch.uint8), z(8, dtype=torch.uint8))

    def begin(*a, **k):
        return Pending()
    # the stand-in for the forward answers the capability question as the real one does: by asking the library
    begin.image_tail_supported = rasterizer_ops._image_tail_supported
    assert rasterizer_ops.rasterize_gaussians_begin.image_tail_supported is rasterizer_ops._image_tail_supported
    monkeypatch.setattr(_lib, "lib", lambda: Recorder())
    monkeypatch.setattr(_lib, "current_stream", lambda: 0)
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "stream", lambda s: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "Stream", lambda device=None: FakeStream())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: FakeStream())
    monkeypatch.setattr(fused_step, "update_visibility", lambda *a, **k: (torch.ones(P, K, 1), torch.ones(P, K, 3),
                                                                          torch.full((P, K, 1), 2.0), None))
    monkeypatch.setattr(shading_ops, "build_taps", lambda dirs, He, We, *a, **k: z(P * K * 3))
    monkeypatch.setattr(shading_ops, "_c", lambda t: t.contiguous())
    monkeypatch.setattr(rasterizer_ops, "rasterize_gaussians_begin", begin)
    monkeypatch.setattr(rasterizer_ops, "rasterize_gaussians_backward", lambda *a, **k: (
        z(P, 3), z(P, 3), z(P, 1), z(P, 3), z(P, 16), z(P, 6), z(P, 16, 3), z(P, 3), z(P, 4)))
    monkeypatch.setattr(rasterizer_ops, "rasterize_gaussians_backward_features", lambda *a, **k: z(P, 16))
    monkeypatch.setattr(rasterizer_ops, "num_rendered_of", lambda geom, P_: torch.tensor(17))
    monkeypatch.delenv("R3DG_IMAGE_TAIL", raising=False)
    params = types.SimpleNamespace(xyz=z(P, 3), normal=z(P, 3), scaling=z(P, 3), rotation=z(P, 4), opacity=z(P, 1),
                                   features_dc=z(P, 1, 3), features_rest=z(P, 15, 3), base_color=z(P, 3), roughness=z(P, 1),
                                   incidents_dc=z(P, 1, 3), incidents_rest=z(P, 15, 3), env=z(1, 16, 32, 3))
    cam = types.SimpleNamespace(image_height=H, image_width=W, world_view_transform=torch.eye(4), full_proj_transform=torch.eye(4),
                                camera_center=z(3), tanfovx=0.5, tanfovy=0.5, cx=2.0, cy=2.0)
    return calls, (lambda **kw: fused_step.FusedStage2Step(params, K, **kw)), cam


def _slab_of(step, cam, calls, **kw):
    """One iteration; -> (names of its calls, the slab _image_loss returned)."""
    seen = {}
    inner = step._image_loss

    def spy(v, fw):
        seen["g"], seen["active"] = inner(v, fw)
        return seen["g"], seen["active"]
    step._image_loss = spy
    calls.clear()
    step(cam, torch.ones(3), z(3, H, W), **kw)
    step._image_loss = inner
    return [c[0] for c in calls], seen["g"]


def test_one_call_in_the_place_of_four(recorded):
    calls, make_step, cam = recorded
    step = make_step()
    for _ in range(2):                                   # the two-phase first iteration and a bounded one
        names, g = _slab_of(step, cam, calls)
        assert names.count(TAIL) == 1 and not any(n in names for n in FOUR)
        # between the shading forward / feature rows and what follows the tail: the Adam under the backward, the gradient unpack
        i = names.index(TAIL)
        assert names.index("r3dg_shade_forward_cached") < names.index("r3dg_stage2_pack_features") < i
        assert i < names.index("r3dg_stage2_unpack_gradients") and i < names.index("r3dg_adam_step")
        args = [c[1] for c in calls if c[0] == TAIL][0]
        assert len(args) == 29 and args[1:3] == (W, H) and args[4:8] == (0.5, 0.5, 2.0, 2.0)
        # the slab ends behind the feature gradients; dL_dimage, dL_dopacity, dL_dfeature are its planes 0, 3, 4
        assert tuple(g.shape) == (20, H, W)
        assert args[23:26] == (g[0].data_ptr(), g[3].data_ptr(), g[4].data_ptr())
        assert args[15] is None                                                   # no object mask in this objective
        assert args[26] == step.sums.data_ptr() and args[27:29] == (step.sums[5].data_ptr(), step.sums[6].data_ptr())
        N = H * W
        lam = 0.2
        assert abs(args[16] - step.w["l1"] * (1 - lam) / (3 * N)) < 1e-12 and abs(args[19] + step.w["l1"] * lam / (3 * N)) < 1e-12
        assert abs(args[17] - step.w["pbr"] * (1 - lam) / (3 * N)) < 1e-12 and abs(args[20] + step.w["pbr"] * lam / (3 * N)) < 1e-12
        assert step.last_active_features == ([2, 3, 4] + ([5, 6, 7] if step.w["normal"] != 0.0 else []))


def test_mask_and_smoothness_under_the_syn4_weights(recorded):
    from relightable3dgaussian_amd import train_step
    calls, make_step, cam = recorded
    frozen_lrs = dict(xyz=0.0, normal=0.0, scaling=0.0, rotation=0.0, opacity=0.0, shs=0.0, shs_rest=0.0, base_color=0.01,
                      roughness=0.01, incidents=0.001, incidents_rest=0.0001, env=0.1)
    step = make_step(lrs=frozen_lrs, loss_weights=train_step.STAGE2_WEIGHTS_SYN4)
    mask = torch.ones(1, H, W)
    names, g = _slab_of(step, cam, calls, image_mask=mask)
    assert names.count(TAIL) == 1 and not any(n in names for n in FOUR)
    assert names.index("r3dg_stage2_pack_features") < names.index(TAIL) < names.index("r3dg_stage2_smooth_fused")
    args = [c[1] for c in calls if c[0] == TAIL][0]
    assert args[15] == mask.data_ptr()
    sm = [c[1] for c in calls if c[0] == "r3dg_stage2_smooth_fused"][0]
    assert sm[12:14] == (g[3].data_ptr(), g[4].data_ptr())                        # the smoothness terms add to the same slab
    assert sm[7] == mask.data_ptr() and tuple(g.shape) == (20, H, W)
    assert set(step.last_active_features) >= {2, 3, 4, 8, 9, 10, 11, 12, 13, 14}


def test_switch_restores_the_four_calls(recorded, monkeypatch):
    calls, make_step, cam = recorded
    step = make_step()
    monkeypatch.setenv("R3DG_IMAGE_TAIL", "0")
    names, g = _slab_of(step, cam, calls)
    assert TAIL not in names and "r3dg_stage2_image_tail_supported" not in names
    assert [n for n in names if n in FOUR] == list(FOUR) and tuple(g.shape) == (47, H, W)
    loss_args = [c[1] for c in calls if c[0] == "r3dg_stage2_loss"][0]
    assert loss_args[16:19] == (g[0].data_ptr(), g[3].data_ptr(), g[4].data_ptr()) and loss_args[14] == g[41].data_ptr()
    monkeypatch.setenv("R3DG_IMAGE_TAIL", "1")
    names, g = _slab_of(step, cam, calls)
    assert names.count(TAIL) == 1 and not any(n in names for n in FOUR)


def test_a_library_or_a_forward_without_the_kernel_keeps_the_four_calls(recorded, monkeypatch):
    from relightable3dgaussian_amd import rasterizer_ops
    calls, make_step, cam = recorded
    step = make_step()
    monkeypatch.setattr(rasterizer_ops.rasterize_gaussians_begin, "image_tail_supported", lambda W_, H_: False)
    names, g = _slab_of(step, cam, calls)
    assert TAIL not in names and [n for n in names if n in FOUR] == list(FOUR)
    monkeypatch.delattr(rasterizer_ops.rasterize_gaussians_begin, "image_tail_supported")
    names, g = _slab_of(step, cam, calls)
    assert TAIL not in names and [n for n in names if n in FOUR] == list(FOUR)
