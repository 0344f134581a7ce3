"""The reference's `--save_training_vis` (train.py:276-317 save_training_vis): the contact sheet a run writes while it trains,
OUT/visualize/<iteration>.png -- 7 panels in stage 1 (render, gt, depth in `turbo`, depth variance, opacity, normal, pseudo normal),
16 in stage 2 (+ base colour, roughness, visibility, diffuse, specular, global lights, pbr, the two halves of the environment
texture), laid out by torchvision's make_grid(nrow=4), resampled to 800 rows and quantised by save_image.

Here a sheet is ONE eval frame of the live step plus ONE launch, r3dg_training_sheet (csrc/training_sheet.hip), which writes the
finished 8-bit picture from the frame's raw outputs: no panel, no grid, no resampled grid, and the loop never waits for a file
(relighting.FrameWriter.submit_bytes: pinned copy, event, PIL on a worker thread).

  stage 1   bench_core.render_stage1 on the step's parameters, as training.evaluate_step renders them.
  stage 2   the eval frame of neilf.py:97-130 (the full 19-column shading output, S = 28 feature rows) driven through the C ABI
            on the step's OWN parameter tensors, its own traced visibility and its own ray set: r3dg_stage2_activate,
            r3dg_shade_forward_cached, r3dg_relight_pack_features, the rasterizer forward.  Nothing is traced, no BVH call is
            made and no parameter group is cloned -- the reference's sheet reads `pc._visibility_tracing`, the cached visibility,
            too.  The environment is softplus(step.env)[0].  A step that holds no direction tensor (the fixed-ray-set kernels:
            the samples ARE the Fibonacci set of the snapshot normals) gets one here, regenerated from those normals once per
            visibility refresh and kept by the sheet (12 bytes per sample), never handed to the step.

THE ONE DIFFERENCE FROM THE REFERENCE: the fused iteration has applied Adam when the training loop's hook runs, so sheet `g`
shows the state AFTER iteration g; the reference renders its sheet before its optimizer step (train.py:150-177), the state
before it."""
import math

import torch

from . import _lib

PANELS = {1: 7, 2: 16}                       # stage -> panels of its sheet (train.py:283-311)


def sheet_size(panels, H, W):
    """-> (out_h, out_w, grid_h, grid_w) of a sheet of `panels` panels of H x W: make_grid(nrow=4, padding=2) and the
    reference's own expression for the resample (train.py:315-316), double-precision division and truncation included
    (800 x 800 frames: 800 x 1599 for 7 panels, 800 x 800 for 16)."""
    rows = -(-int(panels) // 4)
    grid_h, grid_w = rows * (int(H) + 2) + 2, 4 * (int(W) + 2) + 2
    scale = grid_h / 800
    return int(grid_h / scale), int(grid_w / scale), grid_h, grid_w


def launch_sheet(layout, render, gt, opacity, n_contrib, feature, pseudo_normal, background, env, out):
    """r3dg_training_sheet on device tensors: render / gt / pseudo_normal [3,H,W], opacity and n_contrib [.,H,W], the RAW
    feature image [S,H,W] (layout 0: S = 5; 1: S = 28), background [3] and env [R,2R,3] (layout 1), `out` uint8 [out_h,out_w,3]."""
    H, W = int(render.shape[-2]), int(render.shape[-1])
    S = 5 if layout == 0 else 28
    for name, t, shape, dtype in (("render", render, (3, H, W), torch.float32), ("gt", gt, (3, H, W), torch.float32),
                                  ("pseudo_normal", pseudo_normal, (3, H, W), torch.float32),
                                  ("feature", feature, (S, H, W), torch.float32)):
        if not t.is_cuda or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
            raise RuntimeError("training sheet: `%s` must be a contiguous %s %s on the device" % (name, dtype, list(shape)))
    for name, t, dtype in (("opacity", opacity, torch.float32), ("n_contrib", n_contrib, torch.int32)):
        if not t.is_cuda or t.dtype != dtype or t.numel() != H * W or not t.is_contiguous():
            raise RuntimeError("training sheet: `%s` must be a contiguous %s [H,W] on the device" % (name, dtype))
    if out.dtype != torch.uint8 or out.dim() != 3 or out.shape[2] != 3 or not out.is_contiguous() or not out.is_cuda:
        raise RuntimeError("training sheet: the output is a contiguous uint8 [out_h,out_w,3] on the device")
    R = 0
    if layout == 1:
        if env.dim() != 3 or env.shape[1] != 2 * env.shape[0] or env.shape[2] != 3 or not env.is_contiguous() or \
                env.dtype != torch.float32 or background.numel() != 3:
            raise RuntimeError("training sheet: the environment texture is a contiguous float32 [R,2R,3], the background 3 floats")
        R = int(env.shape[0])
    with torch.cuda.device(render.device):
        _lib.check(_lib.lib().r3dg_training_sheet(
            _lib.current_stream(), W, H, layout, render.data_ptr(), gt.data_ptr(), opacity.data_ptr(), n_contrib.data_ptr(),
            feature.data_ptr(), pseudo_normal.data_ptr(), None if background is None else background.data_ptr(),
            None if layout == 0 else env.data_ptr(), R, int(out.shape[1]), int(out.shape[0]), out.data_ptr()), "training_sheet")
    return out


class TrainingSheet:
    """The contact sheets of one live step (a FusedStage1Step or a FusedStage2Step; which one decides the layout).
    `sample_num`: the rays per Gaussian of the stage-2 frame -- the step's own (None), since the frame reads the step's own
    traced visibility; any other count raises.  Buffers are allocated once per size; `writer` (a relighting.FrameWriter) is
    created by the first save()."""

    def __init__(self, step, sample_num=None):
        from .fused_step import FusedStage2Step
        self.step = step
        self.stage = 2 if isinstance(step, FusedStage2Step) else 1
        if self.stage == 2 and sample_num is not None and int(sample_num) != step.K:
            raise RuntimeError("TrainingSheet: the sheet shades with the step's own visibility, traced at %d samples per Gaussian; "
                               "sample_num = %d is another ray set" % (step.K, sample_num))
        self.writer = None
        self.device_png = False               # True: the writer encodes on the device (relighting.FrameWriter(device_png=True))
        self._bytes = {}                      # (out_h, out_w) -> the device sheet
        self._buffers = None                  # stage 2: P and the activation / shading / feature-row buffers of that P
        self._dirs = None                     # stage 2: (snapshot normals, refresh count, directions) of a step that holds none
        self.frame_outputs = None             # the raw outputs the last sheet was made of (tests compare against them)

    # ---- the eval frame ---------------------------------------------------------------------------------------------------------
    def _frame_stage1(self, cam, background):
        from .bench_core import render_stage1
        from .training import _Stage1Model
        outs = render_stage1(_Stage1Model(self.step), cam, background)
        return dict(n_contrib=outs[1], render=outs[2], opacity=outs[3], feature=outs[5], pseudo_normal=outs[6], env=None)

    def _sample_tensors(self):
        """(visibility, directions, areas or None, uniform area) of the step's sample set, none of them traced here."""
        sm = self.step._samples
        if sm.incident_dirs is not None:
            return sm.visibility, sm.incident_dirs, sm.incident_areas, 0.0
        key = self._dirs
        if key is None or key[0] is not sm.ray_normals or key[1] != sm.refreshes:
            from . import sampling
            self._dirs = key = (sm.ray_normals, sm.refreshes, sampling.fibonacci_directions(sm.ray_normals, sm.K)[0])
        return sm.visibility, key[2], None, float(torch.tensor(2 * math.pi, dtype=torch.float32))

    def _frame_stage2(self, cam, background):
        from . import rasterizer_ops, shading_ops
        step, L = self.step, _lib.lib()
        P, dev = step.P, step.dev
        if self._buffers is None or self._buffers[0] != P:
            f = dict(dtype=torch.float32, device=dev)
            self._buffers = (P, [torch.empty(P, n, **f) for n in (3, 4, 1, 3, 3, 1, 3, shading_ops.NOUT, 28)])
        a_scales, a_rot, a_opacity, a_normal, a_base, a_rough, a_viewdirs, shade_out, features = self._buffers[1]
        incidents = step.incidents.detach()                 # (the property orders this stream behind a pending chain kernel)
        env = torch.nn.functional.softplus(step.env.detach())[0].contiguous()
        H, W = cam.image_height, cam.image_width
        vm, campos = cam.world_view_transform.contiguous(), cam.camera_center.contiguous()
        visibility, dirs, areas, uniform_area = self._sample_tensors()
        empty, stream = torch.Tensor([]), _lib.current_stream
        _lib.check(L.r3dg_stage2_activate(
            stream(), P, step.xyz.data_ptr(), step.scaling.data_ptr(), step.rotation.data_ptr(), step.opacity.data_ptr(),
            step.normal.data_ptr(), step.base_color.data_ptr(), step.roughness.data_ptr(), campos.data_ptr(), a_scales.data_ptr(),
            a_rot.data_ptr(), a_opacity.data_ptr(), a_normal.data_ptr(), a_base.data_ptr(), a_rough.data_ptr(),
            a_viewdirs.data_ptr(), None, None), "stage2_activate")
        # (the projection is queued now and runs beside the shading kernel, as in relight.RelightRenderer.frame)
        pending = rasterizer_ops.rasterize_gaussians_begin(
            background, step.xyz, features, empty, a_opacity, a_scales, a_rot, 1.0, empty, vm, cam.full_proj_transform,
            cam.tanfovx, cam.tanfovy, cam.cx, cam.cy, H, W, step.shs, 3, campos, False, True, False, want_weights=False)
        _lib.check(L.r3dg_shade_forward_cached(
            stream(), P, step.K, step.M, a_base.data_ptr(), a_rough.data_ptr(), a_normal.data_ptr(), a_viewdirs.data_ptr(),
            incidents.data_ptr(), env.data_ptr(), int(env.shape[0]), int(env.shape[1]), None, visibility.data_ptr(),
            dirs.data_ptr(), None if areas is None else areas.data_ptr(), uniform_area, None, 0, shade_out.data_ptr()),
            "shade_forward")
        _lib.check(L.r3dg_relight_pack_features(
            stream(), P, step.xyz.data_ptr(), vm.data_ptr(), a_normal.data_ptr(), a_base.data_ptr(), a_rough.data_ptr(),
            shade_out.data_ptr(), features.data_ptr()), "relight_pack_features")
        fw = pending.finish(step._order_stream)
        return dict(n_contrib=fw[1], render=fw[2], opacity=fw[3], feature=fw[5], pseudo_normal=fw[6], env=env)

    # ---- the sheet -------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def sheet(self, cam, gt, background):
        """-> uint8 [out_h,out_w,3] on the device: the sheet of view `cam` with ground truth `gt` [3,H,W] over `background` [3].
        The tensor is this object's buffer for that size: the next sheet of the size overwrites it (save() copies it out first)."""
        step = self.step
        step.flush()
        H, W = cam.image_height, cam.image_width
        gt = gt.detach()
        if tuple(gt.shape) != (3, H, W):
            raise RuntimeError("TrainingSheet: the ground truth of a %d x %d view is [3,%d,%d], got %s" % (H, W, H, W, tuple(gt.shape)))
        background = background.to(step.dev, torch.float32).reshape(3).contiguous()
        with step._ctx, torch.cuda.device(step.dev):
            fr = self._frame_stage1(cam, background) if self.stage == 1 else self._frame_stage2(cam, background)
            out_h, out_w = sheet_size(PANELS[self.stage], H, W)[:2]
            out = self._bytes.get((out_h, out_w))
            if out is None:
                out = self._bytes[(out_h, out_w)] = torch.empty(out_h, out_w, 3, dtype=torch.uint8, device=step.dev)
            self.frame_outputs = fr
            launch_sheet(self.stage - 1, fr["render"].contiguous(), gt.contiguous(), fr["opacity"].contiguous(),
                         fr["n_contrib"].contiguous(), fr["feature"].contiguous(), fr["pseudo_normal"].contiguous(), background,
                         fr["env"], out)
        return out

    def save(self, cam, gt, background, path):
        """The sheet as a PNG at `path`, encoded off the training thread (close() waits for the files and raises their errors)."""
        if self.writer is None:
            from .relighting import FrameWriter
            self.writer = FrameWriter(workers=2, device_png=True) if self.device_png else FrameWriter(workers=2)
        self.writer.submit_bytes(self.sheet(cam, gt, background), path)

    def close(self):
        if self.writer is not None:
            writer, self.writer = self.writer, None
            writer.close()
