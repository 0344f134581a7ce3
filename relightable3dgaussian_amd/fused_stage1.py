"""Fused stage-1 (plain 3DGS + normals) training iteration with densification: the glue kernels of csrc/stage1_glue.hip
around the rasterizer, no autograd graph, one-launch Adam (fused_adam.FusedAdam)."""
import collections

import torch

from . import _lib, densify, rasterizer_ops
from .fused_adam import FusedAdam
from .fused_base import SUM_SLOTS, FusedStepBase, _in_context, _world_of, grad_slab, learning_rates
from .train_step import LAMBDA_DSSIM, STAGE1_WEIGHTS, depth_var_weight, scaling_weight


class FusedStage1Step(FusedStepBase):
    """Stage-1 (plain 3DGS + normals) iteration without an autograd graph: activations -> S=5 feature row -> rasterize ->
    image-space loss + gradients -> rasterize backward -> activation chain rule -> one-launch Adam.  Same computation as
    bench_core.render_stage1 + loss_stage1 + torch.optim.Adam (the parity target, tests/test_fused_step_gpu.py);
    single-bucket gradient all-reduce under data parallelism."""

    _opt_order = ("xyz", "normal", "scaling", "rotation", "opacity", "shs")

    def __init__(self, params, lr=1e-4, lr_rest_scale=1.0, process_group=None, lrs=None, loss_weights=None, bounded=True,
                 iterations=30_000):
        """`bounded`: as FusedStage2Step -- after the first iteration (and again after every densify / prune, which changes
        the count) the rasterizer forward runs without the host read-back of num_rendered; a dropped view updates nothing
        and adds nothing to the densification statistics.
        `lrs`: optional per-group learning rates {xyz, normal, scaling, rotation, opacity, shs, shs_rest} as in
        GaussianModel.training_setup (gaussian_model.py:465-472; fused_base.learning_rates).
        `loss_weights`: overrides of train_step.STAGE1_WEIGHTS (the lambdas of script/run_nerf.sh:7-14).
        `self.iteration` (the reference's 1-based iteration, advanced by __call__) drives the depth-variance schedule
        (render.py:202), the orientation term's gate (:191) and, with `iterations` (the run's length, OptimizationParams.iterations),
        the scaling term's schedule (:218).  The terms no run script uses -- depth_smooth, point_entropy, orientation, scaling
        (csrc/supervision.hip) -- are 0 by default; nothing of them is allocated or launched then."""
        super().__init__(params, self._opt_order[:-1], process_group, *_world_of(process_group), bounded, order_stream=None)
        self.w = dict(STAGE1_WEIGHTS)
        if loss_weights:
            self.w.update(loss_weights)
        self.iteration, self.iterations = 0, int(iterations)
        # the terms beside r3dg_stage1_loss: their sum slots follow the six of that kernel (depth smoothness | point entropy,
        # orientation, scaling)
        self._extra_terms = any(self.w[k] != 0.0 for k in ("depth_smooth", "point_entropy", "orientation", "scaling"))
        rate, tail = learning_rates(lr, lrs, lr_rest_scale)
        two_rates = dict(lr_tail=tail("shs"), period=3 * self.M, split=3)
        self.opt = FusedAdam([dict(param=getattr(self, k), lr=rate(k), **(two_rates if k == "shs" else {})) for k in self._opt_order])
        self.stats = None                  # densification statistics (enable_densification)
        self._handle = None                # the gradient all-reduce in flight (data parallel)
        self._allocate()
        self._flag_cur = self._flag        # the overflow flag slot of the last forward

    def _allocate(self):
        """Per-Gaussian work buffers for the current number of Gaussians (again after every densify / prune)."""
        self.P = P = self.xyz.shape[0]
        f = dict(dtype=torch.float32, device=self.dev)
        self.a_scales, self.a_rot = torch.empty(P, 3, **f), torch.empty(P, 4, **f)
        self.a_opacity, self.a_normal = torch.empty(P, 1, **f), torch.empty(P, 3, **f)
        self.features = torch.empty(P, 5, **f)
        self.sums = torch.zeros(10 if self._extra_terms else 6, SUM_SLOTS, **f)          # (R3DG_SUM_SLOTS floats each) l1, normal mse, mask entropy, SSIM(image), edge-aware normal, sqrt depth var
        # the overflow flag of the bounded forward at the end: reduced with the gradients
        order = ("shs", "xyz", "normal", "scaling", "rotation", "opacity", "flag")
        self.grad_flat, self.grads, _ = grad_slab(order, {k: getattr(self, k) for k in order[:-1]}, self.dev)
        self._flag = self.grads.pop("flag")
        self._capacity = None                      # (a new Gaussian count means a new instance count: learn it again)
        self.last_outs = None

    # ---- densification (train.py:158-175; kernels in csrc/densify.hip, host mirror densify.py) ----------------------
    def enable_densification(self):
        """Start collecting the densification statistics: every forward_backward adds its view (add_densification_stats +
        max radii, train.py:160-165), from this rank's own gradients, before the gradient all-reduce is launched."""
        self.stats = densify.DensificationStats(self.P, self.dev)

    def _groups(self):
        return collections.OrderedDict(
            (k, dict(param=getattr(self, k), exp_avg=self.opt.groups[i]["exp_avg"],
                     exp_avg_sq=self.opt.groups[i]["exp_avg_sq"])) for i, k in enumerate(self._opt_order))

    def _drain(self):
        """Complete a gradient all-reduce that is still in flight (data parallel) before its buffers are replaced."""
        if self._handle is not None:
            self._handle.wait()
            self._handle = None

    def _rebind(self, new, new_stats):
        self._drain()
        for i, k in enumerate(self._opt_order):
            setattr(self, k, new[k]["param"])
            g = self.opt.groups[i]
            g["param"], g["exp_avg"], g["exp_avg_sq"] = new[k]["param"], new[k]["exp_avg"], new[k]["exp_avg_sq"]
        self.stats = new_stats
        self._allocate()

    @_in_context
    def densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size, max_grad_normal, percent_dense=0.01,
                          generator=None):
        """GaussianModel.densify_and_prune on the raw parameters and their Adam moments.  Under data parallelism the
        statistics are summed over ranks first (max for the radii) and every rank must pass a generator in the same state,
        so the replicas stay identical."""
        if self.stats is None:
            raise RuntimeError("densify_and_prune: call enable_densification() first")
        self.stats.all_reduce(self.group)
        new, new_stats, info = densify.densify_and_prune(self._groups(), self.stats, max_grad, min_opacity, extent,
                                                         max_screen_size, max_grad_normal, percent_dense, generator=generator)
        self._rebind(new, new_stats)
        return info

    @_in_context
    def prune(self, min_opacity, extent, max_screen_size):
        if self.stats is None:
            raise RuntimeError("prune: call enable_densification() first")
        self.stats.all_reduce(self.group)
        new, new_stats, info = densify.prune(self._groups(), self.stats, min_opacity, extent, max_screen_size)
        self._rebind(new, new_stats)
        return info

    @_in_context
    def reset_opacity(self):
        """GaussianModel.reset_opacity.  The reference swaps in a fresh parameter object, so the optimizer step of the same
        iteration leaves the opacity alone (its .grad is None): the pending opacity gradient is cleared here, which with
        zeroed moments makes that Adam update exactly zero."""
        g = self.opt.groups[self._opt_order.index("opacity")]
        densify.reset_opacity(self.opacity, g["exp_avg"], g["exp_avg_sq"])
        self._drain()
        self.grads["opacity"].zero_()

    def _extra_weights(self, N):
        """The weights of the four terms of csrc/supervision.hip, each divided by the element count of its mean: depth smoothness,
        point entropy, orientation (0 until iteration > orientation_from_iter, render.py:191), scaling (its schedule, :218)."""
        w, P = self.w, max(self.P, 1)
        gate = self.iteration > w["orientation_from_iter"]
        return (w["depth_smooth"] / (3.0 * N), w["point_entropy"] / P, w["orientation"] / P if gate else 0.0,
                scaling_weight(w["scaling"], self.iteration, self.iterations) / P)

    def _weights(self, N):
        """The five weights of r3dg_stage1_loss / loss(), each already divided by the element count of its mean."""
        w = self.w
        return ((1.0 - LAMBDA_DSSIM) * w["l1"] / (3.0 * N), w["mask_entropy"] / N, w["normal_render_depth"] / (3.0 * N),
                w["normal_smooth"] / (3.0 * N), depth_var_weight(w["depth_var"], self.iteration) / N)

    @_in_context
    def forward_backward(self, cam, bg, gt, image_mask=None):
        """`image_mask` [1,H,W] (the view's object mask, scene/cameras.py image_mask; None = all ones)."""
        L = _lib.lib()
        P, dev = self.P, self.dev
        H, W = cam.image_height, cam.image_width
        N = H * W
        stream = _lib.current_stream
        vm = cam.world_view_transform.contiguous()
        campos = cam.camera_center.contiguous()
        empty = torch.Tensor([])
        with torch.cuda.device(dev):
            _lib.check(L.r3dg_stage2_activate(
                stream(), P, self.xyz.data_ptr(), self.scaling.data_ptr(), self.rotation.data_ptr(),
                self.opacity.data_ptr(), self.normal.data_ptr(), None, None, None, self.a_scales.data_ptr(),
                self.a_rot.data_ptr(), self.a_opacity.data_ptr(), self.a_normal.data_ptr(), None, None, None, None, None),
                "stage2_activate")
            self._iter += 1
            flag_cur = self._flag_cur = self._flag_of_iteration()
            use_bounded = self._use_bounded(W, H)
            if not use_bounded:
                flag_cur.zero_()
            pending = rasterizer_ops.rasterize_gaussians_begin(
                bg, self.xyz, self.features, empty, self.a_opacity, self.a_scales, self.a_rot, 1.0, empty, vm,
                cam.full_proj_transform, cam.tanfovx, cam.tanfovy, cam.cx, cam.cy, H, W, self.shs, 3, campos, False,
                True, False, **(dict(capacity=self._capacity, overflow_flag=flag_cur,
                                     overflow_count=self._overflow_count) if use_bounded else {}))
            _lib.check(L.r3dg_stage1_pack_features(stream(), P, self.xyz.data_ptr(), vm.data_ptr(),
                                                   self.a_normal.data_ptr(), self.features.data_ptr()),
                       "stage1_pack_features")
            self.sums.zero_()
            fw = pending.finish()
            R, n_contrib, image, opacity, depth, feature, pseudo_normal, sxyz, weights, radii, geom, binning, img = fw
            # dL_dimage 3 | dL_dopacity 1 | dL_dfeature 5 | SSIM partials 9 | SSIM gradient 3 | edge-aware scratch 6
            g = torch.empty((27, H, W), dtype=torch.float32, device=dev)
            gt_c = gt.contiguous()
            lam = LAMBDA_DSSIM
            _lib.check(L.r3dg_ssim_forward(stream(), W, H, 3, image.data_ptr(), gt_c.data_ptr(), g[9:18].data_ptr(),
                                           self.sums[3].data_ptr()), "ssim_forward")
            _lib.check(L.r3dg_ssim_backward(stream(), W, H, 3, image.data_ptr(), gt_c.data_ptr(), g[9:18].data_ptr(),
                                            -lam * self.w["l1"] / (3.0 * N), g[18:21].data_ptr()), "ssim_backward")
            w_l1, w_ent, w_nrm, w_smooth, w_var = self._weights(N)
            mask_c = None if image_mask is None else image_mask.contiguous()
            _lib.check(L.r3dg_stage1_loss(
                stream(), W, H, image.data_ptr(), opacity.data_ptr(), feature.data_ptr(), pseudo_normal.data_ptr(),
                n_contrib.data_ptr(), gt_c.data_ptr(), _lib.ptr(mask_c), w_l1, w_ent, w_nrm, w_smooth, w_var,
                g[18:21].data_ptr(), g[21:27].data_ptr(), g[0:3].data_ptr(), g[3:4].data_ptr(), g[4:9].data_ptr(),
                self.sums.data_ptr()), "stage1_loss")
            w_ds, w_pe, w_or, w_sc = self._extra_weights(N) if self._extra_terms else (0.0, 0.0, 0.0, 0.0)
            if w_ds != 0.0:
                # behind the loss kernel: adds to the depth map's gradient and the opacity gradient it wrote
                edge = torch.empty((2, H, W), dtype=torch.float32, device=dev)
                _lib.check(L.r3dg_stage1_depth_smooth(
                    stream(), W, H, opacity.data_ptr(), feature.data_ptr(), n_contrib.data_ptr(), gt_c.data_ptr(), w_ds,
                    edge.data_ptr(), g[3:4].data_ptr(), g[4:9].data_ptr(), self.sums[6].data_ptr()), "stage1_depth_smooth")
            bw = rasterizer_ops.rasterize_gaussians_backward(
                bg, self.xyz, self.features, radii, empty, self.a_scales, self.a_rot, 1.0, empty, vm,
                cam.full_proj_transform, cam.tanfovx, cam.tanfovy, g[0:3], g[3:4], empty, g[4:9],        # (empty: no depth gradient)
                self.shs, 3, campos, geom, R, binning, img, True, False, dL_dsh_out=self.grads["shs"],
                # the normal maps carry the two normal terms, depth / depth^2 the variance term
                active_features=(0, 1, 2, 3, 4) if w_var != 0.0 else ((0, 1, 2, 3) if w_ds != 0.0 else (0, 1, 2)))
            dL_dmeans2D, _dcol, dL_dopacity, dL_dmeans3D, dL_dfeatures, _dcov, _dsh, dL_dscales, dL_drot = bw
            gr = self.grads
            if w_pe != 0.0 or w_or != 0.0 or w_sc != 0.0:
                # between the rasterizer backward and the chain rule: adds to the activated-space gradients the latter consumes
                _lib.check(L.r3dg_stage1_gaussian_terms(
                    stream(), P, weights.data_ptr(), self.a_opacity.data_ptr(), self.a_normal.data_ptr(),
                    self.a_scales.data_ptr(), self.xyz.data_ptr(), campos.data_ptr(), w_pe, w_or, w_sc, dL_dopacity.data_ptr(),
                    dL_dfeatures.data_ptr(), dL_dscales.data_ptr(), dL_dmeans3D.data_ptr(), self.sums[7].data_ptr()),
                    "stage1_gaussian_terms")
            _lib.check(L.r3dg_stage1_activate_backward(
                stream(), P, self.xyz.data_ptr(), self.scaling.data_ptr(), self.rotation.data_ptr(),
                self.opacity.data_ptr(), self.normal.data_ptr(), vm.data_ptr(), dL_dfeatures.data_ptr(),
                dL_dscales.data_ptr(), dL_drot.data_ptr(), dL_dopacity.data_ptr(), dL_dmeans3D.data_ptr(),
                gr["xyz"].data_ptr(), gr["scaling"].data_ptr(), gr["rotation"].data_ptr(), gr["opacity"].data_ptr(),
                gr["normal"].data_ptr()), "stage1_activate_backward")
            if self.stats is not None:           # this view's densification statistics, from the LOCAL gradients
                self.stats.add(dL_dmeans2D, gr["normal"], radii, weights, skip_flag=flag_cur)
            self._handle = None
            if self.dp:
                self._handle = torch.distributed.all_reduce(self.grad_flat, group=self.group, async_op=True)
        return self._end_forward_backward(fw, dL_dmeans2D, use_bounded, N)

    def loss(self):
        self.poll_overflow()
        N = self._N
        lam = LAMBDA_DSSIM
        w_l1, w_ent, w_nrm, w_smooth, w_var = self._weights(N)
        w = torch.tensor([w_l1, w_nrm, w_ent, -lam * self.w["l1"] / (3.0 * N), w_smooth, w_var] +
                         (list(self._extra_weights(N)) if self._extra_terms else []), device=self.dev)
        return (self.sums.sum(1) * w).sum() + lam * self.w["l1"]

    @_in_context
    def optimizer_step(self):
        self._drain()
        skip = self._snapshot_flag() if (self.dp and self.bounded) else self._flag_cur
        self.opt.step([self.grads[k] for k in self._opt_order], 1.0 / self.world, skip_flag=skip)

    @_in_context
    def __call__(self, cam, bg, gt, image_mask=None):
        self.iteration += 1
        outs = self.forward_backward(cam, bg, gt, image_mask)
        self.optimizer_step()
        return outs
