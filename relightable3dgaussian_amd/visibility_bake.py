"""Baking traced visibility into the per-Gaussian SH coefficients `visibility_dc` / `visibility_rest` -- the producer of what
checkpoint.py stores, densify clones and prunes and the contract ops shading_ops.render_equation_* consume as
clamp(0.5 + SH, 0, 1).  Restates GaussianModel.finetune_visibility (scene/gaussian_model.py:275-310): per iteration one random
ray per Gaussian in the hemisphere of its normal, traced through the BVH; eval_sh + 0.5 clamped to [0,1]; L1 against the traced
value; one Adam step (lr 1e-2).

The one deliberate difference: the reference takes `visibility_shs_view = self.get_visibility.transpose(1, 2)` ONCE before its
loop (:289); get_visibility is a torch.cat, i.e. a copy, so every iteration predicts from the initial coefficients and the
parameters only drift by lr * sign.  Here every iteration predicts from the live coefficients -- the loop as evidently intended.
One iteration of the two is the same computation (pinned against the unmodified method by tests/golden/visibility_bake_reference.npz).

The trace does not depend on the coefficients, and a Gaussian's fit only on its own rays (the one cross-Gaussian quantity is the
constant 1/P of the mean), so a chunk of T iterations is two launches instead of T rounds of about thirty: ONE trace of the P x T
rays (bvh_ops.trace_hemisphere) and ONE launch that runs the T Adam steps of every Gaussian with its 48 state values in registers
(r3dg_visibility_sh_fit, csrc/visibility_bake.hip).  Single rank only."""

import torch
import torch.nn.functional as F

from . import _lib, bvh_ops

C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
      -0.5900435899266435)


def sh_basis(dirs):
    """The 16 basis values of eval_sh (utils/sh_utils.py:88-116) at unit directions [...,3] -> [...,16]."""
    x, y, z = dirs[..., 0], dirs[..., 1], dirs[..., 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    return torch.stack([torch.full_like(x, C0), -C1 * y, C1 * z, -C1 * x,
                        C2[0] * xy, C2[1] * yz, C2[2] * (2.0 * zz - xx - yy), C2[3] * xz, C2[4] * (xx - yy),
                        C3[0] * y * (3 * xx - yy), C3[1] * xy * z, C3[2] * y * (4 * zz - xx - yy),
                        C3[3] * z * (2 * zz - 3 * xx - 3 * yy), C3[4] * x * (4 * zz - xx - yy), C3[5] * z * (xx - yy),
                        C3[6] * x * (xx - 3 * yy)], -1)


def sh_visibility(coeffs, dirs):
    """clamp(eval_sh(3, coeffs, dirs) + 0.5, 0, 1): coeffs [...,16], dirs [...,3] -> [...]."""
    return ((coeffs * sh_basis(dirs)).sum(-1) + 0.5).clamp(0.0, 1.0)


@torch.no_grad()
def fit_torch(dirs, vis, coeffs, exp_avg=None, exp_avg_sq=None, steps_done=0, lr=1e-2, betas=(0.9, 0.999), eps=1e-8):
    """What r3dg_visibility_sh_fit computes, in plain PyTorch and in the dtype of `coeffs` [P,16]: dirs [T,P,3], vis [T,P] ->
    (coeffs, exp_avg, exp_avg_sq, losses[T]), new tensors.  Gradient of F.l1_loss(vis, clamp(eval_sh + 0.5, 0, 1)) written out
    (sign / P through the clamp's inclusive mask) and torch.optim.Adam's single-tensor step.  The restatement the CPU tests and
    the timing comparison use; the product path never calls it."""
    c = coeffs.clone()
    m = torch.zeros_like(c) if exp_avg is None else exp_avg.clone()
    v = torch.zeros_like(c) if exp_avg_sq is None else exp_avg_sq.clone()
    T, P = vis.shape
    losses = torch.empty(T, dtype=c.dtype, device=c.device)
    b1, b2 = betas
    for t in range(T):
        Y = sh_basis(dirs[t].to(c.dtype))
        x = (c * Y).sum(-1) + 0.5
        vhat = x.clamp(0.0, 1.0)
        target = vis[t].to(c.dtype)
        losses[t] = (target - vhat).abs().mean()
        g = (torch.sign(vhat - target) / P * ((x >= 0) & (x <= 1)).to(c.dtype))[:, None] * Y
        n = steps_done + t + 1
        m.lerp_(g, 1 - b1)
        v.mul_(b2).addcmul_(g, g, value=1 - b2)
        denom = (v.sqrt() / (1 - b2 ** n) ** 0.5).add_(eps)
        c.addcdiv_(m, denom, value=-(lr / (1 - b1 ** n)))
    return c, m, v, losses


class VisibilityBaker:
    """The fit of the 16 visibility SH coefficients of the Gaussians (xyz, scales, rotations, opacity [P,1], normal: activated
    values, float32 on the device), `chunk` iterations per pair of launches.  The tree and the packed records are built as
    train_step.update_visibility_device builds them; `tracer`: the tracer an earlier visibility update over the SAME tensors
    returned -- its tree and records are reused."""

    def __init__(self, xyz, scales, rotations, opacity, normal, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, chunk=64, tracer=None):
        from .bvh import RayTracer
        P, dev = xyz.shape[0], xyz.device
        if P < 1 or not xyz.is_cuda:
            raise RuntimeError("VisibilityBaker: needs at least one Gaussian, on the device")
        self.P, self.dev = P, dev
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.chunk = max(1, min(int(chunk), 0x7fffffff // P))
        with torch.no_grad():
            if tracer is None:
                tracer = RayTracer.from_device_leaves(xyz, scales, rotations)
            if getattr(tracer, "_records", None) is None:
                covs_inv = getattr(tracer, "covs_inv", None)
                if covs_inv is None:
                    from .train_step import inverse_covariance
                    covs_inv = inverse_covariance(scales, rotations)
                arrays = (xyz, covs_inv, opacity[:, 0].contiguous(), normal)
                tracer._records, tracer._records_ref = bvh_ops.trace_records(tracer.tree, tracer.aabb, *arrays), arrays
                tracer._records_key = tuple((t.data_ptr(), t._version, tuple(t.shape)) for t in arrays)
        self.tracer = tracer
        f = dict(dtype=torch.float32, device=dev)
        self.coeffs, self.exp_avg, self.exp_avg_sq = (torch.zeros(P, 16, **f) for _ in range(3))
        self.steps = 0
        self._draws = self._dirs = self._vis = self._partials = None
        self._rows = int(_lib.lib().r3dg_visibility_sh_fit_loss_rows(P))

    def _buffers(self):
        if self._draws is None:
            f = dict(dtype=torch.float32, device=self.dev)
            self._draws, self._dirs = torch.empty(self.chunk, self.P, 3, **f), torch.empty(self.chunk, self.P, 3, **f)
            self._vis = torch.empty(self.chunk, self.P, **f)
            self._partials = torch.empty(self._rows * self.chunk, **f)

    @torch.no_grad()
    def run(self, iterations, raw_dirs=None, generator=None):
        """`iterations` more Adam steps -> their losses mean |v - vhat| [iterations], on the device (nothing is read back here).
        `raw_dirs` [iterations,P,3]: the draws (float32, on the device) instead of torch.randn's (`generator`: its generator)."""
        L = _lib.lib()
        iterations = int(iterations)
        if raw_dirs is not None and (tuple(raw_dirs.shape) != (iterations, self.P, 3) or raw_dirs.dtype != torch.float32 or
                                     not raw_dirs.is_cuda):
            raise RuntimeError("VisibilityBaker.run: raw_dirs must be float32 [iterations,P,3] on the device")
        self._buffers()
        losses = torch.empty(iterations, dtype=torch.float32, device=self.dev)
        for t0 in range(0, iterations, self.chunk):
            T = min(self.chunk, iterations - t0)
            if raw_dirs is None:
                draws = torch.randn((T, self.P, 3), generator=generator, out=self._draws[:T])
            else:
                draws = raw_dirs[t0:t0 + T].contiguous()
            dirs, vis, partials = self._dirs[:T], self._vis[:T], self._partials[:self._rows * T]
            bvh_ops.trace_hemisphere(self.tracer._records, self.tracer.tree, draws, vis, dirs)
            with torch.cuda.device(self.dev):
                _lib.check(L.r3dg_visibility_sh_fit(_lib.current_stream(), self.P, T, self.steps, dirs.data_ptr(), vis.data_ptr(),
                                                    self.lr, self.betas[0], self.betas[1], self.eps, self.coeffs.data_ptr(),
                                                    self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), partials.data_ptr()),
                           "visibility_sh_fit")
            torch.sum(partials.view(self._rows, T), 0, out=losses[t0:t0 + T])
            self.steps += T
        return losses.div_(self.P)

    def coefficients(self):
        """-> (visibility_dc [P,1,1], visibility_rest [P,15,1]), copies."""
        return self.coeffs[:, :1, None].clone(), self.coeffs[:, 1:, None].clone()

    def state(self):
        return dict(coeffs=self.coeffs.clone(), exp_avg=self.exp_avg.clone(), exp_avg_sq=self.exp_avg_sq.clone(), steps=self.steps)

    def load_state(self, state):
        for k in ("coeffs", "exp_avg", "exp_avg_sq"):
            getattr(self, k).copy_(state[k].reshape(self.P, 16))
        self.steps = int(state["steps"])


@torch.no_grad()
def bake_visibility(restored, iterations=1000, **kw):
    """Fits the visibility SH of a stage-2 model and writes `visibility_dc` / `visibility_rest` into it, in place where it already
    holds them, so that a FusedStage2Step built from it -- and checkpoint.capture of that step -- carries them.  `restored`: what
    checkpoint.restore(..., pbr=True) returns, a bench_core.GaussianParams, or a dict of the same raw parameters (xyz, scaling,
    rotation, opacity, normal), on the device.  The geometry is activated as GaussianModel's get_* properties do.  `kw`: of
    VisibilityBaker and of its run().  -> the losses [iterations], on the device."""
    is_map = isinstance(restored, dict)
    get = restored.__getitem__ if is_map else (lambda k: getattr(restored, k))
    run_kw = {k: kw.pop(k) for k in ("raw_dirs", "generator") if k in kw}
    xyz = get("xyz").detach().float().contiguous()
    baker = VisibilityBaker(xyz, torch.exp(get("scaling").detach()).contiguous(), get("rotation").detach().contiguous(),
                            torch.sigmoid(get("opacity").detach()).contiguous(),
                            F.normalize(get("normal").detach(), dim=-1, eps=1e-3).contiguous(), **kw)
    losses = baker.run(iterations, **run_kw)
    for k, t in zip(("visibility_dc", "visibility_rest"), baker.coefficients()):
        old = restored.get(k) if is_map else getattr(restored, k, None)
        if torch.is_tensor(old) and old.shape == t.shape and old.device == t.device:
            old.detach().copy_(t)
        elif is_map:
            restored[k] = t
        else:
            setattr(restored, k, t)
    return losses
