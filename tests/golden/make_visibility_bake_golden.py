"""Fixture of the visibility bake from the REFERENCE'S OWN Python (this container only), with the machinery of
make_pipeline_golden.py: the reference's GaussianModel, RayTracer, eval_sh over the oracle-backed extension modules, on the CPU.

    python tests/golden/make_visibility_bake_golden.py     # needs /root/reference; writes tests/golden/visibility_bake_reference.npz

What runs:
    GaussianModel.finetune_visibility(iterations=1), UNMODIFIED (scene/gaussian_model.py:275-310)      -> coeffs_unmodified_1
    the loop as evidently intended -- the prediction taken from the LIVE coefficients instead of the copy :289 makes before the
    loop -- built from the reference's own eval_sh, RayTracer.trace_visibility, F.l1_loss and torch.optim.Adam over the same
    draws (torch.randn_like, recorded by wrapping it), the SH / Adam part in float32 and again in float64: final coefficients,
    moments and per-iteration losses of both, spread = max |c32 - c64|, and the knife-edge mask (a Gaussian that at any
    iteration, in either precision, has |x| or |x - 1| below 1e-5, or |vhat - v| below 1e-5 while the clamp passes the gradient:
    a last-bit difference may flip its gradient.  A saturated prediction that meets its target -- x > 1 with v = 1, vhat - v = 0
    exactly, the ordinary end state of an unoccluded Gaussian -- has gradient 0 whatever the sign says and is no knife edge).
The generator asserts what the tests rely on: knife-edge share <= 2 %, both clamp branches taken, visible fraction in [0.1, 0.9].
Data only: inputs and recorded results."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
REF = "/root/reference"

import make_golden as mg  # noqa: E402
import make_pipeline_golden as mpg  # noqa: E402

P, T, SEED, LR, EDGE = 333, 96, 7, 1e-2, 1e-5


def main():
    sys.meta_path.append(mg._Finder())
    mpg.install_oracle_extensions()
    sys.path.insert(0, REF)
    for p in mg._cpu_factories():
        p.start()
    from bvh import RayTracer
    from scene.gaussian_model import GaussianModel
    from utils.sh_utils import eval_sh

    raw = mpg.make_inputs(P, 32, 5, True)[0]
    pc = mpg.to_model(GaussianModel, raw, True)
    for k in ("_xyz", "_normal", "_scaling", "_rotation", "_opacity"):        # (the CPU oracle extension calls .numpy() on them)
        getattr(pc, k).requires_grad_(False)
    pc._visibility_dc = torch.nn.Parameter(torch.zeros(P, 1, 1))
    pc._visibility_rest = torch.nn.Parameter(torch.zeros(P, 15, 1))

    draws = []
    randn_like = torch.randn_like

    def recording(x, *a, **kw):
        z = randn_like(x, *a, **kw)
        draws.append(z.clone())
        return z
    torch.randn_like = recording
    torch.manual_seed(SEED)
    pc.finetune_visibility(iterations=1)
    torch.randn_like = randn_like
    assert len(draws) == 1
    unmodified_1 = torch.cat([pc._visibility_dc, pc._visibility_rest], 1)[:, :, 0].detach().clone()

    # the same draws, T of them, and their traces
    xyz, normal, opacity = pc.get_xyz, pc.get_normal, pc.get_opacity[:, 0]
    scaling, rotation, cov_inv = pc.get_scaling, pc.get_rotation, pc.get_inverse_covariance()
    tracer = RayTracer(xyz, scaling, rotation)
    torch.manual_seed(SEED)
    raw_dirs = torch.stack([torch.randn_like(xyz) for _ in range(T)])
    assert torch.equal(raw_dirs[0], draws[0])
    dirs, vis = [], []
    for t in range(T):
        d = F.normalize(raw_dirs[t], dim=-1)
        mask = (d * normal).sum(-1) < 0
        d[mask] *= -1
        dirs.append(d)
        vis.append(tracer.trace_visibility(xyz, d, xyz, cov_inv, opacity, normal)["visibility"][:, 0])
    dirs, vis = torch.stack(dirs), torch.stack(vis)

    def intended(dtype):
        dc = torch.nn.Parameter(torch.zeros(P, 1, 1, dtype=dtype))
        rest = torch.nn.Parameter(torch.zeros(P, 15, 1, dtype=dtype))
        opt = torch.optim.Adam([{"params": [dc], "lr": LR}, {"params": [rest], "lr": LR}])
        losses, knife = [], torch.zeros(P, dtype=torch.bool)
        lo = hi = 0
        for t in range(T):
            view = torch.cat([dc, rest], 1).transpose(1, 2)
            x = eval_sh(3, view, dirs[t].to(dtype)) + 0.5
            sample_vis = torch.clamp(x, 0.0, 1.0)
            target = vis[t].to(dtype)[:, None]
            loss = F.l1_loss(target, sample_vis)
            with torch.no_grad():
                inside = (x >= 0) & (x <= 1)
                knife |= ((x.abs() < EDGE) | ((x - 1).abs() < EDGE) | (inside & ((sample_vis - target).abs() < EDGE)))[:, 0]
                lo, hi = lo + int((x < 0).sum()), hi + int((x > 1).sum())
            loss.backward()
            opt.step()
            opt.zero_grad()
            losses.append(float(loss.detach()))
        cat = lambda a, b: torch.cat([a, b], 1)[:, :, 0].detach().clone()
        return dict(coeffs=cat(dc, rest), exp_avg=cat(opt.state[dc]["exp_avg"], opt.state[rest]["exp_avg"]),
                    exp_avg_sq=cat(opt.state[dc]["exp_avg_sq"], opt.state[rest]["exp_avg_sq"]),
                    losses=np.array(losses, np.float64), knife=knife, below=lo, above=hi)

    r32, r64 = intended(torch.float32), intended(torch.float64)
    # one iteration of the intended loop IS the unmodified method's (the copy :289 takes is still current)
    dc = torch.nn.Parameter(torch.zeros(P, 16, 1))
    opt = torch.optim.Adam([dc], lr=LR)
    F.l1_loss(vis[0][:, None], torch.clamp(eval_sh(3, dc.transpose(1, 2), dirs[0]) + 0.5, 0.0, 1.0)).backward()
    opt.step()
    assert torch.equal(dc[:, :, 0].detach(), unmodified_1), "one intended iteration differs from the unmodified method"

    knife = r32["knife"] | r64["knife"]
    spread = float((r32["coeffs"].double() - r64["coeffs"]).abs().max())
    visible = float((vis > 0).float().mean())
    print("P=%d T=%d lr=%g: knife-edge %d of %d; x < 0: %d / %d, x > 1: %d / %d (float32 / float64); visible fraction %.3f; "
          "spread %.3e (outside the mask %.3e); max |c64| %.3f; loss %.4f -> %.4f" % (
              P, T, LR, int(knife.sum()), P, r32["below"], r64["below"], r32["above"], r64["above"], visible, spread,
              float((r32["coeffs"].double() - r64["coeffs"]).abs()[~knife].max()), float(r64["coeffs"].abs().max()),
              r64["losses"][0], r64["losses"][-1]))
    assert int(knife.sum()) <= 0.02 * P, "too many knife-edge Gaussians"
    assert min(r32["below"], r64["below"], r32["above"], r64["above"]) > 0, "a clamp branch was never taken"
    assert 0.1 <= visible <= 0.9
    assert torch.isfinite(r64["coeffs"]).all()

    out = {("raw_" + k): raw[k].numpy() for k in ("xyz", "normal", "scaling", "rotation", "opacity")}
    out.update(xyz=xyz.detach().numpy(), normal=normal.detach().numpy(), scales=scaling.detach().numpy(),
               rotations=rotation.detach().numpy(), opacity=pc.get_opacity.detach().numpy(),
               draws=raw_dirs.numpy(), visibility=vis.numpy(), coeffs_unmodified_1=unmodified_1.numpy(),
               lr=np.float64(LR), betas=np.array([0.9, 0.999], np.float64), eps=np.float64(1e-8), edge=np.float64(EDGE),
               spread=np.float64(spread), knife_edge=knife.numpy(), seed=np.int64(SEED))
    for tag, r in (("32", r32), ("64", r64)):
        out.update({"coeffs" + tag: r["coeffs"].numpy(), "exp_avg" + tag: r["exp_avg"].numpy(),
                    "exp_avg_sq" + tag: r["exp_avg_sq"].numpy(), "losses" + tag: r["losses"]})
    path = os.path.join(HERE, "visibility_bake_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
