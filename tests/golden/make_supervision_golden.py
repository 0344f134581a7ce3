"""Golden fixture for the loss terms no run script switches on, from the REFERENCE'S OWN calculate_loss functions (this container only).

    python tests/golden/make_supervision_golden.py     # needs /root/reference; writes tests/golden/supervision_reference.npz

What runs, unmodified, from /root/reference: calculate_loss of gaussian_renderer/neilf.py (:212-318; the lambda_depth and
lambda_normal_mvs_depth terms) and of gaussian_renderer/render.py (:136-223; lambda_depth_smooth, lambda_point_entropy,
lambda_orientation, lambda_scaling), utils/loss_utils.py, arguments/__init__.py -- imported the way make_pipeline_golden.py
imports them (mocks for the packages this container lacks, train_step.spatial_gradient behind kornia's name).  No rasterizer runs:
the inputs are a hand-made 29 x 37 set of rasterizer outputs (feature image, opacity, n_contrib) and P = 300 per-Gaussian arrays
that hold every edge case the kernels of csrc/supervision.hip branch on; the division `feature / opacity.clamp_min(1e-5) * mask`
that render_view applies before calculate_loss (neilf.py:146-147, render.py:107-108) is applied here to leaf tensors, so autograd
returns the gradients with respect to the RAW maps, which is what the kernels write.  Every tensor is float64 holding float32
values: the fixture is the reference's arithmetic without its rounding.  Each term is evaluated alone (all other lambdas 0, the
rendered image equal to the target so that the L1 / SSIM part vanishes); the fixture stores the weighted term, the lambda, and the
gradients.  Nothing of the reference is copied: inputs and outputs only.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
REF = "/root/reference"

import make_golden as mg  # noqa: E402
import make_pipeline_golden as mp  # noqa: E402

H, W, P = 29, 37, 300
ITERATION, ITERATIONS = 6000, 30_000


def make_maps(seed=7):
    """Rasterizer outputs and per-view supervision maps (float32) with the edge cases of tests/test_supervision_gpu.py."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)
    opacity = (0.05 + 0.95 * r(1, H, W))
    n_contrib = torch.randint(1, 9, (H, W), generator=g, dtype=torch.int32)
    n_contrib[r(H, W) < 0.12] = 0                                   # pixels nothing was blended into
    opacity[0, 3, 4:9] = 3e-6                                       # below the 1e-5 clamp (n_contrib > 0 there)
    n_contrib[3, 4:9] = 2
    opacity[0, 5, 5] = 0.0
    n_contrib[5, 5] = 1
    feat16 = torch.randn(16, H, W, generator=g) * opacity
    feat16[0] = (1.5 + 3.0 * r(H, W)) * opacity[0]                 # depth
    feat16[5:8] = torch.nn.functional.normalize(torch.randn(3, H, W, generator=g), dim=0) * opacity[0] * (0.6 + 0.4 * r(H, W))
    gt_depth = 1.5 + 3.0 * r(1, H, W)
    gt_depth[r(1, H, W) < 0.25] = 0.0                               # pixels the MVS filter rejected
    mask = (1.3 - 1.6 * ((torch.linspace(-1, 1, H)[:, None] ** 2 + torch.linspace(-1, 1, W)[None] ** 2).sqrt())).clamp(0, 1)[None]
    # mask and depth disagree both ways: valid depth outside the mask, no depth inside it
    gt_depth[0, 0, 0:6] = 2.0
    assert float(mask[0, 0, 0:6].max()) == 0.0
    gt_depth[0, 14, 16:20] = 0.0
    assert float(mask[0, 14, 16:20].min()) > 0.0
    # rendered depth == gt_depth EXACTLY (opacity a power of two, so F / o and F * (1 / o) are the same float)
    for (y, x) in ((10, 12), (11, 30), (20, 7)):
        opacity[0, y, x], n_contrib[y, x], feat16[0, y, x], gt_depth[0, y, x] = 0.5, 3, 1.25, 2.5
        assert float(mask[0, y, x]) > 0.0
    mvs_normal = torch.nn.functional.normalize(torch.randn(3, H, W, generator=g), dim=0)
    gt = torch.nn.functional.avg_pool2d(r(3, H, W)[None], 5, 1, 2)[0].clamp(0, 1).contiguous()
    feat5 = torch.cat([feat16[5:8], feat16[0:1], (feat16[0:1] / opacity.clamp_min(1e-5)).square() * opacity * 1.1], 0)
    return dict(opacity=opacity.contiguous(), n_contrib=n_contrib, feat16=feat16.contiguous(), feat5=feat5.contiguous(),
                gt_depth=gt_depth.contiguous(), mask=mask.contiguous(), mvs_normal=mvs_normal.contiguous(), gt=gt)


def make_gaussians(P_, seed=11):
    """Per-Gaussian inputs (float32): blend weights with zeros and values above 1, opacities at both ends, back-facing normals."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)
    weights = 2.5 * r(P_, 1) ** 2
    weights[r(P_, 1) < 0.2] = 0.0
    weights[1], weights[2] = 3.0, 0.0
    opac = 0.02 + 0.96 * r(P_, 1)
    opac[0], opac[1], opac[3], opac[4] = 1e-7, 1.0 - 1e-7, 1e-7, 1.0 - 1e-7
    weights[0], weights[3], weights[4] = 0.7, 1.8, 0.4
    xyz = torch.randn(P_, 3, generator=g)
    campos = torch.tensor([2.9, 1.1, 1.3])
    normal = torch.nn.functional.normalize(torch.randn(P_, 3, generator=g), dim=-1)          # about half face away (n.d < 0)
    scales = torch.exp(-3.0 + 0.7 * torch.randn(P_, 3, generator=g))
    scales[5] = torch.tensor([0.02, 0.02, 0.02])                                             # |s - mean| = 0 on every axis
    return dict(weights=weights.contiguous(), opac=opac.contiguous(), xyz=xyz.contiguous(), campos=campos,
                normal=normal.contiguous(), scales=scales.contiguous())


def main():
    sys.meta_path.append(mg._Finder())
    mp.install_oracle_extensions()
    sys.path.insert(0, REF)
    for p in mg._cpu_factories():
        p.start()
    import importlib
    import gaussian_renderer.neilf as nf
    rd = importlib.import_module("gaussian_renderer.render")
    m, q = make_maps(), make_gaussians(P)
    d = lambda t: t.double()
    out = {"map_" + k: v.numpy() for k, v in m.items()}
    out.update({"pt_" + k: v.numpy() for k, v in q.items()})
    out.update(iteration=ITERATION, iterations=ITERATIONS)
    cam = types.SimpleNamespace(original_image=d(m["gt"]), depth=d(m["gt_depth"]), image_mask=d(m["mask"]),
                                normal=d(m["mvs_normal"]))
    mask_c = (m["n_contrib"] > 0)[None]

    # ---------------- stage 2: lambda_depth, lambda_normal_mvs_depth ----------------
    def stage2(lambdas):
        feature, opacity = d(m["feat16"]).requires_grad_(True), d(m["opacity"]).requires_grad_(True)
        rendered = feature / opacity.clamp_min(1e-5) * mask_c                        # neilf.py:146-147
        results = dict(render=cam.original_image, pbr=cam.original_image, depth=rendered[0:1], normal=rendered[5:8],
                       opacity=opacity, base_color=rendered[8:11], roughness=rendered[11:12], diffuse=rendered[12:15])
        opt, _ = mp.options(True, dict(lambda_pbr=1, **lambdas))
        pc = types.SimpleNamespace(get_xyz=torch.zeros(P, 3))
        loss, tb = nf.calculate_loss(cam, pc, results, opt, None)
        if feature.grad is None and loss.requires_grad:
            loss.backward()
        z = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.numpy().copy()
        return float(loss), tb, z(feature), z(opacity)

    base2 = stage2({})[0]
    for name, lam in (("depth", 0.7), ("normal_mvs_depth", 0.3)):
        loss, tb, gf, go = stage2({"lambda_" + name: lam})
        out.update({"s2_%s_lambda" % name: lam, "s2_%s_term" % name: loss - base2, "s2_%s_tb" % name: tb["loss_" + name],
                    "s2_%s_g_feature" % name: gf, "s2_%s_g_opacity" % name: go})
    # the same depth term without an object mask (image_mask all ones)
    cam.image_mask = torch.ones_like(cam.image_mask)
    loss, tb, gf, go = stage2({"lambda_depth": 0.7})
    out.update(s2_depth_nomask_term=loss - base2, s2_depth_nomask_g_feature=gf, s2_depth_nomask_g_opacity=go)
    cam.image_mask = d(m["mask"])
    sel = (m["mask"] != 0) == (m["gt_depth"] > 0)
    out.update(count_masked=np.int64(sel.sum()), count_nomask=np.int64((m["gt_depth"] > 0).sum()))

    # ---------------- stage 1: lambda_depth_smooth, lambda_point_entropy, lambda_orientation, lambda_scaling ----------------
    def stage1(lambdas):
        leaves = dict(feature=d(m["feat5"]), opacity=d(m["opacity"]), opac=d(q["opac"]), normal=d(q["normal"]), xyz=d(q["xyz"]),
                      scales=d(q["scales"]))
        for t in leaves.values():
            t.requires_grad_(True)
        rendered = leaves["feature"] / leaves["opacity"].clamp_min(1e-5) * mask_c    # render.py:107-108
        directions = torch.nn.functional.normalize(leaves["xyz"] - d(q["campos"]), dim=-1)      # render.py:85-86
        pkg = dict(render=cam.original_image, opacity=leaves["opacity"], depth=rendered[3:4], normal=rendered[0:3],
                   visibility_filter=None, weights=d(q["weights"]), opacities=leaves["opac"], normals=leaves["normal"],
                   directions=directions)
        opt, _ = mp.options(False, dict(iterations=ITERATIONS, **lambdas))
        pc = types.SimpleNamespace(get_xyz=leaves["xyz"], get_scaling=leaves["scales"])
        loss, tb = rd.calculate_loss(cam, pc, pkg, opt, ITERATION)
        if loss.requires_grad:
            loss.backward()
        grads = {k: (np.zeros(tuple(t.shape)) if t.grad is None else t.grad.numpy().copy()) for k, t in leaves.items()}
        return float(loss), tb, grads

    base1 = stage1({})[0]
    for name, lam in (("depth_smooth", 0.4), ("point_entropy", 0.6), ("orientation", 0.8), ("scaling", 0.5)):
        loss, tb, grads = stage1({"lambda_" + name: lam})
        out.update({"s1_%s_lambda" % name: lam, "s1_%s_term" % name: loss - base1})
        out.update({"s1_%s_g_%s" % (name, k): v for k, v in grads.items() if np.abs(v).max() > 0})
    # the orientation term is gated on the iteration (render.py:191)
    opt, _ = mp.options(False, dict(lambda_orientation=0.8))
    out.update(orientation_from_iter=np.int64(opt.lambda_orientation_from_iter))
    path = os.path.join(HERE, "supervision_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes): base losses %.2e %.2e; terms %s" % (
        path, os.path.getsize(path), base2, base1, {k: float(v) for k, v in out.items() if k.endswith("_term")}))


if __name__ == "__main__":
    main()
