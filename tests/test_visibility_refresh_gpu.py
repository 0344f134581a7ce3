"""The visibility refresh on the device: leaf preparation in one kernel (r3dg_bvh_prepare_leaves), the trace over rays the kernel
generates itself (r3dg_bvh_trace_bundles), train_step.update_visibility_device, FusedStage2Step(device_visibility=True) /
refresh_visibility() and train_loop.train_stage2.

What is exact and what is not: leaf tables, tree, boxes and Morton codes are bit-identical to the PyTorch path; every traced ray
is bit-identical to the existing trace given the direction the kernel generated for it; the directions agree with
sampling.fibonacci_sphere_sampling to a few ulp (bound: 5e-5, what FixedRaySet.try_build uses to recognise the ray set), so
against update_visibility a ray that grazes a box or the 0.9 threshold may land on the other side (capped, see test 4)."""
import math
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import report
from tests.test_visibility_refresh_cpu import occlusion_scene

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _leaf_case(P, seed):
    """Unnormalised quaternions, scales spread over 1e-4 .. 1, coincident Gaussians (identical Morton codes) at P = 1000."""
    g = torch.Generator().manual_seed(seed)
    xyz = torch.rand(P, 3, generator=g) * 2.6 - 1.3
    rot = torch.randn(P, 4, generator=g) * torch.exp(2.0 * torch.randn(P, 1, generator=g))
    scales = torch.pow(10.0, -4.0 * torch.rand(P, 3, generator=g))
    if P >= 1000:
        for t in (xyz, rot, scales):
            t[P // 2:P // 2 + 5] = t[0]
    return xyz.to(DEV), scales.to(DEV), rot.to(DEV)


def _row_error(got, want64):
    """Worst over the rows of: max |error| of the row / max magnitude of the row."""
    err = (got.double() - want64).abs().max(dim=1).values / want64.abs().max(dim=1).values
    return float(err.max())


@pytest.mark.parametrize("P,seed", [(1, 0), (2, 1), (3, 2), (1000, 3)])
def test_leaves_are_those_of_the_pytorch_path(P, seed):
    from relightable3dgaussian_amd import bvh, bvh_ops, train_step
    xyz, scales, rot = _leaf_case(P, seed)
    nodes, aabbs, cinv = bvh_ops.prepare_leaves(xyz, scales, rot)
    n_ref, a_ref = bvh.leaf_boxes(xyz, scales, rot)
    assert nodes.dtype == torch.int32 and torch.equal(nodes, n_ref), "node table initialisation differs"
    bad = (aabbs.view(torch.int32) != a_ref.view(torch.int32)).any(1)
    assert not bad.any(), "%d box rows differ (max |diff| %g)" % (int(bad.sum()), float((aabbs - a_ref).abs().max()))
    a, b = bvh.RayTracer.from_device_leaves(xyz, scales, rot), bvh.RayTracer(xyz, scales, rot)
    assert torch.equal(a.tree, b.tree) and torch.equal(a.morton, b.morton), "tree or Morton codes differ"
    assert torch.equal(a.aabb.view(torch.int32), b.aabb.view(torch.int32)), "boxes differ"
    assert torch.equal(a.covs_inv, cinv)
    # inverse covariance: both paths against a float64 evaluation of the same formula from the same float32 inputs
    want = train_step.inverse_covariance(scales.double(), rot.double())
    e_kernel, e_torch = _row_error(cinv, want), _row_error(train_step.inverse_covariance(scales, rot), want)
    print("P=%d inverse covariance, worst row error / row magnitude: kernel %.3e, train_step.inverse_covariance %.3e" % (
        P, e_kernel, e_torch))
    assert e_kernel <= 2.0 * e_torch


def _trace_case(P, K, seed=0):
    """A Gaussian set (synthetic.make_scene: activated values) whose first normals are the special cases of rotation_between_z:
    exactly +z, exactly -z (the -I branch), within 1 degree of -z (the 1 / (n_z + 1) terms blow up), and -- all of them --
    unnormalised inputs passed through get_normal."""
    from relightable3dgaussian_amd import synthetic as syn
    sc = syn.make_scene(P=max(P, 4), seed=seed, stage2=False, scale_log_mean=-2.6)
    d = {k: v[:P].to(DEV).contiguous() for k, v in sc.items() if torch.is_tensor(v)}
    g = torch.Generator().manual_seed(100 + seed)
    raw = d["normal"].cpu() * torch.exp(torch.randn(P, 1, generator=g))                   # unnormalised
    t = math.radians(0.7)
    special = [(0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (math.sin(t), 0.0, -math.cos(t)), (0.0, -3.0 * math.sin(t / 2), -3.0 * math.cos(t / 2))]
    for i, n in enumerate(special[:P] if P >= 3 else special[1:1 + P]):
        raw[i] = torch.tensor(n)
    d["normal"] = F.normalize(raw.to(DEV), dim=-1, eps=1e-3)                              # GaussianModel.get_normal
    return d


_TRACED = {}


def _traced(P, K):
    """One device trace per case, shared by the direction and the trace tests (results are never modified)."""
    from relightable3dgaussian_amd import bvh, bvh_ops, sampling
    if (P, K) not in _TRACED:
        d = _trace_case(P, K, seed=P % 7)
        tracer = bvh.RayTracer.from_device_leaves(d["xyz"], d["scales"], d["rotations"])
        op = d["opacity"][:, 0].contiguous()
        records = bvh_ops.trace_records(tracer.tree, tracer.aabb, d["xyz"], tracer.covs_inv, op, d["normal"])
        zs = sampling.fibonacci_z_samples(K, DEV)[0].t().contiguous()
        vis = torch.full((P, K), -7.0, device=DEV)
        cnt = torch.full((P, K), -7, dtype=torch.int32, device=DEV)
        dirs = torch.full((P, K, 3), float("nan"), device=DEV)
        overflow = bvh_ops.trace_bundles(records, tracer.tree, zs, vis, 0, P, contributes=cnt, dirs_out=dirs)
        torch.cuda.synchronize()
        _TRACED[(P, K)] = dict(d=d, tracer=tracer, op=op, records=records, zs=zs, vis=vis, cnt=cnt, dirs=dirs, overflow=int(overflow))
    return _TRACED[(P, K)]


@pytest.mark.parametrize("P,K", [(1, 4), (3, 5), (257, 7), (5000, 64)])
def test_generated_directions_are_the_fibonacci_set(P, K):
    from relightable3dgaussian_amd import sampling
    from relightable3dgaussian_amd.shading_ops import FixedRaySet
    c = _traced(P, K)
    want, _ = sampling.fibonacci_sphere_sampling(c["d"]["normal"], K)
    worst = float((c["dirs"] - want).abs().max())
    print("P=%d K=%d  max |direction component - fibonacci_sphere_sampling| = %.3e  (|d| - 1: %.1e)" % (
        P, K, worst, float((c["dirs"].norm(dim=-1) - 1).abs().max())))
    assert torch.isfinite(c["dirs"]).all() and worst <= 5e-5
    built = FixedRaySet.try_build(c["d"]["normal"], c["dirs"])
    if K % 4 == 0:
        assert built is not None and FixedRaySet.last_mismatch <= 5e-5
    else:
        # (try_build refuses every K that is no multiple of 4 before it looks at a direction: the kernels it builds for do not
        # take such a K.  What it would have compared is what was compared above.)
        assert built is None


@pytest.mark.parametrize("P,K", [(1, 4), (2, 5), (3, 5), (257, 7), (5000, 64)])
def test_bundle_trace_equals_the_array_trace_on_its_own_directions(P, K):
    """(2,5): a ray count that is no multiple of 8 (the per-XCD queue split); (257,7): a bundle across a 256-ray block."""
    from relightable3dgaussian_amd import bvh_ops
    c = _traced(P, K)
    d, tracer = c["d"], c["tracer"]
    assert (c["vis"] != -7.0).all() and (c["cnt"] != -7).all(), "a row was not written"
    res = tracer.trace_visibility(d["xyz"][:, None].expand_as(c["dirs"]), c["dirs"], d["xyz"], tracer.covs_inv, c["op"],
                                  d["normal"])
    torch.cuda.synchronize()
    print("P=%d K=%d  visible %.3f  stack overflow %d / %d" % (P, K, float((c["vis"] > 0).float().mean()), c["overflow"],
                                                              int(bvh_ops.trace_bvh_opacity.last_overflow)))
    assert torch.equal(c["vis"].view(torch.int32), res["visibility"][..., 0].view(torch.int32)), "visibility differs"
    assert torch.equal(c["cnt"], res["contribute"][..., 0]), "hit counts differ"
    assert c["overflow"] == int(bvh_ops.trace_bvh_opacity.last_overflow)
    # two calls over the two halves of the leaf slots fill one buffer like one call (contributes / dirs_out not wanted)
    vis2 = torch.full((P, K), -7.0, device=DEV)
    bvh_ops.trace_bundles(c["records"], tracer.tree, c["zs"], vis2, 0, P // 2)
    if P // 2 > 0:
        rows = tracer.tree[P - 1:, 3].long()[:P // 2]
        untouched = torch.ones(P, dtype=torch.bool, device=DEV)
        untouched[rows] = False
        assert (vis2[untouched] == -7.0).all(), "rows of leaves outside the range were written"
    bvh_ops.trace_bundles(c["records"], tracer.tree, c["zs"], vis2, P // 2, P)
    torch.cuda.synchronize()
    assert torch.equal(vis2.view(torch.int32), c["vis"].view(torch.int32)), "two half ranges differ from one call"


def test_bundle_trace_rejects_bad_arguments():
    from relightable3dgaussian_amd import bvh_ops
    c = _traced(3, 5)
    vis = torch.zeros(3, 5, device=DEV)
    for lo, hi in ((-1, 2), (2, 1), (0, 4)):
        with pytest.raises(RuntimeError, match="bad leaf range"):
            bvh_ops.trace_bundles(c["records"], c["tracer"].tree, c["zs"], vis, lo, hi)
    bvh_ops.trace_bundles(c["records"], c["tracer"].tree, c["zs"], vis, 2, 2)                  # empty range: no launch
    torch.cuda.synchronize()
    assert (vis == 0).all()


def test_device_update_against_the_existing_update():
    """P = 5000, K = 64 on the occlusion scene (tests/test_visibility_refresh_cpu.py, where the CPU trace bounds what direction
    noise of 5e-5 does to it).  Mean |difference| <= 2e-5, the tolerance the project holds its trace to; at most 1 % of the
    entries beyond 2e-5 -- rays whose slab or leaf decision flips under a last-bit change of the direction, each of them exact
    for its own direction by the test above."""
    from relightable3dgaussian_amd import train_step
    sc = {k: v.to(DEV) for k, v in occlusion_scene().items()}
    K = 64
    args = (sc["xyz"], sc["scales"], sc["rotations"], sc["opacity"], sc["normal"], K)
    vis_ref, dirs_ref, areas_ref, _ = train_step.update_visibility(*args)
    vis, dirs, tracer = train_step.update_visibility_device(*args)
    assert dirs is None and vis.shape == vis_ref.shape == (5000, K, 1)
    vis_d, dirs_d, _ = train_step.update_visibility_device(*args, want_dirs=True)
    torch.cuda.synchronize()
    assert torch.equal(vis_d, vis), "want_dirs changes the result"
    diff = (vis - vis_ref).abs()
    beyond = int((diff > 2e-5).sum())
    print("occluded %.3f; mean |diff| %.3e; entries beyond 2e-5: %d of %d (%.4f %%), class flips %d; max |dir diff| %.3e" % (
        float((vis_ref == 0).float().mean()), float(diff.mean()), beyond, diff.numel(), 100.0 * beyond / diff.numel(),
        int(((vis == 0) != (vis_ref == 0)).sum()), float((dirs_d - dirs_ref).abs().max())))
    assert float(diff.mean()) <= 2e-5
    assert beyond <= 0.01 * diff.numel()
    assert float((dirs_d - dirs_ref).abs().max()) <= 5e-5 and float(areas_ref.min()) == float(areas_ref.max())


def _sharded_worker(rank, world, port, out_dir):
    import os
    import torch.distributed as dist
    from relightable3dgaussian_amd import train_step
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    d = _trace_case(3001, 12, seed=4)
    vis, dirs, _ = train_step.update_visibility_device(d["xyz"], d["scales"], d["rotations"], d["opacity"], d["normal"], 12,
                                                       want_dirs=rank == 1)
    torch.save((vis.cpu(), None if dirs is None else dirs.cpu()), os.path.join(out_dir, "vis%d.pt" % rank))
    dist.destroy_process_group()


def test_sharded_device_update_equals_the_single_process_update(tmp_path):
    """Two ranks on the one test GPU (gloo, as tests/test_fused_dp_gpu.py): rank r traces the leaf slots [r*per, (r+1)*per) -- P
    odd, so the last block is short -- and one all-gather assembles the rows.  Every ray is the same ray whoever traces it: the
    replicas' visibility is bit-identical to a single process's."""
    import socket
    import torch.multiprocessing as mp
    from relightable3dgaussian_amd import train_step
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    mp.spawn(_sharded_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    d = _trace_case(3001, 12, seed=4)
    vis, dirs, _ = train_step.update_visibility_device(d["xyz"], d["scales"], d["rotations"], d["opacity"], d["normal"], 12,
                                                       want_dirs=True)
    for rank in range(2):
        got_vis, got_dirs = torch.load(str(tmp_path / ("vis%d.pt" % rank)))
        assert torch.equal(got_vis.view(torch.int32), vis.cpu().view(torch.int32)), "rank %d" % rank
        if rank == 1:        # (under a group the directions are evaluated in PyTorch for all rows)
            assert float((got_dirs - dirs.cpu()).abs().max()) <= 5e-5
        else:
            assert got_dirs is None


# ---- the step object ----------------------------------------------------------------------------------------------------------
def _step_scene(P=2000, res=64, seed=11):
    from relightable3dgaussian_amd import synthetic as syn
    from relightable3dgaussian_amd.bench_core import GaussianParams, render_stage1
    torch.manual_seed(1234)
    scene = syn.make_scene(P=P, seed=seed, stage2=True, scale_log_mean=-3.2)
    cams = [c.to(DEV) for c in syn.orbit_cameras(4, width=res, height=res)]
    bg = torch.tensor([1.0, 0.6, 0.3], device=DEV)
    params = GaussianParams(scene, DEV, True)
    with torch.no_grad():
        teacher = GaussianParams(syn.make_scene(P=P, seed=seed, stage2=False, scale_log_mean=-3.2), DEV, False)
        teacher.features_dc.add_(0.2 * torch.randn_like(teacher.features_dc))
        gts = [render_stage1(teacher, c, bg)[2].clone() for c in cams]
    return params, cams, bg, gts


_GRADS = ("xyz", "normal", "scaling", "rotation", "opacity", "shs", "base_color", "roughness", "incidents", "env")


def _same_iteration(a, b, what):
    """Loss and gradients of two steps' last forward_backward, within the tolerances tests/test_fused_step_gpu.py holds two
    schedules / shading paths of one iteration to: loss rtol 2e-5, gradients 1e-4 of the array's scale."""
    la, lb = float(a.loss()), float(b.loss())
    print("%s: loss %.8f vs %.8f" % (what, la, lb))
    assert np.allclose(la, lb, rtol=2e-5), (what, la, lb)
    for k in _GRADS:
        ok, msg = report("%s %s" % (what, k), a.grads[k], b.grads[k], 1e-4, 1e-12)
        print(msg)
        assert ok, msg


def _params_of(step):
    """A parameter holder with clones of a step's current raw parameters."""
    inc = step.incidents
    return types.SimpleNamespace(features_dc=step.shs[:, :1].clone(), features_rest=step.shs[:, 1:].clone(),
                                 incidents_dc=inc[:, :1].clone(), incidents_rest=inc[:, 1:].clone(),
                                 **{k: getattr(step, k).clone() for k in ("xyz", "normal", "scaling", "rotation", "opacity",
                                                                          "base_color", "roughness", "env")})


def _supported(K):
    from relightable3dgaussian_amd.shading_ops import FixedRaySet
    return FixedRaySet.supported(K, 16, 16, 32)


@pytest.mark.parametrize("K", [16, 6])
def test_step_built_on_the_device_path_equals_the_default_step(K):
    """K = 16: the fixed-ray-set kernels apply and no direction tensor may ever exist; K = 6 (no multiple of 4): they do not, the
    device trace hands the directions to the general kernels."""
    from relightable3dgaussian_amd.fused_step import FusedStage2Step
    params, cams, bg, gts = _step_scene()
    assert _supported(16) and not _supported(6)
    ref = FusedStage2Step(params, K, lr=1e-3)
    dev = FusedStage2Step(params, K, lr=1e-3, device_visibility=True)
    for s in (ref, dev):
        s.forward_backward(cams[0], bg, gts[0])
    torch.cuda.synchronize()
    if _supported(K):
        assert dev.incident_dirs is None and dev.incident_areas is None and dev._frs is not None and ref._frs is not None
        assert dev._taps is None
    else:
        assert dev._frs is None and dev.incident_dirs.shape == (dev.P, K, 3) and dev.incident_areas.shape == (dev.P, K, 1)
        assert float((dev.incident_dirs - ref.incident_dirs).abs().max()) <= 5e-5
    flips = int(((dev.visibility == 0) != (ref.visibility == 0)).sum())
    print("K=%d visibility: mean |diff| %.3e, class flips %d of %d" % (
        K, float((dev.visibility - ref.visibility).abs().mean()), flips, ref.visibility.numel()))
    _same_iteration(dev, ref, "device_visibility K=%d" % K)


@pytest.mark.parametrize("device_visibility", [True, False])
def test_refresh_visibility_retraces_and_leaves_the_optimizer_alone(device_visibility):
    from relightable3dgaussian_amd.fused_step import FusedStage2Step
    K = 16
    params, cams, bg, gts = _step_scene()
    step = FusedStage2Step(params, K, lr=1e-3, device_visibility=device_visibility)
    for it in range(3):
        step(cams[it], bg, gts[it])
    vis_before = step.visibility
    with torch.no_grad():
        g = torch.Generator(device=DEV).manual_seed(3)
        rows = torch.randperm(step.P, generator=g, device=DEV)[:step.P // 10]
        step.normal[rows] = torch.randn(rows.numel(), 3, generator=g, device=DEV)
    step.refresh_activations()
    torch.cuda.synchronize()
    assert not torch.equal(step._ray_normals, step.a_normal), "the snapshot normals should be stale now"
    names = ("xyz", "normal", "scaling", "rotation", "opacity", "shs", "base_color", "roughness", "env")
    before = {k: getattr(step, k).clone() for k in names}
    before["incidents"] = step.incidents.clone()
    moments = [(g_["exp_avg"].clone(), g_["exp_avg_sq"].clone()) for g_ in step.opt.groups]
    count, refreshes = step.opt.step_count, step.visibility_refreshes
    step.refresh_visibility()
    torch.cuda.synchronize()
    assert step.visibility_refreshes == refreshes + 1 and step.opt.step_count == count == 3
    assert torch.equal(step._ray_normals, step.a_normal)
    assert step.incident_dirs is None and step._frs is not None and step._pre_rotated is None
    assert step.visibility is not vis_before and not torch.equal(step.visibility, vis_before)
    for k in names:
        assert torch.equal(getattr(step, k), before[k]), "parameter %s changed" % k
    assert torch.equal(step.incidents, before["incidents"])
    for g_, (m, v) in zip(step.opt.groups, moments):
        assert torch.equal(g_["exp_avg"], m) and torch.equal(g_["exp_avg_sq"], v), "Adam moments changed"
    # the next iteration is the first iteration of a fresh step built from the same parameters
    fresh = FusedStage2Step(_params_of(step), K, lr=1e-3)
    for s in (step, fresh):
        s.forward_backward(cams[3], bg, gts[3])
    torch.cuda.synchronize()
    _same_iteration(step, fresh, "after refresh (device_visibility=%s)" % device_visibility)


def test_stage2_loop_refreshes_at_the_interval():
    from relightable3dgaussian_amd import train_loop
    params, cams, bg, gts = _step_scene()
    seen = []
    step, history = train_loop.train_stage2(params, cams, gts, bg, extent=2.6, sample_num=16, iterations=12,
                                            visibility_interval=5, on_iteration=lambda it, s: seen.append(float(s.loss())))
    assert [(i, e, n) for i, e, n in history if e == "visibility"] == [(5, "visibility", step.P), (10, "visibility", step.P)]
    assert len(seen) == 12 and all(math.isfinite(x) for x in seen), seen
    assert step.visibility_refreshes == 2 and step.device_visibility and step.incident_dirs is None
    assert step.opt.step_count + step.dropped_steps == 12
    xyz_lr = step.opt.groups[step._opt_order.index("xyz")]["lr"]
    assert math.isclose(xyz_lr, train_loop.position_lr(12, 0.00016 * 2.6, 0.0000016 * 2.6), rel_tol=1e-12)
    kept = []
    step0, history0 = train_loop.train_stage2(params, cams, gts, bg, extent=2.6, sample_num=16, iterations=12,
                                              on_iteration=lambda it, s: kept.append(s.visibility))
    assert not [h for h in history0 if h[1] == "visibility"] and step0.visibility_refreshes == 0
    assert all(v is kept[0] for v in kept)
    from relightable3dgaussian_amd.fused_step import FusedStage2Step
    built = FusedStage2Step(params, 16)
    torch.cuda.synchronize()
    assert torch.equal(step0.visibility, built.visibility), "without an interval the visibility is the one from construction"
