"""Host side of the on-device visibility refresh (no GPU): the two C ABI entry points as the header declares them and as the
binding reads them, the stage-2 fields of train_loop.Schedule, the refresh iterations train_stage2 emits -- and the occlusion
scene of tests/test_visibility_refresh_gpu.py, with the check that scene has to pass before the GPU test may use it."""
import ctypes as C
import math
import re

import numpy as np
import torch

_i, _f, _p = C.c_int, C.c_float, C.c_void_p


def test_header_declares_and_binding_types_the_two_entry_points():
    from relightable3dgaussian_amd import _abi
    header = re.sub(r"\s+", " ", open(_abi.HEADER).read())
    assert ("int r3dg_bvh_prepare_leaves(void* stream, int P, const float* d_means3D, const float* d_scales, "
            "const float* d_rotations, int32_t* d_nodes, float* d_aabbs, float* d_covs3D_inv);") in header
    assert ("int r3dg_bvh_trace_bundles(void* stream, int num_gaussians, int K, void* d_records, const int32_t* d_nodes, "
            "const float* d_zsamples, int leaf_lo, int leaf_hi, float origin_offset, float* d_visibility, "
            "int32_t* d_num_contributes, float* d_dirs_out, int32_t* d_stack_overflow);") in header
    assert _abi.prototypes["r3dg_bvh_prepare_leaves"] == (_i, [_p, _i] + [_p] * 6)
    assert _abi.prototypes["r3dg_bvh_trace_bundles"] == (_i, [_p, _i, _i, _p, _p, _p, _i, _i, _f, _p, _p, _p, _p])


def test_schedule_carries_the_stage2_rates_of_the_reference():
    """arguments/__init__.py:87-96."""
    from relightable3dgaussian_amd import train_loop
    sch = train_loop.Schedule()
    want = dict(env_lr=0.1, env_rest_lr=0.001, base_color_lr=0.01, roughness_lr=0.01, light_lr=0.001, light_rest_lr=0.0001,
                light_init=3.0, visibility_lr=0.0025, visibility_rest_lr=0.0025)
    assert {k: getattr(sch, k) for k in want} == want
    assert train_loop.Schedule(light_lr=0.5).light_lr == 0.5 and sch.sh_lr == 0.0025          # (overrides, stage-1 fields kept)
    lrs = train_loop.stage2_learning_rates(sch, extent=2.0)
    assert lrs == dict(xyz=0.00032, normal=0.01, scaling=0.005, rotation=0.001, opacity=0.05, shs=0.0025, shs_rest=0.0025 / 20.0,
                       base_color=0.01, roughness=0.01, incidents=0.001, incidents_rest=0.0001, env=0.1)
    # a negative light_rest_lr means light_lr / 20 (scene/gaussian_model.py:476-477)
    assert train_loop.stage2_learning_rates(train_loop.Schedule(light_rest_lr=-1.0), 1.0)["incidents_rest"] == 0.001 / 20.0


def test_refresh_iterations_of_the_stage2_loop():
    from relightable3dgaussian_amd.train_loop import visibility_refresh_iterations
    assert visibility_refresh_iterations(12, 5) == [5, 10]
    assert visibility_refresh_iterations(12, 0) == []
    assert visibility_refresh_iterations(10, 5) == [5, 10] and visibility_refresh_iterations(4, 5) == []
    assert visibility_refresh_iterations(3, 1) == [1, 2, 3]


# ---- the occlusion scene of the GPU comparison with the existing path ----------------------------------------------------------
def occlusion_scene(P=5000, seed=21):
    """An open shell of mostly opaque, inward-facing Gaussians (the part z < 0.8 of the unit sphere) around a small sphere of
    outward-facing ones: rays from the inner sphere run into the shell, rays from the shell into the inner sphere or the far
    side of the shell, and both escape through the opening -- real occlusion, partial transmittance and free rays in one scene.
    (A ray that only touches the 3-sigma boxes of Gaussians it passes is attenuated by up to 1 % each, and such a value moves
    with the direction CONTINUOUSLY: the wider the opening, the more of those -- at z < 0.35 direction noise of 5e-5 already
    moves 1.6 % of all rays by more than 2e-5, see the test below.)  Activated values as CPU float32 tensors."""
    g = torch.Generator().manual_seed(seed)
    n_in = P // 3
    n_sh = P - n_in
    d = torch.randn(4 * n_sh, 3, generator=g)
    d = d / d.norm(dim=-1, keepdim=True)
    d = d[d[:, 2] < 0.8][:n_sh]
    assert d.shape[0] == n_sh
    e = torch.randn(n_in, 3, generator=g)
    e = e / e.norm(dim=-1, keepdim=True)
    xyz = torch.cat([d, 0.4 * e]) + 0.004 * torch.randn(P, 3, generator=g)
    normal = torch.cat([-d, e])
    normal = torch.nn.functional.normalize(normal + 0.05 * torch.randn(P, 3, generator=g), dim=-1)
    log_s = math.log(0.04) + 0.2 * torch.randn(P, 3, generator=g)
    log_s[torch.arange(P), torch.randint(0, 3, (P,), generator=g)] += math.log(0.5)
    rot = torch.randn(P, 4, generator=g)
    rot = rot / rot.norm(dim=-1, keepdim=True)
    opacity = torch.sigmoid(2.5 + 1.5 * torch.randn(P, 1, generator=g))
    perm = torch.randperm(P, generator=g)                         # (index order is not spatial)
    return {k: v[perm].contiguous() for k, v in dict(xyz=xyz, normal=normal, scales=torch.exp(log_s), rotations=rot,
                                                     opacity=opacity).items()}


def test_occlusion_scene_keeps_the_reference_formulation_inside_the_cap():
    """The GPU test allows 1 % of the P x K visibilities to differ by more than 2e-5 between update_visibility and
    update_visibility_device, whose float32 directions differ by at most 5e-5 per component.  The cap must be a property of the
    SCENE, not of the code under test: the reference formulation alone (the CPU trace of oracle/bvh.py, same tree, same origins
    rule) traces the directions and the directions perturbed by uniform noise of 5e-5 per component -- a hundred times what two
    fp32 evaluations of one formula differ by -- and the changed rays must stay inside the cap.  Also: the scene occludes."""
    from oracle import bvh as ob
    from relightable3dgaussian_amd import sampling, train_step
    K = 64
    sc = occlusion_scene()
    P = sc["xyz"].shape[0]
    nodes, aabbs = ob.leaf_boxes(sc["xyz"].numpy(), sc["scales"].numpy(), sc["rotations"].numpy())
    nodes, aabbs, _ = ob.create_bvh(nodes, aabbs)
    cinv = train_step.inverse_covariance(sc["scales"], sc["rotations"]).numpy()
    dirs = sampling.fibonacci_sphere_sampling(sc["normal"], K)[0]
    g = torch.Generator().manual_seed(5)
    noisy = dirs + (torch.rand(dirs.shape, generator=g) * 2 - 1) * 5e-5
    vis = []
    for d in (dirs, noisy):
        o = sc["xyz"][:, None, :] + d * 0.05
        vis.append(ob.trace_bvh_opacity(nodes, aabbs, o.numpy(), d.numpy(), sc["xyz"].numpy(), cinv, sc["opacity"][:, 0].numpy(),
                                        sc["normal"].numpy())[1])
    changed = int((np.abs(vis[0] - vis[1]) > 2e-5).sum())
    occluded, free = float((vis[0] == 0).mean()), float((vis[0] == 1).mean())
    print("occlusion scene: P=%d K=%d  occluded %.3f  free %.3f  partial %.3f;  rays changed by 5e-5 direction noise: %d of %d "
          "(%.3f %%)" % (P, K, occluded, free, 1 - occluded - free, changed, vis[0].size, 100.0 * changed / vis[0].size))
    assert 0.5 < occluded < 0.97 and free > 0.01 and 1 - occluded - free > 0.02, "the scene must occlude, let rays through and attenuate some"
    assert changed <= 0.01 * vis[0].size
