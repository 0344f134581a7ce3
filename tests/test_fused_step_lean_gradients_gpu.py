"""Whole single-GPU iterations of FusedStage2Step with the two [P,48] gradients kept on chip (the geometry backward applies the
SH colour group's Adam, the incident-light chain does not write the rotated-back gradient) against the schedule with the
separate SH Adam launch and the gradient write (R3DG_SH_ADAM_IN_BACKWARD=0, R3DG_CHAIN_WRITES_GRADIENT=1)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
P, K, RES = 3000, 16, 96


def _scene():
    from relightable3dgaussian_amd import synthetic as syn
    from relightable3dgaussian_amd.bench_core import GaussianParams, render_stage1
    scene = syn.make_scene(P=P, seed=1, stage2=True, scale_log_mean=-3.0)
    cam = syn.orbit_cameras(4, width=RES, height=RES)[0].to(DEV)
    bg = torch.ones(3, device=DEV)
    params = GaussianParams(scene, DEV, True)
    with torch.no_grad():
        gt = render_stage1(params, cam, bg)[2].clone() * 0.9
    return params, cam, bg, gt


def _iterations(monkeypatch, lean, scene, samples=None, lrs=None):
    """Three iterations that train and, between the second and the third, one whose view is dropped on the device (a capacity
    far below the view's instance count).  -> (the step, {name: tensor} of every parameter group and both its moments, the Adam
    launches' group indices, was grads["shs"] left untouched by the iterations)."""
    from relightable3dgaussian_amd.fused_step import FusedStage2Step
    monkeypatch.setenv("R3DG_SH_ADAM_IN_BACKWARD", "1" if lean else "0")
    monkeypatch.setenv("R3DG_CHAIN_WRITES_GRADIENT", "0" if lean else "1")
    params, cam, bg, gt = scene
    step = FusedStage2Step(params, K, lr=1e-3, lrs=lrs)
    if samples is not None:             # (every run shades with the same traced visibility)
        step.visibility, step.incident_dirs, step.incident_areas = samples
    launches = []
    step_groups = step.opt.step_groups
    step.opt.step_groups = lambda idx, *a, **k: (launches.append(tuple(idx)), step_groups(idx, *a, **k))[1]
    sentinel = torch.full_like(step.grads["shs"], 777.0)
    step.grads["shs"].copy_(sentinel)
    step(cam, bg, gt)                   # two-phase forward: learns the instance count
    step(cam, bg, gt)                   # bounded forward, three streams, the chain kernel
    n_before = step.opt.step_count
    step._capacity = 1000               # this view will not fit
    step(cam, bg, gt)
    assert step.poll_overflow() == 1 and step.opt.step_count == n_before
    step(cam, bg, gt)
    step.flush()
    torch.cuda.synchronize()
    assert step.opt.step_count == 3 and step.poll_overflow() == 0
    state = {}
    for i, k in enumerate(step._opt_order):
        state[k] = (step.incidents if k == "incidents" else getattr(step, k)).clone()
        state[k + ".exp_avg"], state[k + ".exp_avg_sq"] = step.opt.groups[i]["exp_avg"].clone(), step.opt.groups[i]["exp_avg_sq"].clone()
    return step, state, launches, torch.equal(step.grads["shs"], sentinel)


def test_lean_iterations_train_like_the_separate_launches(monkeypatch):
    """Every parameter group and both its moments after 3 + 1 (dropped) iterations agree with the parent schedule within 4x the
    difference two runs of the PARENT schedule show against each other on the same inputs (the tile backward's float atomics
    make that non-zero).  The schedule itself: with the switch on no Adam launch carries the SH group and grads["shs"] is never
    written; with it off the group has its own early launch every iteration.
    Measured on MI355X (P 3000, 96x96, K 16; per tensor the largest |difference| relative to the tensor's largest entry, the
    worst tensor): two parent runs 1.04e-5 (scaling.exp_avg; the parameters themselves 2e-9 .. 9e-7), lean against parent
    1.04e-5 -- in that run most tensors of the lean run were bit-identical to one of the two parent runs."""
    scene = _scene()
    step_a, a, launches_a, untouched_a = _iterations(monkeypatch, False, scene)
    samples = (step_a.visibility, step_a.incident_dirs, step_a.incident_areas)
    assert step_a._frs is not None, "the scenario has to run the fixed-ray-set path (the chain kernel)"
    step_b, b, _launches_b, _ = _iterations(monkeypatch, False, scene, samples)
    step_c, c, launches_c, untouched_c = _iterations(monkeypatch, True, scene, samples)
    assert step_c._frs is not None
    sh = step_c._opt_order.index("shs")
    assert any(l == (sh,) for l in launches_a) and not untouched_a
    assert all(sh not in l for l in launches_c) and untouched_c
    # ONE number for "the difference two parent runs show": per tensor the largest |difference| relative to the tensor's largest
    # entry, the worst of them over all tensors.  (Tensor by tensor the statistic is one draw of a heavy-tailed quantity -- a
    # handful of Gaussians whose atomics landed in another order: two pairs of parent runs gave 6.8e-9 and 1.3e-9 for the same
    # tensor -- so a per-tensor 4x would fail on the parent against itself.)
    rel = lambda x, y: float((x - y).abs().max()) / max(float(x.abs().max()), 1e-30)
    noise = max(rel(a[k], b[k]) for k in a)
    assert noise > 0.0, "two parent runs are bit-identical here: the scene does not exercise the atomics"
    worst = 0.0
    for k in a:
        diff = rel(a[k], c[k])
        print("%-24s parent vs parent %.3e  lean vs parent %.3e  (relative to the largest entry)" % (k, rel(a[k], b[k]), diff))
        worst = max(worst, diff)
        assert diff <= 4.0 * noise, "%s: lean vs parent %.3e, parent vs parent (worst tensor) %.3e" % (k, diff, noise)
    print("worst tensor: parent vs parent %.3e, lean vs parent %.3e" % (noise, worst))
    for k in ("shs", "incidents", "xyz", "env"):        # (the two groups in question and their neighbours did train)
        assert float(c[k + ".exp_avg_sq"].abs().max()) > 0.0


def test_frozen_geometry_keeps_the_separate_schedule(monkeypatch):
    """run_syn4.sh's schedule (every geometry rate and the SH colour rates 0): there is no geometry backward to apply an Adam
    step in, the step says so, and the iterations run as before -- one Adam launch of the four groups that train."""
    frozen = dict(xyz=0.0, normal=0.0, scaling=0.0, rotation=0.0, opacity=0.0, shs=0.0, shs_rest=0.0, base_color=0.01,
                  roughness=0.01, incidents=0.001, incidents_rest=0.0001, env=0.1)
    step, state, launches, _ = _iterations(monkeypatch, True, _scene(), lrs=frozen)
    assert step.frozen_geometry and not step._fuses_sh_adam()
    assert launches and all(len(l) <= 4 and step._opt_order.index("shs") not in l for l in launches)
    assert float(state["shs.exp_avg_sq"].abs().max()) == 0.0 and float(state["base_color.exp_avg_sq"].abs().max()) > 0.0
