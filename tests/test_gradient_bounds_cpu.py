"""The element-wise gradient bounds of the rasterizer backward, on the CPU: sound (another correct fp32 implementation stays
inside) and with teeth (defects confined to light rows, which `report`'s array-maximum tolerance accepts, are rejected).

Two bounds, one per stage:

  tile pass        |err| <= TILE_BOUND_C * 2^-24 * E          E = the oracle's weighted absolute sum of the element's terms
                                                              (oracle/rasterizer_oracle.c r3dgo_render_backward_bounds)
  per-Gaussian     |err| <= STAGE_BOUND_C * sigma             sigma = the stage's input conditioning (8 seeded float64
                                                              evaluations, inputs perturbed by <= 1 fp32 ulp)

MEASURED here, over the 21 cases (tests/helpers.py BWD_CASES, NO_GEOMETRY_CASE, ELEMENTWISE_CASES):
  tile pass: largest err / (2^-24 E) over the stand-ins (a) fp32 sums in pixel order, (b) reverse order, (c) per 8x8 block then
  across blocks, (d) perturbed exp / T / accum_rec steps:  %(tile_max)s  (stand-in (d), case `bg_geom_off`; (a)-(c) stay below 0.1)
      ->  TILE_BOUND_C = 4.0   (4 x the maximum, rounded up)
  per-Gaussian stage: largest |oracle_fp32 - float64| / sigma, oracle_fp32 the fp32 C restatement in the reference's operation
  order:  %(stage_max)s  (dL_dscales of `aniso_fov_ragged`; per array: scales 2064, cov3D 571, means3D 236, rotations 109, sh 8;
  the 99.9th percentile is below 260 everywhere -- the tail is the reference formulation's own cancellation, e.g.
  denom - a c in backward.cu:209, which no perturbation of the inputs shows)
      ->  STAGE_BOUND_C = 8300   (4 x the maximum, rounded up)
"""
import re
import os

import numpy as np
import pytest
import torch

from tests.helpers import (BWD_CASES, ELEMENTWISE_CASES, NO_GEOMETRY_CASE, STAGE_ARRAYS, STAGE_BOUND_C, TILE_ARRAYS,
                           TILE_BOUND_C, U32, fwd_args, make_case, oracle_backward, report, report_elementwise, stage_args,
                           upstream)

__doc__ = __doc__ % dict(tile_max="0.96", stage_max="2064")

ALL_CASES = dict(BWD_CASES, bg_geom_off=NO_GEOMETRY_CASE, **ELEMENTWISE_CASES)
TILE_INDEX = dict(mean2D=0, colors=1, opacity=2, feature=4, conic=9)          # position in the oracle's result tuple
STAGE_INDEX = dict(means3D=3, cov3D=5, sh=6, scales=7, rot=8)
OLD_RTOL, OLD_ATOL = 2e-3, 1e-6                                              # test_backward_parity's `report` tolerance

_cache = {}


def _case(name):
    """Oracle forward + backward with bounds of a case, computed once and shared (never modified)."""
    if name not in _cache:
        from oracle import rasterizer as orc
        case = make_case(**ALL_CASES[name])
        fwd = orc.rasterize_gaussians(*fwd_args(case)[:-3], want_margin=True)
        ups = upstream(case)
        geom = name != "bg_geom_off"
        ref = oracle_backward(case, fwd, ups, geom, want_bounds=True)
        _cache[name] = dict(case=case, fwd=fwd, ups=ups, geom=geom, ref=ref, bounds=ref[-1])
    return _cache[name]


def _tile_bound(bounds, key, frac=1.0):
    return frac * TILE_BOUND_C * U32 * bounds["E"][key]


@pytest.mark.parametrize("name", list(ALL_CASES))
def test_tile_pass_bound_is_sound(name):
    """Stand-ins (a)-(d) for another correct fp32 implementation stay within ONE QUARTER of the tile-pass bound on every
    element (and are exact where the bound is zero)."""
    d = _case(name)
    worst = 0.0
    for tag, kw in (("a: fp32, pixel order", dict(sum_mode=1)), ("b: fp32, reverse order", dict(sum_mode=2)),
                    ("c: fp32, 8x8 blocks", dict(sum_mode=3)), ("d: perturbed steps", dict(perturb=1.0, seed=11)),
                    ("d: perturbed steps, other seed", dict(perturb=1.0, seed=12))):
        alt = oracle_backward(d["case"], d["fwd"], d["ups"], d["geom"], **kw)
        for key in TILE_ARRAYS:
            ok, msg = report_elementwise("%s %s" % (key, tag), alt[TILE_INDEX[key]], d["ref"][TILE_INDEX[key]],
                                         _tile_bound(d["bounds"], key, 0.25))
            E = d["bounds"]["E"][key]
            err = np.abs(alt[TILE_INDEX[key]] - d["ref"][TILE_INDEX[key]])
            if (E > 0).any():
                worst = max(worst, float((err[E > 0] / (U32 * E[E > 0])).max()))
            assert ok, "[%s] %s" % (name, msg)
    e, ep = d["bounds"]["E"]["mean2D"][:, :2], d["bounds"]["E_pixel_form"]
    print("[%s] largest err / (2^-24 E) over (a)-(d): %.3f   (TILE_BOUND_C / 4 = %.2f);  moment form / pixel form of "
          "dL_dmean2D's absolute sum: max %.1f" % (name, worst, TILE_BOUND_C / 4, float((e[ep > 0] / ep[ep > 0]).max())))
    assert (e >= ep * (1 - 1e-12)).all()                                      # the moment form is never the smaller one
    assert worst <= TILE_BOUND_C / 4


@pytest.mark.parametrize("name", list(ALL_CASES))
def test_per_gaussian_bound_is_calibrated_on_the_reference_formulation(name):
    """|oracle_fp32 - float64| / sigma of the per-Gaussian stage, both evaluated on the same fp32 sums: within a quarter of
    STAGE_BOUND_C on every element of every case (the kernel gets the factor 4: other product order, FMA contraction)."""
    from oracle import rasterizer as orc
    d = _case(name)
    ref = d["ref"]
    base, sigma = orc.per_gaussian_sigma(*stage_args(d["case"], d["fwd"], ref[0], ref[9], ref[1]))
    d["stage"] = (base, sigma)
    worst = {}
    for key in STAGE_ARRAYS:
        got = np.asarray(ref[STAGE_INDEX[key]], np.float64).reshape(base[key].shape)
        if got.size == 0:
            continue
        ok, msg = report_elementwise(key, got, base[key], 0.25 * STAGE_BOUND_C * sigma[key])
        nz = sigma[key] > 0
        worst[key] = float((np.abs(got - base[key])[nz] / sigma[key][nz]).max()) if nz.any() else 0.0
        assert ok, "[%s] %s" % (name, msg)
    print("[%s] largest |oracle_fp32 - float64| / sigma: %s   (STAGE_BOUND_C / 4 = %.0f)" % (
        name, "  ".join("%s %.1f" % kv for kv in worst.items()), STAGE_BOUND_C / 4))


def _light_rows(ref):
    """Rows (Gaussians) of an array that lie wholly below `report`'s old tolerance."""
    a = np.abs(np.asarray(ref, np.float64)).reshape(ref.shape[0], -1)
    return (a <= OLD_ATOL + OLD_RTOL * a.max()).all(1) & (a > 0).any(1)


@pytest.mark.parametrize("name", ["S5", "big_splats"])
def test_zeros_in_light_rows_pass_the_old_check_and_fail_the_new(name):
    d = _case(name)
    for key in TILE_ARRAYS:
        ref = d["ref"][TILE_INDEX[key]]
        rows = _light_rows(ref)
        assert rows.sum() >= 0.2 * (np.abs(ref).reshape(len(ref), -1).max(1) > 0).sum(), (key, rows.sum())
        bad = ref.copy()
        bad[rows] = 0.0
        ok_old, m_old = report(key, bad, ref, OLD_RTOL, OLD_ATOL)
        ok_new, m_new = report_elementwise(key, bad, ref, _tile_bound(d["bounds"], key))
        print("[%s] zeros in %d light rows: old %s | new %s" % (name, rows.sum(), m_old, m_new))
        assert ok_old, "the gap this test documents has closed?  " + m_old
        assert not ok_new, m_new


@pytest.mark.parametrize("name", ["S5", "big_splats"])
def test_one_tile_of_a_light_gaussian_removed_passes_the_old_check_and_fails_the_new(name):
    """One Gaussian's contribution from ONE tile (what a dropped staging round or a lost wave leaves out), for a Gaussian below the old
    tolerance: the oracle on upstream gradients restricted to that tile gives the contribution."""
    d = _case(name)
    case, st = d["case"], d["fwd"][-1]
    ref_c = d["ref"][TILE_INDEX["colors"]]
    light = _light_rows(ref_c) & _light_rows(d["ref"][TILE_INDEX["conic"]]) & _light_rows(d["ref"][TILE_INDEX["mean2D"]])
    tiles_x = (case["W"] + 15) // 16
    # a light Gaussian that touches at least two tiles, and the tile of its list entries where it contributes
    g_pick, t_pick, part = None, None, None
    for t in range(st["ranges"].shape[0]):
        r0, r1 = st["ranges"][t]
        cand = [g for g in st["point_list"][r0:r1] if light[g] and st["tiles_touched"][g] >= 2]
        if not cand:
            continue
        ty, tx = divmod(t, tiles_x)
        mask = torch.zeros(1, case["H"], case["W"])
        mask[:, 16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16] = 1.0
        part = oracle_backward(case, d["fwd"], [u * mask for u in d["ups"]], d["geom"])
        hit = [g for g in cand if np.abs(part[TILE_INDEX["colors"]][g]).max() > 0
               and np.abs(part[TILE_INDEX["colors"]][g] - ref_c[g]).max() > 0]
        if hit:
            g_pick, t_pick = int(hit[0]), t
            break
    assert g_pick is not None, "no light Gaussian spans two tiles"
    rejected = []
    for key in TILE_ARRAYS:
        ref = d["ref"][TILE_INDEX[key]]
        if ref.shape[1] == 0:
            continue
        bad = ref.copy()
        bad[g_pick] -= part[TILE_INDEX[key]][g_pick]
        ok_old, m_old = report(key, bad, ref, OLD_RTOL, OLD_ATOL)
        ok_new, m_new = report_elementwise(key, bad, ref, _tile_bound(d["bounds"], key))
        print("[%s] Gaussian %d without tile %d: old %s | new %s" % (name, g_pick, t_pick, m_old, m_new))
        assert ok_old, m_old
        if not ok_new:
            rejected.append(key)
    # (one defect, five arrays: an array whose terms cancel heavily in that row may stay inside its bound -- dL_dopacity of
    # `big_splats` does, at 0.96 of it -- the colour, feature and depth-channel sums, which do not cancel, never do)
    assert {"colors", "feature"} <= set(rejected) and len(rejected) >= 3, rejected


def test_shifted_feature_column_and_negated_conic_b_are_rejected():
    d = _case("S5")
    case, st = d["case"], d["fwd"][-1]
    ref = d["ref"][TILE_INDEX["feature"]]
    bad = ref.copy()
    bad[:, 2] = ref[:, 3]                                                      # one column reads its neighbour's channel
    ok, msg = report_elementwise("feature", bad, ref, _tile_bound(d["bounds"], "feature"))
    print(msg)
    assert not ok
    # dL_dmean2D = -(W/2) (A S_x + B S_y), -(H/2) (C S_y + B S_x): recover the moments, form it again with -B
    m2 = d["ref"][TILE_INDEX["mean2D"]]
    A, B, Cc = (st["conic_opacity"][:, i].astype(np.float64) for i in range(3))
    gx, gy = m2[:, 0] / (-0.5 * case["W"]), m2[:, 1] / (-0.5 * case["H"])
    det = A * Cc - B * B
    vis = (st["radii"] > 0) & (det != 0)
    sx = np.where(vis, (Cc * gx - B * gy) / np.where(vis, det, 1), 0)
    sy = np.where(vis, (A * gy - B * gx) / np.where(vis, det, 1), 0)
    bad = m2.copy()
    bad[:, 0] = -0.5 * case["W"] * (A * sx - B * sy)
    bad[:, 1] = -0.5 * case["H"] * (Cc * sy - B * sx)
    ok, msg = report_elementwise("mean2D", bad, m2, _tile_bound(d["bounds"], "mean2D"))
    print(msg)
    assert not ok


def test_sh_gradients_of_degree_3_under_degree_2_are_rejected():
    from oracle import rasterizer as orc
    d = _case("sh_degree_2")
    ref = d["ref"]
    base, sigma = d.get("stage") or orc.per_gaussian_sigma(*stage_args(d["case"], d["fwd"], ref[0], ref[9], ref[1]))
    assert np.abs(base["sh"][:, 9:]).max() == 0 and sigma["sh"][:, 9:].max() == 0
    wrong = oracle_backward(dict(d["case"], degree=3), d["fwd"], d["ups"], True)[STAGE_INDEX["sh"]]
    ok, msg = report_elementwise("sh", wrong, base["sh"], STAGE_BOUND_C * sigma["sh"])
    print(msg)
    assert not ok
    ok, msg = report_elementwise("sh", ref[STAGE_INDEX["sh"]], base["sh"], STAGE_BOUND_C * sigma["sh"])
    assert ok, msg


def test_cases_contain_what_they_are_for():
    """Coverage: the projection clamp with x/y_grad_mul = 0, clamped colour channels, and back-to-front walks shorter than, exactly
    and eight times one staging round of render_backward_wave_kernel."""
    here = os.path.dirname(os.path.abspath(__file__))
    src = open(os.path.join(here, "..", "relightable3dgaussian_amd", "csrc", "rasterizer_render_bwd.hip")).read()
    body = src[src.index("render_backward_wave_kernel(const uint2*"):]
    m = re.search(r"for \(int base = 0; base < n; base \+= (\d+)\)", body)
    assert m, "the staging loop of render_backward_wave_kernel has changed shape"
    ROUND = int(m.group(1))
    assert ROUND == 64            # `for (int base = 0; base < n; base += 64)`: one lane per entry, 64 entries per round
    # x_grad_mul / y_grad_mul = 0 (backward.cu:176-177)
    d = _case("camera_inside")
    case, st = d["case"], d["fwd"][-1]
    cam = case["cam"]
    hom = np.concatenate([case["means3D"].numpy(), np.ones((case["P"], 1), np.float32)], 1) @ cam.world_view_transform.numpy()
    vis = st["radii"] > 0
    off = (np.abs(hom[:, 0] / hom[:, 2]) > np.float32(1.3 * cam.tanfovx)) | (np.abs(hom[:, 1] / hom[:, 2]) > np.float32(1.3 * cam.tanfovy))
    print("camera_inside: %d visible Gaussians, %d with x_grad_mul = 0 or y_grad_mul = 0" % (vis.sum(), (vis & off).sum()))
    assert (vis & off).sum() >= 50
    d = _case("sh_negative")
    st = d["fwd"][-1]
    n_clamped = int(st["clamped"][st["radii"] > 0].sum())
    print("sh_negative: %d clamped colour channels" % n_clamped)
    assert n_clamped >= 100
    # The wave of an 8x8 pixel block walks the first n entries of its tile's list, n = the block's deepest last contributor,
    # in rounds of 64: fewer than one round, exactly one round, at least eight rounds.
    walks = []
    for name in ALL_CASES:
        d = _case(name)
        nc, H, W = d["fwd"][1], d["case"]["H"], d["case"]["W"]
        pad = np.zeros(((H + 7) // 8 * 8, (W + 7) // 8 * 8), np.int64)
        pad[:H, :W] = nc
        walks.append(pad.reshape(pad.shape[0] // 8, 8, pad.shape[1] // 8, 8).max((1, 3)).ravel())
    walks = np.concatenate(walks)
    print("walk lengths: %d below one round, %d of exactly one round, %d of at least eight" % (
        ((walks > 0) & (walks < ROUND)).sum(), (walks == ROUND).sum(), (walks >= 8 * ROUND).sum()))
    assert ((walks > 0) & (walks < ROUND)).sum() >= 10 and (walks == ROUND).sum() >= 1 and (walks >= 8 * ROUND).sum() >= 10
    lens = np.concatenate([(_case(n)["fwd"][-1]["ranges"][:, 1].astype(np.int64) - _case(n)["fwd"][-1]["ranges"][:, 0])
                           for n in ALL_CASES])
    assert (lens < ROUND).any() and (lens >= 8 * ROUND).any()
