"""On-device evaluation (relightable3dgaussian_amd/evaluate.py; r3dg_relight_capture, r3dg_eval_image_metrics,
r3dg_eval_median_ratio) against its PyTorch restatement (evaluate.reference_metrics / reference_albedo_scale /
capture_reference), against the reference's own Python (tests/golden/eval_reference.npz, pipeline_reference_relight.npz) and
against the training path's SSIM kernel."""
import functools
import os

import numpy as np
import pytest
import torch

from tests.helpers import report

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LINEAR = ("roughness", "visibility", "normal", "depth_var")            # rtol 1e-6 + atol 1e-7: one division and one product
SRGB = ("pbr", "base_color", "diffuse", "specular", "lights", "local_lights", "global_lights")   # 4e-4 behind the sRGB curve
ORDER = ("pbr", "base_color", "roughness", "normal", "visibility", "diffuse", "specular", "lights", "local_lights",
         "global_lights", "depth_var")                                 # argument order of r3dg_relight_capture


def _capture(feature, opacity, n_contrib, bg, mask=None, names=ORDER):
    from relightable3dgaussian_amd import _lib
    from relightable3dgaussian_amd.relight import CAPTURE_MAPS
    _, H, W = feature.shape
    out = {k: torch.full((CAPTURE_MAPS[k], H, W), float("nan"), device=DEV) for k in names}
    _lib.check(_lib.lib().r3dg_relight_capture(
        _lib.current_stream(), W, H, feature.data_ptr(), opacity.data_ptr(), n_contrib.data_ptr(), bg.data_ptr(),
        _lib.ptr(mask), *[out[k].data_ptr() if k in out else None for k in ORDER]), "relight_capture")
    return out


def _relight_fixture():
    z = np.load(os.path.join(GOLD, "pipeline_reference_relight.npz"))
    t = lambda k: torch.from_numpy(z[k]).to(DEV).contiguous()
    return z, t("a_feature_image"), t("a_map_opacity"), t("a_num_contrib"), t("a_bg")


def _check_maps(got, want, names):
    msgs, ok_all = [], True
    for k in names:
        rtol, atol = (1e-6, 1e-7) if k in LINEAR else (0.0, 4e-4)
        g, w = got[k].double(), want[k].reshape(got[k].shape).to(got[k].device).double()
        err = (g - w).abs()
        bad = int((~(err <= atol + rtol * w.abs())).sum())                      # elementwise; a NaN counts as bad
        msgs.append("%-14s max|err| %.3e  bad %d/%d (rtol %g, atol %g)" % (k, float(err.max()), bad, err.numel(), rtol, atol))
        ok_all &= bad == 0
    print("\n".join(msgs))
    assert ok_all, "\n".join(msgs)


def test_capture_maps_reproduce_the_reference_frame():
    """Every a_map_* the reference's render_view wrote for the fixture's frame, from the fixture's raw feature image."""
    from relightable3dgaussian_amd import evaluate as E
    z, feature, opacity, n_contrib, bg = _relight_fixture()
    got = _capture(feature, opacity, n_contrib, bg)
    want = {k: torch.from_numpy(z["a_map_" + k]).to(DEV) for k in ORDER if k != "depth_var"}
    # (the fixture holds no depth_var: the reference's float32 expression, evaluated where the fixture was -- on the host,
    # whose division is correctly rounded; the difference of two nearly equal terms shows a last-place difference of either)
    want["depth_var"] = E.capture_reference(feature.cpu(), opacity.cpu(), n_contrib.cpu(), bg.cpu())["depth_var"]
    _check_maps(got, want, ORDER)
    # a subset: the maps not asked for are not touched, the others keep their bits
    some = _capture(feature, opacity, n_contrib, bg, names=("normal", "lights"))
    assert torch.equal(some["normal"], got["normal"]) and torch.equal(some["lights"], got["lights"])


def test_capture_maps_with_mask_and_background():
    from relightable3dgaussian_amd import evaluate as E
    _, feature, opacity, n_contrib, _ = _relight_fixture()
    H, W = feature.shape[1:]
    g = torch.Generator().manual_seed(3)
    mask = (torch.rand(H, W, generator=g) * 1.5 - 0.25).clamp(0, 1).to(DEV)         # exact zeros and ones and values between
    bg = torch.tensor([0.9, 0.4, 0.1], device=DEV)
    got = _capture(feature, opacity, n_contrib, bg, mask)
    _check_maps(got, E.capture_reference(feature.cpu(), opacity.cpu(), n_contrib.cpu(), bg.cpu(), mask.cpu()), ORDER)
    assert float(mask.min()) == 0.0 and float(mask.max()) == 1.0
    for k in ("pbr", "normal"):
        assert torch.equal(got[k][:, mask == 0], bg[:, None].expand(3, int((mask == 0).sum())))


# ---- image metrics -----------------------------------------------------------------------------------------------------------
def _images(H, W, seed):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(3, H, W, generator=g)
    pred = (gt + 0.1 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    mask = (torch.rand(H, W, generator=g) * 1.5 - 0.25).clamp(0, 1)
    return pred.to(DEV), gt.to(DEV), mask.to(DEV), torch.rand(3, generator=g).to(DEV), torch.rand(3, H, W, generator=g).to(DEV)


def _rows(ev):
    torch.cuda.synchronize()
    return ev.table[:len(ev._rows)].clone()


@pytest.mark.parametrize("shape", [(5, 7), (37, 50), (16, 200), (64, 64)])
def test_image_metrics_match_the_pytorch_restatement(shape):
    """A tile smaller than the window, ragged tiles in both directions, several tiles -- without a mask, with a mask alone,
    with a fill colour and with a fill image.  PSNR within 1e-4 dB of the float64 value (fp32 squares summed in double: ~1e-6 dB),
    SSIM within 2e-6 (the tolerance of the training path's SSIM test), two runs bit-identical, and the value-only SSIM sum
    equal to the one r3dg_ssim_forward writes."""
    from relightable3dgaussian_amd import _abi, _lib, evaluate as E
    H, W = shape
    pred, gt, mask, colour, image = _images(H, W, 100 + H)
    cases = (("plain", None, None), ("mask", mask, None), ("colour", mask, colour), ("image", mask, image))
    runs = []
    for _ in range(2):
        ev = E.Evaluator(len(cases), DEV)
        for name, m, f in cases:
            ev.add(name, pred, gt, m, f)
        runs.append(_rows(ev))
    assert torch.equal(runs[0], runs[1])
    res = ev.result()
    for i, (name, m, f) in enumerate(cases):
        want = E.reference_metrics(pred, gt, m, f)
        print(shape, name, "psnr %.9f vs %.9f  ssim %.9f vs %.9f" % (res[name]["psnr"], float(want["psnr"]), res[name]["ssim"],
                                                                   float(want["ssim"])))
        assert abs(res[name]["psnr"] - float(want["psnr"])) <= 1e-4, name
        assert abs(res[name]["ssim"] - float(want["ssim"])) <= 2e-6, name
        torch.testing.assert_close(runs[0][i, :3], want["mse"], rtol=1e-6, atol=0)
        assert float(runs[0][i, 6]) == 3.0
    # the training path's kernel on the same unmasked images
    slots = _abi.constants["R3DG_SUM_SLOTS"]
    part, total = torch.empty(3, 3, H, W, device=DEV), torch.zeros(slots, device=DEV)
    _lib.check(_lib.lib().r3dg_ssim_forward(_lib.current_stream(), W, H, 3, pred.data_ptr(), gt.data_ptr(), part.data_ptr(),
                                            total.data_ptr()), "ssim_forward")
    assert abs(float(runs[0][0, 3]) - float(total.double().sum())) / (3 * H * W) <= 2e-6


def test_single_channel_image_metrics():
    from relightable3dgaussian_amd import evaluate as E
    pred, gt, mask, colour, _ = _images(37, 50, 9)
    ev = E.Evaluator(1, DEV)
    ev.add("rough", pred[:1], gt[:1], mask, colour[:1])
    with pytest.raises(RuntimeError):
        ev.add("one too many", pred, gt)
    got, want = ev.result()["rough"], E.reference_metrics(pred[:1], gt[:1], mask, colour[:1])
    assert abs(got["psnr"] - float(want["psnr"])) <= 1e-4 and abs(got["ssim"] - float(want["ssim"])) <= 2e-6


@functools.lru_cache(None)
def _eval_fixture():
    z = np.load(os.path.join(GOLD, "eval_reference.npz"))
    return {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}


@pytest.mark.parametrize("tag", ["a", "b"])
def test_metrics_against_the_reference_python(tag):
    """tests/golden/eval_reference.npz: the device PSNR is no further from the reference's float64 value than the reference's
    own float32 result is, plus 1e-4 dB; SSIM within 2e-6; the albedo scale within rtol 1e-6 (a CPU division may differ in the
    last place)."""
    from relightable3dgaussian_amd import evaluate as E
    z = _eval_fixture()
    d = lambda k: z[tag + "_" + k].to(DEV)
    pred, gt, mask, bg, env = d("pred"), d("gt"), d("mask"), d("bg"), d("env")
    ev = E.Evaluator(4, DEV)
    ev.add("plain", pred, gt)
    ev.add("bg", pred, gt, mask, bg)
    ev.add("env", pred, gt, mask, env)
    # (the script takes the median of the images it has already masked onto the background, :165,177,201)
    ev.add_albedo_scale(E.composite(pred, mask, bg), E.composite(gt, mask, bg), mask)
    res = ev.result()
    for case in ("plain", "bg", "env"):
        p32, p64, s = (float(z["%s_%s_%s" % (tag, case, k)]) for k in ("psnr32", "psnr64", "ssim"))
        print(tag, case, "psnr %.9f (reference: float32 %.9f, float64 %.9f)  ssim %.9f (%.9f)" % (
            res[case]["psnr"], p32, p64, res[case]["ssim"], s))
        assert abs(res[case]["psnr"] - p64) <= abs(p32 - p64) + 1e-4, case
        assert abs(res[case]["ssim"] - s) <= 2e-6, case
    print(tag, "albedo scale", res["albedo_scale"][0].tolist(), z[tag + "_albedo_scale32"].tolist())
    torch.testing.assert_close(res["albedo_scale"][0], z[tag + "_albedo_scale32"], rtol=1e-6, atol=0)


# ---- albedo scale ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4096, 100003])
def test_median_ratio_is_torch_median(n):
    """Bit-equal to torch.median of the ratio array PyTorch computes on the device: random 8-bit images (runs of equal values,
    predictions below the clamp), an all-equal array, a random mask, and a mask that leaves exactly two elements (the LOWER
    median)."""
    from relightable3dgaussian_amd import evaluate as E
    g = torch.Generator().manual_seed(n)
    q = lambda t: ((t * 255).round() / 255).to(DEV)
    gt, pred = q(torch.rand(3, 1, n, generator=g)), q(torch.rand(3, 1, n, generator=g) ** 2)
    smooth_gt, smooth_pred = torch.rand(3, 1, n, generator=g).to(DEV), (0.05 + torch.rand(3, 1, n, generator=g)).to(DEV)
    some = (torch.rand(1, n, generator=g) > 0.4).float().to(DEV) * 0.5
    some[0, n // 2] = 1.0
    cases = [(pred, gt, None), (smooth_pred, smooth_gt, None), (torch.full_like(pred, 0.25), torch.full_like(gt, 0.5), None),
             (pred, gt, some), (smooth_pred, smooth_gt, some)]
    if n >= 2:
        two = torch.zeros(1, n, device=DEV)
        two[0, 0] = two[0, n - 1] = 1.0
        cases += [(smooth_pred, smooth_gt, two), (pred, gt, two)]
    ev = E.Evaluator(len(cases), DEV)
    for p, t, m in cases:
        ev.add_albedo_scale(p, t, m)
    counts = _rows(ev)[:, 3]
    got = ev.result()["albedo_scale"]
    for i, (p, t, m) in enumerate(cases):
        want = E.reference_albedo_scale(p, t, m)
        assert torch.equal(got[i], want.cpu()), (n, i, got[i].tolist(), want.tolist())
        assert int(counts[i]) == (n if m is None else int((m > 0).sum()))


def test_an_empty_mask_gives_nan_and_result_raises():
    from relightable3dgaussian_amd import evaluate as E
    pred, gt, _, _, _ = _images(16, 20, 1)
    ev = E.Evaluator(2, DEV)
    ev.add_albedo_scale(pred, gt, torch.ones(16, 20, device=DEV))
    ev.add_albedo_scale(pred, gt, torch.zeros(16, 20, device=DEV))
    rows = _rows(ev)
    assert bool(torch.isnan(rows[1, :3]).all()) and float(rows[1, 3]) == 0.0 and float(rows[0, 3]) == 320.0
    with pytest.raises(RuntimeError, match="empty mask"):
        ev.result()


# ---- end to end --------------------------------------------------------------------------------------------------------------
def _scene(base_color_scale="absent", cache="radiance"):
    from relightable3dgaussian_amd import relight, synthetic as syn
    from relightable3dgaussian_amd.bench_core import GaussianParams
    scene = syn.make_scene(P=2000, seed=5, stage2=True, scale_log_mean=-3.0)
    envmap = (3.0 * torch.rand(32, 64, 3, generator=torch.Generator().manual_seed(11)) ** 2).to(DEV)
    kw = {} if isinstance(base_color_scale, str) else {"base_color_scale": base_color_scale}
    r = relight.RelightRenderer(GaussianParams(scene, DEV, True), envmap, 16, cache=cache, **kw)
    cams = [c.to(DEV) for c in syn.orbit_cameras(8, width=64, height=64)[1:7:2]]
    return r, cams


def test_evaluate_relighting_end_to_end():
    """Three views of the 2 000-Gaussian, 64x64 scene: evaluate_relighting's results equal reference_metrics /
    reference_albedo_scale applied to relight.frame_reference's maps (capture_reference on its raw images) -- PSNR within
    1e-4 dB, SSIM within 2e-6, the albedo scale within rtol 1e-6 (the median tolerance for inputs that are not the same bits:
    the two frames' maps differ by an ulp of the sRGB curve).  On the way: the maps the frame serves equal those maps within
    the map tolerances, and the albedo scale is bit-equal to torch.median on the frame's own base_color."""
    from relightable3dgaussian_amd import evaluate as E, relight
    r, cams = _scene()
    g = torch.Generator().manual_seed(8)
    bg = torch.tensor([1.0, 1.0, 1.0], device=DEV)
    gts = [torch.rand(3, 64, 64, generator=g).to(DEV) for _ in cams]
    albedos = [(0.1 + 0.9 * torch.rand(3, 64, 64, generator=g)).to(DEV) for _ in cams]
    masks = [(torch.rand(64, 64, generator=g) * 1.5 - 0.25).clamp(0, 1).to(DEV) for _ in cams]
    res = E.evaluate_relighting(r, cams, gts, albedos, masks, bg)
    assert set(res) == {"pbr", "base_color", "pbr_env", "albedo_scale"} and res["albedo_scale"].shape == (3, 3)
    ref = {k: [] for k in ("pbr", "base_color", "pbr_env")}
    scales = []
    for i, cam in enumerate(cams):
        f = r.frame(cam, bg, outputs=("pbr", "base_color", "env_only"))
        w = relight.frame_reference(r, cam, bg, exact_activations=True)
        maps = E.capture_reference(w["feature"], w["opacity"], w["num_contrib"], bg)
        _check_maps(f, maps, ("pbr", "base_color"))
        ok, msg = report("env_only", f["env_only"], w["env_only"], 0.0, 4e-4)
        assert ok, msg
        ref["pbr"].append(E.reference_metrics(maps["pbr"], gts[i], masks[i], bg))
        ref["base_color"].append(E.reference_metrics(maps["base_color"], albedos[i], masks[i], bg))
        ref["pbr_env"].append(E.reference_metrics(maps["pbr"], gts[i], masks[i], w["env_only"]))
        scales.append(E.reference_albedo_scale(maps["base_color"], albedos[i], masks[i]).cpu())
        assert torch.equal(res["albedo_scale"][i], E.reference_albedo_scale(f["base_color"], albedos[i], masks[i]).cpu())
    for k in ref:
        psnr, ssim = (float(torch.stack([m[q] for m in ref[k]]).mean()) for q in ("psnr", "ssim"))
        print(k, "psnr %.9f vs %.9f  ssim %.9f vs %.9f  (frame_reference's maps)" % (res[k]["psnr"], psnr, res[k]["ssim"], ssim))
    print("albedo scale", res["albedo_scale"].tolist(), "vs", torch.stack(scales).tolist())
    for k in ref:
        psnr, ssim = (float(torch.stack([m[q] for m in ref[k]]).mean()) for q in ("psnr", "ssim"))
        assert abs(res[k]["psnr"] - psnr) <= 1e-4, k
        assert abs(res[k]["ssim"] - ssim) <= 2e-6, k
    torch.testing.assert_close(res["albedo_scale"], torch.stack(scales), rtol=1e-6, atol=0)
    nvs = E.evaluate_nvs(r, cams, gts, bg)
    want = [E.reference_metrics(relight.frame_reference(r, cam, bg, exact_activations=True)["render"], gt)
            for cam, gt in zip(cams, gts)]
    assert abs(nvs["psnr"] - float(torch.stack([m["psnr"] for m in want]).mean())) <= 1e-4
    assert abs(nvs["ssim"] - float(torch.stack([m["ssim"] for m in want]).mean())) <= 2e-6


def test_capture_maps_leave_the_composites_alone():
    r, cams = _scene()
    cam, bg = cams[0], torch.zeros(3, device=DEV)
    alone = r.frame(cam, bg, outputs=("pbr_env",))
    both = r.frame(cam, bg, outputs=("base_color", "pbr_env", "pbr"))
    assert torch.equal(alone["pbr_env"], both["pbr_env"]) and both["base_color"].shape == (3, 64, 64)
    with pytest.raises(RuntimeError, match="unknown relight output"):
        r.frame(cam, bg, outputs=("base_color", "nonsense"))
    # a background and a mask given as plain lists / host tensors
    listed = r.frame(cam, bg, outputs=("pbr",), capture_background=[0.0, 0.0, 0.0], mask=torch.ones(64, 64))
    assert torch.equal(listed["pbr"], both["pbr"])


@pytest.mark.parametrize("cache", ["radiance", "transport"])
def test_base_color_scale(cache):
    """None: every output has the bits of a renderer built without the argument.  A scale: the base_color map is
    srgb(scale x the unscaled linear albedo) and the shaded colour follows -- with the radiance cache and with the default one,
    whose per-frame kernel reads the scaled base colour too."""
    from relightable3dgaussian_amd import relight
    r, cams = _scene(cache=cache)
    cam, bg = cams[0], torch.zeros(3, device=DEV)
    outs = ("pbr_env", "render_env", "env_only", "pbr", "base_color", "roughness", "diffuse")
    plain = r.frame(cam, bg, outputs=outs)
    none = _scene(None, cache)[0].frame(cam, bg, outputs=outs)
    for k in outs + ("render", "opacity", "feature"):
        assert torch.equal(plain[k], none[k]), k
    scale = torch.tensor([1.3, 0.7, 0.9], device=DEV)
    rs = _scene([1.3, 0.7, 0.9], cache)[0]
    scaled = rs.frame(cam, bg, outputs=outs)
    lin = plain["feature"][8:11] / plain["opacity"].clamp_min(1e-5) * (plain["num_contrib"] > 0)
    ok, msg = report("base_color", scaled["base_color"], relight.rgb_to_srgb(scale[:, None, None] * lin), 0.0, 4e-4)
    assert ok, msg
    assert float((scaled["pbr"] - plain["pbr"]).abs().max()) > 1e-2
    assert torch.equal(scaled["roughness"], plain["roughness"]) and torch.equal(scaled["render"], plain["render"])
    # the scaled frame against the PyTorch-glue frame of the same renderer (tolerances of tests/test_relight_gpu.py)
    w = relight.frame_reference(rs, cam, bg, exact_activations=True)
    for k, rtol, atol in (("feature", 2e-4 if cache == "transport" else 2e-5, 1e-6), ("pbr_env", 0.0, 4e-4)):
        ok, msg = report(k, scaled[k], w[k], rtol, atol)
        assert ok, msg
