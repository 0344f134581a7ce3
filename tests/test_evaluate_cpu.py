"""relightable3dgaussian_amd/evaluate.py without a GPU: its PyTorch restatement (reference_metrics, reference_albedo_scale)
against the reference's own psnr / ssim / mask composites / albedo-scale median (tests/golden/eval_reference.npz, written by
make_eval_golden.py), and the argument checks of the three C entry points (no launch happens)."""
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_reference.npz")


def fixture():
    z = np.load(GOLD)
    return {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}


def cases_of(z, tag):
    """(case name, mask, fill) of make_eval_golden.py"""
    return (("plain", None, None), ("bg", z[tag + "_mask"], z[tag + "_bg"]), ("env", z[tag + "_mask"], z[tag + "_env"]))


@pytest.mark.parametrize("tag", ["a", "b"])
def test_reference_metrics_reproduce_the_reference_python(tag):
    """PSNR within 1e-4 dB of the reference's float32 AND float64 results, SSIM within 2e-6, the median exact."""
    from relightable3dgaussian_amd import evaluate as E
    z = fixture()
    pred, gt = z[tag + "_pred"], z[tag + "_gt"]
    for case, mask, fill in cases_of(z, tag):
        m = E.reference_metrics(pred, gt, mask, fill)
        for ref in ("psnr32", "psnr64"):
            want = float(z["%s_%s_%s" % (tag, case, ref)])
            print(tag, case, ref, float(m["psnr"]), want)
            assert abs(float(m["psnr"]) - want) <= 1e-4, (case, ref)
        want = float(z["%s_%s_ssim" % (tag, case)])
        print(tag, case, "ssim", float(m["ssim"]), want)
        assert abs(float(m["ssim"]) - want) <= 2e-6, case
    mask, bg = z[tag + "_mask"], z[tag + "_bg"]
    # the script takes the median of the images it has already masked onto the background (:165,177,201)
    base_color, gt_albedo = E.composite(pred, mask, bg), E.composite(gt, mask, bg)
    assert torch.equal(E.reference_albedo_scale(base_color, gt_albedo, mask), z[tag + "_albedo_scale32"])
    assert torch.equal(E.reference_albedo_scale(base_color.double(), gt_albedo.double(), mask), z[tag + "_albedo_scale64"])
    assert float(z[tag + "_albedo_scale32"].min()) > 1.02            # (the fixture's albedo is darker than its ground truth)


def test_capture_reference_is_the_map_derivation_of_the_relight_fixture():
    """evaluate.capture_reference on the reference's own raw feature image gives the reference's own maps."""
    from relightable3dgaussian_amd import evaluate as E
    z = np.load(os.path.join(os.path.dirname(GOLD), "pipeline_reference_relight.npz"))
    t = lambda k: torch.from_numpy(z[k])
    maps = E.capture_reference(t("a_feature_image"), t("a_map_opacity"), t("a_num_contrib"), t("a_bg"))
    for k in ("roughness", "visibility", "normal"):
        torch.testing.assert_close(maps[k], t("a_map_" + k), rtol=1e-6, atol=1e-7)
    for k in ("pbr", "base_color", "diffuse", "specular", "lights", "local_lights", "global_lights"):
        torch.testing.assert_close(maps[k], t("a_map_" + k), rtol=0, atol=1e-6)


def test_entry_points_reject_bad_arguments():
    from relightable3dgaussian_amd import _abi, _lib
    L = _lib.lib()
    EINVAL = -1
    assert _abi.constants["R3DG_EVAL_ROW"] == 8 and _abi.constants["R3DG_EVAL_MEDIAN_STATE_WORDS"] >= 3 * 256 + 7
    maps = [1] * 11
    assert L.r3dg_relight_capture(None, 8, 8, None, 1, 1, 1, None, *maps) == EINVAL                   # no feature image
    assert b"null" in L.r3dg_last_error()
    assert L.r3dg_relight_capture(None, 8, 8, 1, 1, None, 1, None, *maps) == EINVAL                   # no num_contrib
    assert L.r3dg_relight_capture(None, 8, 8, 1, 1, 1, None, None, *maps) == EINVAL                   # pbr without a background
    assert b"background" in L.r3dg_last_error()
    assert L.r3dg_relight_capture(None, 8, 8, 1, 1, 1, None, 1, None, *maps[1:]) == EINVAL            # mask without a background
    assert L.r3dg_relight_capture(None, -1, 8, 1, 1, 1, 1, None, *maps) == EINVAL
    assert L.r3dg_relight_capture(None, 1 << 16, 1 << 15, 1, 1, 1, 1, None, *maps) == EINVAL          # 2^31 pixels
    assert b"too large" in L.r3dg_last_error()
    assert L.r3dg_relight_capture(None, 0, 8, None, None, None, None, None, *([None] * 11)) == 0      # empty image
    assert L.r3dg_eval_image_metrics(None, 8, 8, 3, None, 1, None, None, 0, 1, 1) == EINVAL           # no prediction
    assert L.r3dg_eval_image_metrics(None, 8, 8, 3, 1, 1, None, None, 0, None, 1) == EINVAL           # no scratch
    assert L.r3dg_eval_image_metrics(None, 8, 8, 3, 1, 1, None, None, 0, 1, None) == EINVAL           # no table row
    assert L.r3dg_eval_image_metrics(None, 8, 8, 4, 1, 1, None, None, 0, 1, 1) == EINVAL              # a row holds three channels
    assert L.r3dg_eval_image_metrics(None, 8, 0, 3, 1, 1, None, None, 0, 1, 1) == EINVAL
    assert L.r3dg_eval_image_metrics(None, 8, 8, 3, 1, 1, None, 1, 0, 1, 1) == EINVAL                 # fill without a mask
    assert b"mask" in L.r3dg_last_error()
    assert L.r3dg_eval_image_metrics(None, 1 << 16, 1 << 15, 3, 1, 1, None, None, 0, 1, 1) == EINVAL
    assert L.r3dg_eval_median_ratio(None, 8, 8, None, 1, None, 1, 1) == EINVAL
    assert L.r3dg_eval_median_ratio(None, 8, 8, 1, 1, None, None, 1) == EINVAL                        # no scratch
    assert L.r3dg_eval_median_ratio(None, 8, 8, 1, 1, None, 1, None) == EINVAL                        # no table row
    assert L.r3dg_eval_median_ratio(None, 8, -8, 1, 1, None, 1, 1) == EINVAL
    assert L.r3dg_eval_median_ratio(None, 1 << 16, 1 << 15, 1, 1, None, 1, 1) == EINVAL
    assert b"too large" in L.r3dg_last_error()


def test_evaluator_has_no_cpu_path():
    from relightable3dgaussian_amd import evaluate as E
    with pytest.raises(RuntimeError):
        E.Evaluator(4, "cpu")
