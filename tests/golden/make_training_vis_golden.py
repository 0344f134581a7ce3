"""Golden fixture of the training contact sheet from the REFERENCE'S OWN Python (this container only).

    python tests/golden/make_training_vis_golden.py   # needs /root/reference and matplotlib; writes training_vis_reference.npz

What runs, unmodified, from /root/reference:
    utils/image_utils.py      visualize_depth (:6-21; its `.cuda()` lands on the CPU through make_golden._cpu_factories)
    utils/graphics_utils.py   rgb_to_srgb (:198-213)
and torch's own torch.nn.functional.interpolate on the CPU for the two nearest-neighbour resamples (the environment panels of
train.py:296 and the grid of :316).  Written out here because the reference has no function around them: the normalisation of the
feature image (render.py:107-113, neilf.py:146-182) and the panel list of train.py:283-311, line for line in float32.
RESTATED here because torchvision is not installed: make_grid(nrow=4) (padding 2, pad_value 0: every panel at
(k // 4) * (H + 2) + 2, (k % 4) * (W + 2) + 2 of a zero image) and save_image's quantisation
(grid.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(uint8)).

The inputs are tests/training_vis_reference.synthetic_maps at 30 x 40 (one stage-1 frame over a black background, one stage-2
frame with an 8 x 16 environment texture over a white one).  Stored: the inputs, the reference's float32 sheet bytes, matplotlib's
256 x 3 `turbo` table (matplotlib's data) and the two float32 constants of visualize_depth's defaults as NumPy computes them.
Nothing of the reference is copied: inputs and outputs only."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as mg  # noqa: E402
from tests import training_vis_reference as R  # noqa: E402

REF = "/root/reference"


def make_grid(panels):
    """torchvision.utils.make_grid(tensor [N,3,H,W], nrow=4) restated (padding=2, pad_value=0)."""
    n, _, H, W = panels.shape
    rows = -(-n // 4)
    grid = panels.new_zeros(3, rows * (H + 2) + 2, 4 * (W + 2) + 2)
    for k in range(n):
        y, x = (k // 4) * (H + 2) + 2, (k % 4) * (W + 2) + 2
        grid[:, y:y + H, x:x + W] = panels[k]
    return grid


def save_image_bytes(grid):
    """torchvision.utils.save_image's quantisation restated: the uint8 [H,W,3] array it hands to PIL."""
    return grid.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8).numpy()


def reference_sheet(layout, m, visualize_depth, rgb_to_srgb):
    t = lambda k: torch.from_numpy(np.ascontiguousarray(m[k]))
    opacity, n_contrib, bg = t("opacity"), t("n_contrib"), t("background")
    feature = t("feature") / opacity.clamp_min(1e-5) * (n_contrib > 0)                    # render.py:107-108, neilf.py:146-147
    if layout == 0:
        normal, depth, depth2 = torch.split(feature, [3, 1, 1], dim=0)                   # render.py:111
    else:
        depth, depth2, pbr, normal, base_color, roughness, diffuse, specular, _light, _local, global_light, visibility = \
            feature.split([1, 1, 3, 3, 3, 1, 3, 3, 3, 3, 3, 1], dim=0)                  # neilf.py:159-161
    depth_var = depth2 - depth.square()                                                   # render.py:113, neilf.py:172
    panels = [t("render"), t("gt"), visualize_depth(depth), (depth_var / 0.001).clamp_max(1).repeat(3, 1, 1),
              opacity.repeat(3, 1, 1), normal * 0.5 + 0.5, t("pseudo_normal") * 0.5 + 0.5]     # train.py:283-291
    if layout == 1:
        H, W = opacity.shape[1:]
        env = F.interpolate(t("env")[None].permute(0, 3, 1, 2), (H, 2 * W))                # train.py:296
        panels += [rgb_to_srgb(base_color), roughness.repeat(3, 1, 1), visibility.repeat(3, 1, 1), rgb_to_srgb(diffuse),
                   rgb_to_srgb(specular), rgb_to_srgb(global_light),
                   rgb_to_srgb(pbr * opacity + (1 - opacity) * bg[:, None, None]),       # neilf.py:175,182
                   rgb_to_srgb(env[0, :, :, :W]), rgb_to_srgb(env[0, :, :, W:])]         # train.py:297-311
    grid = make_grid(torch.stack(panels, dim=0))                                          # train.py:313-314
    scale = grid.shape[-2] / 800
    grid = F.interpolate(grid[None], (int(grid.shape[-2] / scale), int(grid.shape[-1] / scale)))[0]      # train.py:315-316
    return save_image_bytes(grid)


def main():
    import matplotlib
    sys.meta_path.append(mg._Finder())
    sys.path.insert(0, REF)
    for p in mg._cpu_factories():
        p.start()
    from utils.graphics_utils import rgb_to_srgb
    from utils.image_utils import visualize_depth

    out = {"turbo": np.asarray(matplotlib.colormaps["turbo"].colors, np.float64).astype(np.float32)}
    # visualize_depth's constants as ITS lines compute them (image_utils.py:9-17 with near = 0.2, far = 13)
    eps = np.finfo(np.float32).eps
    near, far = 0.2, 13
    near -= eps
    far += eps
    curve_fn = lambda x: -np.log(x + np.finfo(np.float32).eps)
    near, far = curve_fn(near), curve_fn(far)
    out["c_far"], out["span"] = np.asarray(np.minimum(near, far)), np.asarray(np.abs(far - near))
    assert out["c_far"].dtype == np.float32 and out["span"].dtype == np.float32, "NumPy 2 keeps these float32"
    for layout, bg in ((0, 0.0), (1, 1.0)):
        m = R.synthetic_maps(layout, 30, 40, R=8, seed=5, background=bg)
        for k, v in m.items():
            out["l%d_%s" % (layout, k)] = v
        out["l%d_sheet" % layout] = reference_sheet(layout, m, visualize_depth, rgb_to_srgb)
        print("layout", layout, "sheet", out["l%d_sheet" % layout].shape)
    path = os.path.join(HERE, "training_vis_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
