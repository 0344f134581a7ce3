"""Golden fixture of the evaluation metrics from the REFERENCE'S OWN, UNMODIFIED Python (this container only).

    python tests/golden/make_eval_golden.py     # needs /root/reference; writes tests/golden/eval_reference.npz (CPU, no GPU)

What runs, unmodified, from /root/reference:
    utils/image_utils.py   psnr (:24-29)
    utils/loss_utils.py    ssim (:39-63)
and, written out here because the script has no function around them, the expressions of eval_relighting_syn4.py: the mask
composites of :161-186 (`x * mask + (1 - mask) * bg`, `gt * mask + bg * (1 - mask)`, the env_only fill of :169,186) and the
albedo scale of :201 (`(gt_albedo / base_color.clamp(1e-6, 1))[:, mask[0] > 0].median(dim=1).values`).
Two seeded image pairs (37x50 and 64x64, 8-bit values like the PNGs the script loads), a soft mask with exact 0 and 1 regions,
a fill colour and a fill image.  Per pair and per case ("plain", "bg": masked onto the colour, "env": masked onto the image):
psnr in float32 (the reference's own result) and in float64 (the same function on the float32 composites cast to double), ssim
(float32); the albedo scale in float32 and float64.  Nothing of the reference is copied: inputs and outputs only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

REF = "/root/reference"


def main():
    sys.meta_path.append(mg._Finder())
    sys.path.insert(0, REF)
    from utils.image_utils import psnr
    from utils.loss_utils import ssim

    out = {}
    g = torch.Generator().manual_seed(20240611)
    q = lambda t: (t.clamp(0, 1) * 255).round() / 255           # 8-bit images
    for tag, (H, W) in (("a", (37, 50)), ("b", (64, 64))):
        gt = q(torch.rand(3, H, W, generator=g))
        # (darker per channel, as a trained albedo is up to its scale, + noise)
        pred = q(gt * torch.tensor([0.8, 0.6, 0.9])[:, None, None] + 0.05 * torch.randn(3, H, W, generator=g))
        pred[:, : H // 4, : W // 4] = 0.0                       # a region below the clamp of the albedo ratio
        env = q(torch.rand(3, H, W, generator=g) ** 2)
        yy, xx = torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing="ij")
        mask = q((1.6 - 2.2 * (xx.square() + yy.square()).sqrt()))[None]          # 1 inside, soft rim, 0 in the corners
        assert float(mask.min()) == 0.0 and float(mask.max()) == 1.0 and 0 < float((mask > 0).float().mean()) < 1
        bg = torch.tensor([1.0, 0.5, 0.25])
        cases = {
            "plain": (pred, gt),
            "bg": (pred * mask + (1 - mask) * bg[:, None, None], gt * mask + bg[:, None, None] * (1 - mask)),
            "env": (pred * mask + (1 - mask) * env, gt * mask + env * (1 - mask)),
        }
        for k, v in (("pred", pred), ("gt", gt), ("env", env), ("mask", mask), ("bg", bg)):
            out["%s_%s" % (tag, k)] = v.numpy()
        for case, (x, y) in cases.items():
            out["%s_%s_psnr32" % (tag, case)] = psnr(x, y).mean().numpy()
            out["%s_%s_psnr64" % (tag, case)] = psnr(x.double(), y.double()).mean().numpy()
            out["%s_%s_ssim" % (tag, case)] = ssim(x, y).mean().numpy()
        base_color, gt_albedo = cases["bg"]
        out[tag + "_albedo_scale32"] = (gt_albedo / base_color.clamp(1e-6, 1))[:, mask[0] > 0].median(dim=1).values.numpy()
        out[tag + "_albedo_scale64"] = (gt_albedo.double() / base_color.double().clamp(1e-6, 1))[:, mask[0] > 0] \
            .median(dim=1).values.numpy()
    path = os.path.join(HERE, "eval_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    for k in sorted(out):
        if out[k].size <= 3:
            print(k, out[k])


if __name__ == "__main__":
    main()
