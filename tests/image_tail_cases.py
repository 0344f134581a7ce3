"""Seeded inputs and the float64 reference of the fused stage-2 image tail (r3dg_stage2_image_tail, csrc/image_tail.hip), for
tests/test_image_tail_gpu.py; checked on the CPU by tests/test_image_tail_cases_cpu.py.  Everything is composed from what exists:

INPUTS (CPU float32, flattened [., HW] as the ABI takes them)
  opacity, feature, n_contrib, bg, mask   tests/glue_cases.s2_pixels: its crafted threshold pixels (the sRGB knee, the clip, the
                                          1e-5 opacity clamp, n_contrib == 0) and its random pixels, kept clear of every threshold.
                                          The flattened pixel order is ROTATED so that the crafted pixels are the image's LAST ones:
                                          the image's origin belongs to block 0 of the SSIM images below.
  image, gt                               tests/stencil_cases.ssim_images (x0 and y): noise and the four blocks (both exactly 0 in
                                          the zero-padded corner, target 0 alone, two flat pairs whose variance cancels against C2).
                                          At the crafted pixels image and gt take s2_pixels' crafted values (image == gt,
                                          srgb == gt == 0, srgb == gt == 1 ...), which replaces up to twelve pixels of a block in the
                                          images the blocks cover entirely.
  depth                                   a tilted plane + 5 % noise, premultiplied by the opacity (tests/test_glue_kernels_gpu.py's
                                          pseudo-normal case), with that test's view matrix and intrinsics.
  DECISIONS.  The knee, the clip and the opacity clamp are kept clear by s2_pixels.  sign(image - gt) is exact in any precision.
  sign(srgb - gt) is either exact by construction (both sides the same constant: the clip's 0 / 1 against a block's 0 / 1) or kept
  glue_cases.CLEAR * (scale of srgb + |gt|) away from 0: offending target values are re-drawn from the case's own generator.

REFERENCE (tail_reference; one dtype throughout, as tests/glue_reference.py)
  srgb          glue_reference.stage2_pbr_srgb
  SSIM          stencil_reference.ssim_forward, then stencil_reference.ssim_backward on its partials, for (image, gt) with
                scale_image and for (srgb, gt) with scale_pbr
  loss          glue_reference.stage2_loss(sparse=True) with the two SSIM gradients as extra_dimage / extra_dsrgb
  SCALES compose the same way: the SSIM gradient's scale is stencil_reference.ssim_backward_abs over the partials' SCALES (their
  first-order propagated scales, not their values), and stage2_loss's own scale expressions -- linear in |extra| -- are evaluated
  with those in place of |extra|."""
import torch

from tests import glue_cases as gc
from tests import glue_reference as gr
from tests import stencil_cases as sc
from tests import stencil_reference as sr

TILE = 32                                      # TAIL_T (csrc/image_tail.hip)
# (W, H): the SSIM kernels' shapes; then, for the tile edge T = 32, T + 11 and 2 T + 1 along each axis with the other axis small --
# the first sizes at which a recomputed partial comes from a neighbour tile's interior, and at which a tile has neighbours on both
# sides ((65, 6) and (6, 70) are SSIM shapes already)
SHAPES = sc.SSIM_SHAPES + [s for s in [(TILE + 11, 11), (11, TILE + 11), (2 * TILE + 1, 6), (6, 2 * TILE + 6)]
                           if s not in sc.SSIM_SHAPES]
TAN_FOVX, TAN_FOVY = 0.6, 0.45
_CASES = {}


def weights(W, H):
    """w_l1, w_pbr, w_normal as an iteration passes them (the 1 / (3 H W) of the reference's means inside), as float32 values."""
    n = 3.0 * W * H
    return gr.f32(0.8 / n), gr.f32(0.6 / n), gr.f32(0.3 / n)


def _pbr_sign_offenders(c):
    """[3,HW] elements of the target whose sign(srgb - gt) is neither exact by construction nor clear of 0."""
    o, f, b, t = c["opacity"].double(), c["feature"].double(), c["bg"].double(), c["gt"].double()
    r64 = gr.stage2_pbr_srgb(o, f, c["n_contrib"], b)["srgb"]
    r32 = gr.stage2_pbr_srgb(c["opacity"], c["feature"], c["n_contrib"], c["bg"])["srgb"][0]
    exact = (r64[0] == t) & (r32 == c["gt"])
    return ((r64[0] - t).abs() < gc.CLEAR * (r64[1] + t.abs())) & ~exact


def tail_case(W, H):
    """The inputs of one W x H image (module docstring); computed once, shared, never modified."""
    if (W, H) in _CASES:
        return _CASES[(W, H)]
    HW = W * H
    s2 = gc.s2_pixels(HW, seed=7000 + W * 7 + H)
    ne = s2["n_edge"]
    roll = lambda t: torch.roll(t, -ne, dims=-1)                       # pixel i of s2_pixels -> pixel (i - n_edge) mod HW
    x0, _, y = sc.ssim_images(W, H, 3, seed=7100 + W * 5 + H)
    image, gt = x0.reshape(3, HW).clone(), y.reshape(3, HW).clone()
    if ne:
        image[:, HW - ne:], gt[:, HW - ne:] = s2["image"][:, :ne], s2["gt"][:, :ne]
    c = dict(W=W, H=H, HW=HW, n_edge=ne, image=image, gt=gt, opacity=roll(s2["opacity"]), feature=roll(s2["feature"]),
             n_contrib=roll(s2["n_contrib"]), bg=s2["bg"], mask=roll(s2["mask"]))
    g = torch.Generator().manual_seed(7200 + W * 3 + H)
    for _ in range(100):
        bad = _pbr_sign_offenders(c)
        bad[:, HW - ne:] = False
        if not bad.any():
            break
        c["gt"][bad] = torch.rand(int(bad.sum()), generator=g)
    else:
        raise AssertionError("tail_case: could not clear sign(srgb - gt)")
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    noise = torch.rand(H, W, generator=g)
    c["depth"] = ((2.0 + 0.9 * xs / max(W, 2) + 0.7 * ys / max(H, 2)) * (1.0 + 0.05 * noise)).reshape(HW) * c["opacity"]
    c["viewmatrix"] = gc.gaussians(1, seed=1)["viewmatrix"]
    c["cx"], c["cy"] = 0.5 * W + 0.25, 0.5 * H - 0.5
    _CASES[(W, H)] = c
    return c


def decisions(c, dtype):
    """Every decision the tail takes per pixel, by the restatement in `dtype`."""
    cast = lambda t: t.to(dtype)
    o, f, b, t, im = cast(c["opacity"]), cast(c["feature"]), cast(c["bg"]), cast(c["gt"]), cast(c["image"])
    x, _ = gr.pbr_x(o, f, c["n_contrib"], b)
    curve = gr.srgb_curve(x)
    return {"knee": x > gr.KNEE, "clip_low": curve < 0.0, "clip_high": curve > 1.0, "opacity_clamp": o >= gr.OP_MIN,
            "covered": c["n_contrib"] > 0, "sign_image": torch.sign(im - t), "sign_pbr": torch.sign(gr.rgb_to_srgb(x) - t)}


def tail_reference(W, H, image, opacity, feature, pseudo, n_contrib, gt, bg, mask, w_l1, w_pbr, w_normal, scale_image, scale_pbr):
    """{name: (value, scale)} of everything r3dg_stage2_image_tail writes from these inputs: dL_dimage [3,HW], dL_dopacity [HW],
    dL_dfeature [16,HW] (maps the kernel does not write are zeros here), sum_l1, sum_pbr, sum_normal (w_normal != 0 only),
    ssim_image, ssim_pbr.  `pseudo` [3,HW] are the pseudo normals (the kernel forms them itself; the test takes them from
    r3dg_stage2_normals_srgb, which it also holds the kernel's equal to)."""
    HW = W * H
    srgb = gr.stage2_pbr_srgb(opacity, feature, n_contrib, bg)["srgb"][0]
    maps = lambda t: t.reshape(3, H, W)
    out, grads, grad_scales = {}, [], []
    for name, x, scale in (("image", image, scale_image), ("pbr", srgb, scale_pbr)):
        fwd = sr.ssim_forward(maps(x), maps(gt))
        grads.append(sr.ssim_backward(maps(x), maps(gt), fwd["partials"][0], scale)["grad_x"][0].reshape(3, HW))
        grad_scales.append(sr.ssim_backward_abs(maps(x), maps(gt), fwd["partials"][1], scale).reshape(3, HW))
        out["ssim_" + name] = fwd["sum"]
    args = (image, opacity, feature, pseudo, n_contrib, gt, bg, mask, w_l1, w_pbr, w_normal)
    value = gr.stage2_loss(*args, grads[0], grads[1], sparse=True)
    scale = gr.stage2_loss(*args, grad_scales[0], grad_scales[1], sparse=True)
    for k in value:
        out[k] = (value[k][0], scale[k][1])
    return out
