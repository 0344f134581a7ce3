"""Seeded inputs of the image-stencil tests (tests/test_stencil_kernels_gpu.py; checked on the CPU by
tests/test_stencil_reference_cpu.py): CPU float32 tensors.  The conventions are those of tests/glue_cases.py: a decision quantity is
either exact by construction or kept clear of its threshold by re-drawing (deterministically, from the case's own generator)."""
import torch

from tests import glue_cases as gc
from tests import glue_reference as gr

# ---- SSIM --------------------------------------------------------------------------------------------------------------------------
SSIM_SHAPES = [(1, 1), (7, 5), (32, 32), (33, 33), (38, 27), (65, 6), (6, 70)]      # (W, H): the tile is 32 x 32, the halo 5
SSIM_CHANNELS = [1, 3]
BLOCK = 16


def ssim_blocks(W, H):
    """Origins (x, y) of the four 16 x 16 blocks (clipped to the image): a 2 x 2 grid where it fits, a row or a column of four in
    the strips, none in the two small images."""
    if W >= 32 and H >= 27:
        return [(0, 0), (16, 0), (0, 16), (16, 16)]
    if W >= 64:
        return [(0, 0), (16, 0), (32, 0), (48, 0)]
    if H >= 64:
        return [(0, 0), (0, 16), (0, 32), (0, 48)]
    return []


def ssim_images(W, H, C, seed):
    """x0, x1 (two rendered images) and y (the target), [C,H,W]: noise ~ U(-0.1, 1.2), independent per image and channel, and in it
      block 0  x0 = x1 = y = 0.0: both agree exactly (with the zero padding, in the corner), mu = 0, D = C2 exactly;
      block 1  y = 0.0 alone, the rendered images keep their noise;
      block 2  x = 1.0 against y = 1 - 2^-7: flat in BOTH images, E[x^2] - mu^2 cancels against C2 (a white background) -- the two
               constants differ so that dS/dmu1 is not a 0 that only exact arithmetic delivers;
      block 3  y = 1.0 against x = 1 - 2^-6, with one pixel of x at 0.25 / 0.5 / 0.75 (per channel) three pixels in from the block's
               corner: the window's footprint and symmetry on a constant ground, and flat pixels beyond its reach.
    The two small images hold noise, the last pixel of y at 1.0 and (7 x 5) pixel 0 at 0.0 in all three."""
    g = torch.Generator().manual_seed(seed)
    U = lambda: torch.rand(C, H, W, generator=g) * 1.3 - 0.1
    x0, x1, y = U(), U(), U()
    blocks = ssim_blocks(W, H)
    if not blocks:
        if W * H > 1:
            for t in (x0, x1, y):
                t[:, 0, 0] = 0.0
        y[:, -1, -1] = 1.0
        return x0, x1, y
    sl = lambda o: (slice(None), slice(o[1], o[1] + BLOCK), slice(o[0], o[0] + BLOCK))
    for t in (x0, x1, y):
        t[sl(blocks[0])] = 0.0
    y[sl(blocks[1])] = 0.0
    for t in (x0, x1):
        t[sl(blocks[2])] = 1.0
        t[sl(blocks[3])] = 1.0 - 2.0 ** -6
    y[sl(blocks[2])] = 1.0 - 2.0 ** -7
    y[sl(blocks[3])] = 1.0
    ix, iy = blocks[3][0] + 3, blocks[3][1] + 3
    if ix < W and iy < H:
        for c in range(C):
            x0[c, iy, ix] = 0.25 * (1 + c % 3)
            x1[c, iy, ix] = 0.75 - 0.25 * (c % 3)
    return x0, x1, y


def ssim_scales(W, H, C):
    """The two images' backward scales: the loss term's 1 / (C H W) and a second, different value (sign and size); as float32
    values, which is what the ABI takes."""
    return gr.f32(1.0 / (C * H * W)), gr.f32(-0.2 / (C * H * W))


# ---- edge-aware smoothness ------------------------------------------------------------------------------------------------------------
# (W, H): degenerate adjoints (a side of 1 or 2); the streamed kernel's 60-column strip at exactly one strip, one strip + one column,
# two strips + one column; its 8-row strip at exactly one strip and one strip + one row
SMOOTH_SHAPES = [(1, 1), (1, 9), (9, 1), (2, 2), (2, 17), (7, 5), (60, 8), (61, 3), (121, 9)]
SIGN_CLEAR = 128.0 * gr.U32                    # >= 4 x the 21 roundings of a data map's Sobel response (the GPU module's table)


def _special_pixels():
    """(opacity, n_contrib, mask, x of the base-colour / light maps [3] or None = keep the noise): written as F = x * max(op, 1e-5)."""
    k, hi = gr.KNEE, gc.clip_hi()
    return [(gr.OP_MIN, 3, 1.0, None),                                  # exactly 1e-5f: the clamp passes the gradient (>=)
            (gc.step32(gr.OP_MIN, 1), 2, 0.625, None),                  # the next float above
            (4e-6, 4, 1.0, None),                                       # below: scale 1e5, no gradient to the opacity
            (0.5, 0, 1.0, None),                                        # n_contrib == 0 next to covered pixels, feature != 0
            (1.0, 1, 1.0, (gc.step32(k, -1), k, gc.step32(k, 1))),      # the knee's two sides
            (1.0, 5, 0.375, (-0.25, 0.0, -1e-3)),                       # maps below 0 (clipped: no gradient) and 0 itself
            (1.0, 2, 1.0, (1.0, hi, 4.0)),                              # the clip at 1
            (0.25, 6, 0.0, None),                                       # mask exactly 0 on covered content
            (0.125, 7, 1.0, None)]                                      # mask exactly 1


def smooth_maps(W, H, seed):
    """Inputs of the three smoothness entry points for a W x H image, flattened [., HW].
    Noise: opacity in {1, 1/2, 1/4, 1/8} (F / o and F * (1 / o) are the same float), n_contrib in 1..8, normal ~ N(0,1), base
    colour and diffuse light x ~ U(-0.08, 1.3) (6 % below 0, 23 % above 1 where the clip makes a constant), roughness ~ U(0.09, 0.99),
    depth ~ U(0.5, 5) (feature 0, map 3 of the stage-1 image), depth^2 beside it, mask 0 / 1 / U(0,1) on 15 / 45 / 40 %, target
    ~ U(0,1); everything covered (n_contrib > 0) and non-constant on the four borders and in the corners.
    Crafted: the pixels of _special_pixels at seeded interior positions (without an interior: anywhere but pixel 0, the first half
    of them as far as half the free pixels go); a 5 x 5 block (3 x 3 in a corner of the images with no side of 17; clipped) where every data map, the guide normal, the mask and the opacity are constant -- the
    stencil is exactly 0 in every precision and the gradient in the block's middle must be exactly 0; the target is constant over the
    same block; a 2 x 2 island of n_contrib == 0 where the image is at least 30 wide and 4 high.
    Every Sobel response of a data map, of the guide normal and of the depth is then either bit-equal in float32 and float64 or at
    least SIGN_CLEAR * (its absolute sum) from 0: offending neighbourhoods are re-drawn."""
    HW = W * H
    g = torch.Generator().manual_seed(seed)
    U = lambda *s: torch.rand(*s, generator=g)
    op = torch.tensor([1.0, 0.5, 0.25, 0.125])[torch.randint(0, 4, (HW,), generator=g)]
    nc = torch.randint(1, 9, (HW,), generator=g, dtype=torch.int32)
    r = U(HW)
    mask = torch.where(r < 0.15, torch.zeros(HW), torch.where(r < 0.6, torch.ones(HW), U(HW)))
    gt = U(3, HW)
    x = torch.zeros(16, HW)                                            # the DIVIDED maps; feature = x * max(op, 1e-5)

    def draw(idx):
        n = len(idx)
        x[5:8, idx] = torch.randn(3, n, generator=g)
        x[8:11, idx] = U(3, n) * 1.38 - 0.08
        x[11, idx] = 0.09 + 0.9 * U(n)
        x[12:15, idx] = U(3, n) * 1.38 - 0.08
        x[0, idx] = 0.5 + 4.5 * U(n)
        x[1, idx] = x[0, idx] ** 2 + 0.01
    draw(torch.arange(HW))
    x[2:5], x[15] = U(3, HW), U(HW)
    locked, special = torch.zeros(H, W, dtype=torch.bool), torch.zeros(HW, dtype=torch.bool)
    # the constant blocks
    nb = 5 if max(W, H) >= 17 else 3
    bx, by = (10 if W >= 17 else max(0, W - nb)), (10 if H >= 17 else max(0, H - nb))
    blk = torch.zeros(H, W, dtype=torch.bool)
    if HW > 4:
        blk[by:by + nb, bx:bx + nb] = True
    b = blk.reshape(-1)
    op[b], nc[b], mask[b] = 0.5, 3, 0.75
    x[:, b] = torch.tensor([1.5, 2.26, .1, .2, .3, 0.25, -0.5, 0.75, 0.3, 0.6, 0.9, 0.4, 0.2, 0.5, 0.8, 0.1])[:, None]
    locked |= blk
    # (the target is constant over the SAME block: a constant target beside changing data gives neighbouring adjoint inputs of
    # exactly equal size, w * 3, whose weighted sum is a 0 that only one order of operations delivers)
    gt[:, b] = torch.tensor([0.25, 0.5, 0.75])[:, None]
    if W >= 30 and H >= 4:
        isl = torch.zeros(H, W, dtype=torch.bool)
        isl[1:3, 28:30] = True
        nc[isl.reshape(-1)] = 0
        locked |= isl
    # the special pixels
    interior = torch.zeros(H, W, dtype=torch.bool)
    interior[1:H - 1, 1:W - 1] = True
    free = (interior & ~locked).reshape(-1).nonzero()[:, 0]
    count = 9
    if len(free) < 9:
        free = (~locked).reshape(-1).nonzero()[:, 0]
        free = free[1:] if HW > 1 else free                             # (not pixel 0: the first corner stays noise)
        count = min(9, (len(free) + 1) // 2)
    spots = free[torch.randperm(len(free), generator=g)][:count]
    for i, (o, n, m, xs) in zip(spots.tolist(), _special_pixels()):
        op[i], nc[i], mask[i] = o, n, m
        if xs is not None:
            x[8:11, i] = torch.tensor(xs)
            x[12:15, i] = torch.tensor(xs[::-1])
        locked.view(-1)[i] = True
        special[i] = True
    opc = op.clamp_min(gr.OP_MIN)
    for _ in range(100):
        feature = x * opc
        bad = smooth_offenders(W, H, op, feature, nc, mask, special)
        if not bad.any():
            break
        # re-draw the unlocked pixels of every offending 3 x 3 neighbourhood
        grow = torch.nn.functional.max_pool2d(bad.float()[None, None], 3, 1, 1)[0, 0] > 0
        idx = (grow & ~locked).reshape(-1).nonzero()[:, 0]
        assert len(idx), "smooth_maps: an offending neighbourhood is all crafted pixels"
        draw(idx)
    else:
        raise AssertionError("smooth_maps: could not clear the decisions")
    feat5 = torch.cat([feature[5:8], feature[0:1], feature[1:2]], 0).contiguous()
    g2 = torch.Generator().manual_seed(seed + 1)
    return dict(W=W, H=H, opacity=op, feature=feature.contiguous(), feat5=feat5, n_contrib=nc, gt=gt, mask=mask, block=blk, special=special,
                old_dopacity=torch.randn(HW, generator=g2), old_normal=torch.randn(3, HW, generator=g2),
                old_dfeat5=torch.randn(5, HW, generator=g2))


def smooth_decision_maps(W, H, opacity, feature, n_contrib, mask, dtype):
    """The maps whose Sobel SIGN the kernels decide on, in `dtype`: {name: [C,H,W]} -- srgb(base) m, roughness m, srgb(light) m, the
    guide normal, the stage-1 depth -- and the sRGB arguments x of the base-colour and light maps [6,HW]."""
    o, f = opacity.to(dtype), feature.to(dtype)
    feat, _, _ = gr.divided(o, f, n_contrib)
    mk = mask.to(dtype)
    img = lambda t: t.reshape(-1, H, W)
    maps = dict(base=img(gr.rgb_to_srgb(feat[8:11]) * mk), rough=img(feat[11:12] * mk), light=img(gr.rgb_to_srgb(feat[12:15]) * mk),
                normal=img(feat[5:8]), depth=img(feat[0:1]))
    return maps, torch.cat([feat[8:11], feat[12:15]], 0)


def srgb_offenders(x32, x64, skip):
    """[HW] bool: pixels with an sRGB argument (x [6,HW]) that differs between float32 and float64 within 64 * 2^-24 |x| of the knee,
    or whose curve lies within 64 * 2^-24 * (its scale) of the clip's 0 or 1 -- except at the crafted pixels `skip`, whose arguments
    are exact by construction (x = F at opacity 1: the knee's neighbours, 0, 1 and the first float at which the clip is decided)."""
    curve = gr.srgb_curve(x64)
    sc = torch.where(x64 > gr.KNEE, 1.055 * torch.pow(x64.clamp_min(gr.KNEE), 1.0 / 2.4) + 0.055, 12.92 * x64.abs())
    bad = (gc.near(x64, (gr.KNEE,), x64.abs()) & (x32.double() != x64)) | gc.near(curve, (0.0, 1.0), sc)
    return bad.any(0) & ~skip


def smooth_offenders(W, H, opacity, feature, n_contrib, mask, skip, clear=SIGN_CLEAR):
    """[H,W] bool: pixels where some decision map's Sobel response differs between float32 and float64 AND lies within
    clear * (the stencil's absolute sum) of 0 -- checked with the mask and without it (mask = 1) -- or srgb_offenders."""
    _, x32 = smooth_decision_maps(W, H, opacity, feature, n_contrib, mask, torch.float32)
    _, x64 = smooth_decision_maps(W, H, opacity, feature, n_contrib, mask, torch.float64)
    bad = srgb_offenders(x32, x64, skip).reshape(H, W)
    for mk in (mask, torch.ones_like(mask)):
        m32, _ = smooth_decision_maps(W, H, opacity, feature, n_contrib, mk, torch.float32)
        m64, _ = smooth_decision_maps(W, H, opacity, feature, n_contrib, mk, torch.float64)
        for k in m64:
            g32, g64 = gr.sobel(m32[k]).double(), gr.sobel(m64[k])
            s = gr._sobel_abs(m64[k].abs()[None])[0]
            bad |= ((g32 != g64) & (g64.abs() < clear * s)).any(0).any(0)
    return bad


def smooth_weights(W, H):
    """The three weights, carrying the 1 / (3 H W) of the reference's means (lambdas 1, 0.5, 1 of script/run_syn4.sh), as float32 values."""
    n = 3.0 * W * H
    return gr.f32(1.0 / n), gr.f32(0.5 / n), gr.f32(1.0 / n)


def depth_weight(W, H):
    return gr.f32(0.4 / (3.0 * W * H))


SUBSETS = {"base": (1, 0, 0), "rough": (0, 1, 0), "base+rough": (1, 1, 0), "light": (0, 0, 1), "base+light": (1, 0, 1),
           "rough+light": (0, 1, 1), "all": (1, 1, 1)}
THREE_PASS_SUBSETS = ("all", "base+rough", "light")
_CASES = {}


def smooth_case(W, H):
    if (W, H) not in _CASES:
        _CASES[(W, H)] = smooth_maps(W, H, seed=500 + 13 * W + H)
    return _CASES[(W, H)]


def ssim_case(W, H, C):
    if ("ssim", W, H, C) not in _CASES:
        _CASES[("ssim", W, H, C)] = ssim_images(W, H, C, seed=700 + 11 * W + 3 * H + C)
    return _CASES[("ssim", W, H, C)]
