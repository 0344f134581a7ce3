"""Float64 restatements of the glue kernels of the two fused training iterations (csrc/stage2_glue.hip, csrc/stage1_glue.hip,
csrc/adam.hip + csrc/adam_update.hpp), one function per kernel; plain torch on the CPU, no GPU and no library.

Every function takes torch tensors of ONE dtype and works in it: called on the float32 inputs widened to float64 it is the reference
(ref64), called on the float32 inputs themselves it is the yardstick of the tolerance rule (ref32, `tolerance` below).  VALUES are
plain expressions (the generic pieces are train_step's and torch's: tv_loss, F.normalize, F.softplus; the Sobel stencil is `sobel`);
GRADIENTS come from autograd of those expressions -- the kernels' hand-written chain rules are what is under test, so no chain rule is written here.

Two rules make the comparison exact where it has to be:
  * DECISION LITERALS (what a kernel compares against) enter as their float32 value, widened: a float32 input on either side of one
    takes the same branch in the kernel, in ref32 and in ref64.  That is why rgb_to_srgb is restated here (train_step's compares with
    the double 0.0031308); tests/test_glue_reference_cpu.py pins the restatement to train_step's in float32.
  * PER-ELEMENT SCALE: every function returns {name: (value, scale)}; `scale` has the value's shape and holds the sum of the
    absolute values of the addends that form the element (what was added, not what remained), so that a cancellation
    (g_op = r - bg + op F dscale/dop, var = D2 - D D, 1 - sigmoid) is judged against what the kernel really rounded.  The scales
    are written by hand from the kernels' expressions; they only size the bound, a wrong value still fails."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from relightable3dgaussian_amd import train_step as ts

U32 = 2.0 ** -24                    # one float32 rounding, relative
TINY = 2.0 ** -126                  # smallest normal float32: a result below it may be flushed, an absolute error of the FORMAT
SUM_SLOTS = 32                      # R3DG_SUM_SLOTS (include/r3dg_hip.h)


def f32(x):
    return float(np.float32(x))


KNEE = f32(0.0031308)
OP_MIN = f32(1e-5)
VAR_MIN = f32(1e-6)
ENT_LO = f32(1e-6)
ENT_HI = float(np.float32(1.0) - np.float32(1e-6))
N_EPS = f32(1e-3)
Q_EPS = f32(1e-12)
SOFT_T = 20.0
BAD = f32(3.0e38)
LOG2E = 1.4426950408889634


def n_exp(x):
    """Roundings of __expf(x) / __logf: 4 + those of the scaled argument, ceil(|x| log2 e) -- per element (never wider than the count
    at the case's largest |x|)."""
    return 4.0 + np.ceil(np.abs(np.asarray(x, np.float64)) * LOG2E)


def n_sig(x):
    return n_exp(x) + 2.0


def widen(args, dtype):
    """Float tensors of a (nested) argument structure as `dtype`; everything else as it is."""
    if isinstance(args, torch.Tensor):
        return args.to(dtype) if args.is_floating_point() else args
    if isinstance(args, dict):
        return {k: widen(v, dtype) for k, v in args.items()}
    if isinstance(args, (list, tuple)):
        return type(args)(widen(v, dtype) for v in args)
    return args


def tolerance(ref64, ref32, scale, n):
    """The rule of section 4 for one output array -> (d, bound): d = max (|ref32 - ref64| - TINY)+ / scale, and per element
    bound = max(2 d, n 2^-24) scale + TINY.  TINY (2^-126) is the float32 format's underflow: a value below it may come out as 0."""
    r64, r32, s = (np.asarray(a, np.float64) for a in (ref64, ref32, scale))
    diff = np.maximum(np.abs(r32 - r64) - TINY, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(s > 0, diff / np.where(s > 0, s, 1.0), np.where(diff > 0, np.inf, 0.0))
    d = float(ratio.max()) if ratio.size else 0.0
    n = np.broadcast_to(np.asarray(n, np.float64), s.shape)
    bound = np.maximum(2.0 * d, n * U32) * s + np.where(s > 0, TINY, 0.0)
    return d, bound


# ---- generic pieces --------------------------------------------------------------------------------------------------------------
def rgb_to_srgb(x):
    """train_step.rgb_to_srgb (utils/graphics_utils.py:207-213, clip=True) with the knee as its float32 value."""
    curve = torch.where(x > KNEE, torch.pow(torch.clamp_min(x, KNEE), 1.0 / 2.4) * 1.055 - 0.055, 12.92 * x)
    return curve.clamp(0.0, 1.0)


def srgb_curve(x):
    """The unclipped curve (a decision quantity: against 0 and 1)."""
    return torch.where(x > KNEE, torch.pow(torch.clamp_min(x, KNEE), 1.0 / 2.4) * 1.055 - 0.055, 12.92 * x)


def _grad(out, leaves, **kw):
    gs = torch.autograd.grad(out, leaves, allow_unused=True, **kw)
    return [torch.zeros_like(l) if g is None else g for g, l in zip(gs, leaves)]


def _leaf(t):
    return t.detach().clone().requires_grad_(True)


def divided(opacity, feature, n_contrib):
    """feat = feature / max(opacity, 1e-5) * (n_contrib > 0) (neilf.py:190-200, render.py:107-112) -> (feat, mask / opc, opc)."""
    m = (n_contrib > 0).to(opacity.dtype)
    opc = opacity.clamp_min(OP_MIN)
    sc = m / opc
    return feature * sc, sc, opc


def pbr_x(opacity, feature, n_contrib, bg):
    """The linear PBR image pbr_img = feat[2:5] * op + (1 - op) * bg and the scale of its two addends."""
    feat, sc, opc = divided(opacity, feature[2:5], n_contrib)
    a, b = feat * opacity, (1.0 - opacity) * bg[:, None]
    return a + b, a.abs() + b.abs()


def _srgb_scale(x, sx):
    """Scale of srgb(x): 1.055 p + 0.055 on the curve, 12.92 (scale of x) on the line; 0 where the clip makes the value a constant."""
    with torch.no_grad():
        p = torch.pow(torch.clamp_min(x, KNEE), 1.0 / 2.4)
        s = torch.where(x > KNEE, 1.055 * p + 0.055, 12.92 * sx)
        c = srgb_curve(x)
        return torch.where((c < 0) | (c > 1), torch.zeros_like(s), s)


# ---- stage 2, per pixel -------------------------------------------------------------------------------------------------------------
def stage2_pbr_srgb(opacity, feature, n_contrib, bg):
    """s2_pbr_srgb_kernel and the sRGB half of s2_normals_srgb_kernel."""
    x, sx = pbr_x(opacity, feature, n_contrib, bg)
    return {"srgb": (rgb_to_srgb(x), _srgb_scale(x, sx))}


def stage2_loss(image, opacity, feature, pseudo, n_contrib, gt, bg, mask, w_l1, w_pbr, w_normal, extra_dimage, extra_dsrgb,
                sparse):
    """s2_loss_kernel<SPARSE>: the three sums and dL_dimage [3,HW], dL_dopacity [HW], dL_dfeature [16,HW] (maps the sparse kernel
    does not write come out as zeros here; the test expects their canary)."""
    image, opacity, feature = _leaf(image), _leaf(opacity), _leaf(feature)
    feat, sc, opc = divided(opacity, feature, n_contrib)
    x = feat[2:5] * opacity + (1.0 - opacity) * bg[:, None]
    x.retain_grad()
    srgb = rgb_to_srgb(x)
    mk = torch.ones_like(opacity) if mask is None else mask
    d0, d1 = image - gt, srgb - gt
    normal_on = (not sparse) or w_normal != 0.0
    dn = (feat[5:8] - pseudo) * mk
    sums = [d0.abs().sum(), d1.abs().sum(), dn.square().sum() if normal_on else None]
    L = w_l1 * sums[0] + w_pbr * sums[1]
    if extra_dimage is not None:
        L = L + (extra_dimage * image).sum()
    if extra_dsrgb is not None:
        L = L + (extra_dsrgb * srgb).sum()
    if normal_on:
        L = L + w_normal * sums[2]
    dsr, = _grad(srgb.sum(), [x], retain_graph=True)
    gi, go, gf = _grad(L, [image, opacity, feature])
    with torch.no_grad():
        ei = 0.0 if extra_dimage is None else extra_dimage.abs()
        es = 0.0 if extra_dsrgb is None else extra_dsrgb.abs()
        m = (n_contrib > 0)
        dsc = torch.where(m & (opacity >= OP_MIN), -1.0 / (opc * opc), torch.zeros_like(opc))
        A = (abs(w_pbr) * torch.sign(d1).abs() + es) * dsr.abs()
        s_gi = abs(w_l1) * torch.sign(d0).abs() + ei
        s_gf = torch.zeros_like(gf)
        s_gf[2:5] = A * opacity.abs() * sc
        addn = (feat[5:8].abs() + pseudo.abs()) * mk
        s_gn = 2.0 * abs(w_normal) * addn * mk if normal_on else torch.zeros_like(addn)
        s_gf[5:8] = s_gn * sc
        s_go = (A * (feat[2:5].abs() + bg[:, None].abs() + (opacity * feature[2:5] * dsc).abs())).sum(0) \
            + (s_gn * (feature[5:8] * dsc).abs()).sum(0)
        sx = (feat[2:5] * opacity).abs() + ((1.0 - opacity) * bg[:, None]).abs()
        out = {"dL_dimage": (gi, s_gi), "dL_dopacity": (go, s_go), "dL_dfeature": (gf, s_gf),
               "sum_l1": (sums[0].detach(), d0.abs().sum()),
               "sum_pbr": (sums[1].detach(), (_srgb_scale(x, sx) + torch.where(d1 != 0, gt.abs(), torch.zeros_like(gt))).sum())}
        if normal_on:
            out["sum_normal"] = (sums[2].detach(), addn.square().sum())
        return out


# ---- stage 1, per pixel -------------------------------------------------------------------------------------------------------------
def sobel(x):
    """train_step.spatial_gradient of x [C,H,W] -> [C,2,H,W] (Sobel / 8 on the replicate-padded image), written as differences of
    shifted images: over a constant neighbourhood they are exactly 0 in float32 as in float64, which sign(G) = 0 needs -- torch's
    float32 convolution returns 1e-9 there, with a sign.  tests/test_glue_reference_cpu.py pins this to train_step's."""
    c, h, w = x.shape
    p = F.pad(x[None], (1, 1, 1, 1), mode="replicate")[0]
    s = lambda dy, dx: p[:, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    gx = ((s(-1, 1) - s(-1, -1)) + 2.0 * (s(0, 1) - s(0, -1)) + (s(1, 1) - s(1, -1))) * 0.125
    gy = ((s(1, -1) - s(-1, -1)) + 2.0 * (s(1, 0) - s(-1, 0)) + (s(1, 1) - s(-1, 1))) * 0.125
    return torch.stack([gx, gy], 1)


def _sobel_abs(x):
    """|Sobel| / 8 on the replicate-padded image: the sum of the absolute addends of train_step.spatial_gradient."""
    b, c, h, w = x.shape
    kx = torch.tensor([[1.0, 0.0, 1.0], [2.0, 0.0, 2.0], [1.0, 0.0, 1.0]], dtype=x.dtype) / 8.0
    k = torch.stack([kx, kx.t()])[:, None]
    return F.conv2d(F.pad(x.reshape(b * c, 1, h, w), (1, 1, 1, 1), mode="replicate"), k).reshape(b, c, 2, h, w)


def stage1_loss(W, H, image, opacity, feature, pseudo, n_contrib, gt, mask, w_l1, w_entropy, w_normal, w_smooth, w_var,
                extra_dimage):
    """s1_edge_kernel + s1_loss_kernel: sums 0, 1, 2, 4 (w_smooth != 0 only), 5 and dL_dimage [3,HW], dL_dopacity [HW],
    dL_dfeature [5,HW]."""
    image, opacity, feature = _leaf(image), _leaf(opacity), _leaf(feature)
    feat, sc, opc = divided(opacity, feature, n_contrib)
    mk = torch.ones_like(opacity) if mask is None else mask
    d0 = image - gt
    o = opacity.clamp(ENT_LO, ENT_HI)
    ent = -(mk * torch.log(o) + (1.0 - mk) * torch.log(1.0 - o))
    dn = (feat[:3] - pseudo) * mk
    D, D2 = feat[3], feat[4]
    var = D2 - D * D
    sd = var.clamp_min(VAR_MIN).sqrt()
    sums = {"sum_l1": d0.abs().sum(), "sum_normal": dn.square().sum(), "sum_entropy": ent.sum(), "sum_var": sd.sum()}
    L = w_l1 * sums["sum_l1"] + w_entropy * sums["sum_entropy"] + w_normal * sums["sum_normal"] + w_var * sums["sum_var"]
    if w_smooth != 0.0:
        gn_ = sobel(feat[:3].reshape(3, H, W))
        e = torch.exp(-sobel(gt.reshape(3, H, W)).abs())
        sums["sum_edge"] = (gn_.abs() * e).sum()              # first_order_edge_aware_loss * 3 H W
        L = L + w_smooth * sums["sum_edge"]
    if extra_dimage is not None:
        L = L + (extra_dimage * image).sum()
    gi, go, gf = _grad(L, [image, opacity, feature])
    with torch.no_grad():
        ei = 0.0 if extra_dimage is None else extra_dimage.abs()
        m = (n_contrib > 0)
        dsc = torch.where(m & (opacity >= OP_MIN), 1.0 / (opc * opc), torch.zeros_like(opc))
        inside = (opacity >= ENT_LO) & (opacity <= ENT_HI)
        s_ent = torch.where(inside, abs(w_entropy) * (mk.abs() / o + (1.0 - mk).abs() / (1.0 - o)), torch.zeros_like(o))
        addn = (feat[:3].abs() + pseudo.abs()) * mk
        s_gn = 2.0 * abs(w_normal) * addn * mk
        s_edge = None
        if w_smooth != 0.0:
            # adjoint of the |stencil| on |sign(G n)| e: the absolute addends of the gathered adjoint (pass B of s1_loss_kernel)
            nl = _leaf(feat[:3].reshape(1, 3, H, W))
            with torch.enable_grad():
                t = (_sobel_abs(nl)[0] * (torch.sign(gn_).abs() * e)).sum()
                s_dsm, = _grad(t, [nl])
            s_gn = s_gn + abs(w_smooth) * s_dsm.reshape(3, -1)
            s_edge = (_sobel_abs(feat[:3].abs().reshape(1, 3, H, W))[0] * e).sum()
        unclamped = var >= VAR_MIN
        s_var = D2.abs() + D * D
        s_sd = torch.where(unclamped, sd + s_var / (2.0 * sd), torch.zeros_like(sd))     # clamped: the constant sqrt(1e-6)
        s_dvar = torch.where(unclamped, abs(w_var) * 0.5 / sd * (s_sd / sd), torch.zeros_like(sd))
        s_gf = torch.zeros_like(gf)
        s_gf[:3] = s_gn * sc
        s_gf[3] = 2.0 * D.abs() * s_dvar * sc
        s_gf[4] = s_dvar * sc
        s_go = s_ent + (s_gn * (feature[:3].abs() * dsc)).sum(0) \
            + (2.0 * D.abs() * s_dvar * feature[3].abs() + s_dvar * feature[4].abs()) * dsc
        # log(1 - o): the argument 1 - o is itself rounded (relative 2^-24, which the logarithm turns into an ABSOLUTE 2^-24)
        s_e = (mk.abs() * torch.log(o).abs() + (1.0 - mk).abs() * (torch.log(1.0 - o).abs() + 1.0)).sum()
        out = {"dL_dimage": (gi, abs(w_l1) * torch.sign(d0).abs() + ei), "dL_dopacity": (go, s_go), "dL_dfeature": (gf, s_gf),
               "sum_l1": (sums["sum_l1"].detach(), d0.abs().sum()), "sum_normal": (sums["sum_normal"].detach(), addn.square().sum()),
               "sum_entropy": (sums["sum_entropy"].detach(), s_e),
               "sum_var": (sums["sum_var"].detach(), (torch.where(unclamped, s_sd, sd)).sum())}
        if w_smooth != 0.0:
            out["sum_edge"] = (sums["sum_edge"].detach(), s_edge)
        return out


# ---- per Gaussian ------------------------------------------------------------------------------------------------------------------
def _depth(xyz, vm):
    """depth = xyz . viewmatrix[:, 2] + viewmatrix[3, 2] (row-vector convention) and the scale of its four addends."""
    col = vm.reshape(4, 4)[:, 2]
    return xyz @ col[:3] + col[3], xyz.abs() @ col[:3].abs() + col[3].abs()


def _activations(a):
    out = {"scales": torch.exp(a["scaling_raw"]), "rot": F.normalize(a["rotation_raw"], dim=-1, eps=Q_EPS),
           "opacity": torch.sigmoid(a["opacity_raw"]), "normal": F.normalize(a["normal_raw"], dim=-1, eps=N_EPS)}
    if a.get("base_raw") is not None:
        out["base_color"] = 0.03 + 0.77 * torch.sigmoid(a["base_raw"])
        out["roughness"] = 0.09 + 0.9 * torch.sigmoid(a["rough_raw"])
        out["viewdirs"] = F.normalize(a["campos"][None] - a["xyz"], dim=-1, eps=Q_EPS)
    return out


def stage2_activate(a, with_features=True):
    """s2_activate_kernel (GaussianModel.get_*; base_raw None = the stage-1 use): values with scale |value| (0.03 + 0.77 s and
    0.09 + 0.9 s: the two addends); the feature row's columns 0, 1 (depth, depth^2), 5..7, 8..10, 11 when `with_features`."""
    v = _activations(a)
    out = {k: (t, t.abs()) for k, t in v.items()}
    if "base_color" in v and with_features:
        d, sd = _depth(a["xyz"], a["viewmatrix"])
        feats = torch.zeros(a["xyz"].shape[0], 16, dtype=d.dtype)
        sf = torch.zeros_like(feats)
        feats[:, 0], feats[:, 1], feats[:, 5:8], feats[:, 8:11], feats[:, 11] = d, d * d, v["normal"], v["base_color"], v["roughness"]
        sf[:, 0], sf[:, 1], sf[:, 5:8], sf[:, 8:11], sf[:, 11] = sd, sd * sd, v["normal"].abs(), v["base_color"], v["roughness"]
        out["features"] = (feats, sf)
    return out


def softplus_env(env_raw):
    """The texture side job of s2_activate_kernel: F.softplus(beta 1, threshold 20)."""
    v = F.softplus(env_raw, beta=1.0, threshold=SOFT_T)
    return {"env": (v, v.abs())}


def light_l1(dl):
    """sum_p sum_c |dl_c - mean_c dl| (neilf.py:286-292) and its scale (|dl_c| + the mean's three addends / 3)."""
    m = dl.mean(-1, keepdim=True)
    return (dl - m).abs().sum(), (dl.abs() + dl.abs().sum(-1, keepdim=True) / 3.0).sum()


def stage2_pack_features(xyz, vm, normal, base_color, roughness, shade_out):
    """s2_pack_features_kernel: columns 0, 1 computed; every other column is a COPY (compared bit for bit by the test)."""
    d, sd = _depth(xyz, vm)
    v, s = light_l1(shade_out[:, 3:6])
    rows = torch.cat([d[:, None], (d * d)[:, None], shade_out[:, 0:3], normal, base_color, roughness.reshape(-1, 1), shade_out[:, 3:6],
                      shade_out[:, 18:19]], 1)
    srows = rows.abs().clone()
    srows[:, 0], srows[:, 1] = sd, sd * sd
    return {"features": (rows, srows), "light_l1_sum": (v, s)}


def stage1_pack_features(xyz, vm, normal):
    d, sd = _depth(xyz, vm)
    rows = torch.cat([normal, d[:, None], (d * d)[:, None]], 1)
    srows = rows.abs().clone()
    srows[:, 3], srows[:, 4] = sd, sd * sd
    return {"features": (rows, srows)}


def stage2_unpack_gradients(dL_dfeatures, shade_out, light_weight):
    """s2_unpack_kernel: dL_dpbr (a copy), dL_ddiffuse = feature gradient + light_weight * d(light_l1)/d dl, and the light sum."""
    dl = _leaf(shade_out[:, 3:6])
    v, s = light_l1(dl)
    g, = _grad(light_weight * v, [dl])
    with torch.no_grad():
        sg = torch.sign(dl - dl.mean(-1, keepdim=True)).abs()
        s_d = dL_dfeatures[:, 12:15].abs() + abs(light_weight) * (sg + sg.sum(-1, keepdim=True) / 3.0)
        return {"dL_dpbr": (dL_dfeatures[:, 2:5], dL_dfeatures[:, 2:5].abs()), "dL_ddiffuse": (dL_dfeatures[:, 12:15] + g, s_d),
                "light_l1_sum": (v.detach(), s.detach())}


def _normalize_backward_scale(v, g, eps):
    """Absolute addends of the backward of v / max(|v|, eps): (|g_c| + |u_c| sum_k |u_k g_k|) / |v| above eps, |g_c| / eps below."""
    n = v.norm(dim=-1, keepdim=True)
    u = v / n.clamp_min(1e-300)
    above = (g.abs() + u.abs() * (u * g).abs().sum(-1, keepdim=True)) / n.clamp_min(1e-300)
    return torch.where(n > eps, above, g.abs() / eps)


def activate_backward(a, up, stage2=True, frozen=False):
    """s2_activate_backward_kernel / s1_activate_backward_kernel: the chain rule of every activation, by autograd of
    sum(upstream * activation).  `up`: dL_dfeatures [P,16 | 5], dL_dscales, dL_drot, dL_dopacity, dL_dmeans3D and, stage 2,
    dL_dbase, dL_drough, dL_dviewdirs.  frozen: only g_base / g_rough (the others are not touched)."""
    names = ["xyz", "scaling_raw", "rotation_raw", "opacity_raw", "normal_raw"] + (["base_raw", "rough_raw"] if stage2 else [])
    a = dict(a)
    for k in names:
        a[k] = _leaf(a[k])
    if not stage2:
        a["base_raw"] = None
    v = _activations(a)
    d, sd = _depth(a["xyz"], a["viewmatrix"])
    gf = up["dL_dfeatures"]
    if stage2:
        L = (gf[:, 0] * d + gf[:, 1] * d * d).sum() + (gf[:, 5:8] * v["normal"]).sum() \
            + ((gf[:, 8:11] + up["dL_dbase"]) * v["base_color"]).sum() + ((gf[:, 11] + up["dL_drough"]) * v["roughness"]).sum() \
            + (up["dL_dviewdirs"] * v["viewdirs"]).sum()
        gdepth, gdepth2, gnormal = gf[:, 0], gf[:, 1], gf[:, 5:8]
    else:
        L = (gf[:, :3] * v["normal"]).sum() + (gf[:, 3] * d + gf[:, 4] * d * d).sum()
        gdepth, gdepth2, gnormal = gf[:, 3], gf[:, 4], gf[:, :3]
    L = L + (up["dL_dscales"] * v["scales"]).sum() + (up["dL_drot"] * v["rot"]).sum() + (up["dL_dopacity"] * v["opacity"]).sum() \
        + (up["dL_dmeans3D"] * a["xyz"]).sum()
    g = dict(zip(names, _grad(L, [a[k] for k in names])))
    with torch.no_grad():
        sig = torch.sigmoid
        out = {}
        if stage2:
            sb, sr = sig(a["base_raw"]), sig(a["rough_raw"])
            out["g_base"] = (g["base_raw"], (gf[:, 8:11].abs() + up["dL_dbase"].abs()) * 0.77 * sb * (1.0 + sb))
            out["g_rough"] = (g["rough_raw"], (gf[:, 11].abs() + up["dL_drough"].abs()) * 0.9 * sr * (1.0 + sr))
            if frozen:
                return out
        so = sig(a["opacity_raw"])
        col = a["viewmatrix"].reshape(4, 4)[:3, 2]
        s_xyz = up["dL_dmeans3D"].abs() + ((gdepth.abs() + 2.0 * sd * gdepth2.abs())[:, None] * col.abs()[None])
        if stage2:
            s_xyz = s_xyz + _normalize_backward_scale(a["campos"][None] - a["xyz"], up["dL_dviewdirs"], Q_EPS)
        out.update({"g_xyz": (g["xyz"], s_xyz), "g_scaling": (g["scaling_raw"], g["scaling_raw"].abs()),
                    "g_rotation": (g["rotation_raw"], _normalize_backward_scale(a["rotation_raw"], up["dL_drot"], Q_EPS)),
                    "g_opacity": (g["opacity_raw"], up["dL_dopacity"].abs() * so * (1.0 + so)),
                    "g_normal": (g["normal_raw"], _normalize_backward_scale(a["normal_raw"], gnormal, N_EPS))})
        return out


def env_backward(He, We, raw, env, dL_denv, w_tv):
    """env_backward_block (s2_env_backward_kernel and the texture job of s2_activate_backward_kernel): g_raw = (dL_denv + w_tv
    dTV/denv) softplus'(raw) and TV(env) = train_step.tv_loss of the [3,He,We] image.  A direction with no differences (a one-row or
    one-column texture) contributes 0, the kernel's convention -- torch's mean over nothing is NaN."""
    env, raw = _leaf(env), _leaf(raw)
    img = env.reshape(He, We, 3).permute(2, 0, 1)
    zero = env.sum() * 0.0
    if He > 1 and We > 1:
        tv = ts.tv_loss(img)
    else:
        tv = (img[:, 1:, :] - img[:, :-1, :]).square().mean() if He > 1 else zero
        tv = tv + ((img[:, :, 1:] - img[:, :, :-1]).square().mean() if We > 1 else zero)
    gtv, = _grad(tv, [env])
    dsoft, = _grad(F.softplus(raw, beta=1.0, threshold=SOFT_T).sum(), [raw])
    with torch.no_grad():
        a = img.abs()
        s_g, s_tv = torch.zeros_like(a), zero.detach().clone()
        if He > 1:
            pair = (a[:, 1:, :] + a[:, :-1, :]) / (3.0 * (He - 1) * We)
            s_g[:, 1:, :] += 2.0 * pair
            s_g[:, :-1, :] += 2.0 * pair
            s_tv = s_tv + ((a[:, 1:, :] + a[:, :-1, :]).square() / (3.0 * (He - 1) * We)).sum()
        if We > 1:
            pair = (a[:, :, 1:] + a[:, :, :-1]) / (3.0 * He * (We - 1))
            s_g[:, :, 1:] += 2.0 * pair
            s_g[:, :, :-1] += 2.0 * pair
            s_tv = s_tv + ((a[:, :, 1:] + a[:, :, :-1]).square() / (3.0 * He * (We - 1))).sum()
        s_g = s_g.permute(1, 2, 0).reshape(-1)
        return {"g_raw": ((dL_denv + w_tv * gtv) * dsoft, (dL_denv.abs() + abs(w_tv) * s_g) * dsoft),
                "tv_sum": (tv.detach(), s_tv)}


# ---- Adam --------------------------------------------------------------------------------------------------------------------------
def adam_rates(n, lr, lr_tail, period, split):
    idx = np.arange(n)
    return np.where((idx % period) >= split, lr_tail, lr) if period else np.full(n, lr)


def adam_step(p, g, m, v, lr, beta1, beta2, eps, step, grad_scale):
    """One torch.optim.Adam step (no weight decay / amsgrad) from a GIVEN state, numpy arrays of one dtype; `lr` per element.
    -> {param, exp_avg, exp_avg_sq: (value, scale)}; the scales follow adam_update (csrc/adam_update.hpp): m + (gk - m)(1 - beta1)."""
    dt = p.dtype.type
    beta1, beta2, eps, grad_scale = dt(beta1), dt(beta2), dt(eps), dt(grad_scale)
    lr = np.asarray(lr, p.dtype)
    gk = g * grad_scale
    m2 = beta1 * m + (dt(1) - beta1) * gk
    v2 = beta2 * v + (dt(1) - beta2) * gk * gk
    b1, b2 = 1.0 - float(beta1) ** step, 1.0 - float(beta2) ** step
    denom = np.sqrt(v2) / dt(math.sqrt(b2)) + eps
    upd = (lr / dt(b1)) * (m2 / denom)
    s_m = np.abs(m) * (2.0 - beta1) + (dt(1) - beta1) * np.abs(gk)
    return {"param": (p - upd, np.abs(p) + (lr / dt(b1)) * (s_m / denom)), "exp_avg": (m2, s_m), "exp_avg_sq": (v2, v2)}
