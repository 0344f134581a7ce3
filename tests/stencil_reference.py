"""Float64 restatements of the image-stencil kernels of the training loss (csrc/ssim.hip, csrc/smooth.hip and the depth-smoothness
pair of csrc/supervision.hip), one function per kernel; plain torch on the CPU, in the conventions of tests/glue_reference.py, whose
generic pieces (divided, rgb_to_srgb, sobel, widen, tolerance) are used as they are.

Every function takes torch tensors of ONE dtype and works in it (ref64 on the widened float32 inputs, ref32 on the inputs
themselves).  VALUES are plain expressions; GRADIENTS come from autograd of those expressions -- the kernels' hand-written adjoints
(the gathered adjoint of the replicate-padded stencil, the quotient rule of the division, the symmetric-window SSIM backward) are
what is under test.  Decision literals (1e-5, the sRGB knee, the clip's 0 and 1) enter as their float32 values, through
glue_reference.  Every function returns {name: (value, scale)}; `scale` holds, per element, the sum of the absolute addends.

SSIM scales.  A window average's scale is sum w |.|.  The per-pixel function S(mu1, mu2, E[x^2], E[y^2], E[xy]) cancels -- in a
flat region E[x^2] - mu1^2 is a difference of two numbers near 1 that is then added to C2 = 9e-4 -- so the scale of S and of each
partial derivative is the FIRST-ORDER PROPAGATION of the five averages' scales, sum_i |d out / d t_i| scale(t_i) + |out|, taken
from autograd of the per-pixel function: a flat region is judged against what float32 can deliver there, not against |out|."""
import torch
import torch.nn.functional as F

from tests.glue_reference import OP_MIN, _grad, _leaf, _sobel_abs, divided, f32, rgb_to_srgb, sobel

# kSsimWin (csrc/ssim.hip): the eleven float32 taps, widened -- not a recomputed Gaussian
SSIM_WIN = [f32(v) for v in (1.028380124e-03, 7.598758209e-03, 3.600077331e-02, 1.093606874e-01, 2.130055279e-01, 2.660117149e-01,
                             2.130055279e-01, 1.093606874e-01, 3.600077331e-02, 7.598758209e-03, 1.028380124e-03)]
SSIM_C1, SSIM_C2 = 0.01 ** 2, 0.03 ** 2


# ---- SSIM --------------------------------------------------------------------------------------------------------------------------
def _win1(t, axis):
    """The eleven taps along `axis` (-1 or -2) of t [..., H, W], zero padding: a sum of shifted slices (exactly 0 over zeros)."""
    n = t.shape[axis]
    p = F.pad(t, (5, 5, 0, 0) if axis == -1 else (0, 0, 5, 5))
    return sum(SSIM_WIN[k] * p.narrow(axis, k, n) for k in range(11))


def window(t):
    return _win1(_win1(t, -1), -2)


def _ssim_pixel(mu1, mu2, e11, e22, e12):
    A = 2.0 * mu1 * mu2 + SSIM_C1
    B = 2.0 * (e12 - mu1 * mu2) + SSIM_C2
    C = mu1 * mu1 + mu2 * mu2 + SSIM_C1
    D = (e11 - mu1 * mu1) + (e22 - mu2 * mu2) + SSIM_C2
    return A * B / (C * D)


def ssim_forward(x, y):
    """ssim_forward_kernel on x, y [C,H,W]: the SSIM map, the three partial derivatives dS/dmu1, dS/dE[x^2], dS/dE[xy] [C,3,H,W]
    (the five window averages treated as independent: autograd of the per-pixel function at them) and the map's sum."""
    with torch.no_grad():
        t = [window(x), window(y), window(x * x), window(y * y), window(x * y)]
        st = [window(x.abs()), window(y.abs()), window(x * x), window(y * y), window((x * y).abs())]
    t = [_leaf(v) for v in t]
    S = _ssim_pixel(*t)
    p = torch.autograd.grad(S.sum(), [t[0], t[2], t[4]], create_graph=True)
    outs = [S, p[0], p[1], p[2]]
    scales = []
    for o in outs:
        gs = _grad(o.sum(), t, retain_graph=True)
        scales.append((sum(g.abs() * s for g, s in zip(gs, st)) + o.abs()).detach())
    outs = [o.detach() for o in outs]
    return {"map": (outs[0], scales[0]), "partials": (torch.stack(outs[1:], 1), torch.stack(scales[1:], 1)),
            "sum": (outs[0].sum(), scales[0].sum())}


def ssim_backward(x, y, partials, scale):
    """ssim_backward_kernel: the linear map scale * (W*p0 + 2 x W*p1 + y W*p2) of GIVEN partials [C,3,H,W] (the window is symmetric)."""
    p0, p1, p2 = partials[:, 0], partials[:, 1], partials[:, 2]
    return {"grad_x": (scale * (window(p0) + 2.0 * x * window(p1) + y * window(p2)), ssim_backward_abs(x, y, partials.abs(), scale))}


def ssim_backward_abs(x, y, b, scale):
    """The same map over absolute values: the scale of ssim_backward, and what it makes of per-element bounds b [C,3,H,W]."""
    return abs(scale) * (window(b[:, 0]) + 2.0 * x.abs() * window(b[:, 1]) + y.abs() * window(b[:, 2]))


def ssim_value_and_grad(x, y):
    """train_step.ssim (five grouped conv2d calls with the 11 x 11 outer-product window, zero padding) under autograd, as a SUM over
    the map: {"sum", "grad": d sum / d x}.  train_step builds its window as a float32 tensor, so its body is restated here in the
    inputs' dtype with the window from the same eleven float32 taps (tests/test_stencil_reference_cpu.py pins both)."""
    x = _leaf(x)
    C = x.shape[0]
    g = torch.tensor(SSIM_WIN, dtype=x.dtype)
    w = (g[:, None] @ g[None, :])[None, None].expand(C, 1, 11, 11).contiguous()
    conv = lambda t: F.conv2d(t[None], w, padding=5, groups=C)
    mu1, mu2 = conv(x), conv(y)
    s1, s2, s12 = conv(x * x) - mu1.pow(2), conv(y * y) - mu2.pow(2), conv(x * y) - mu1 * mu2
    m = ((2 * mu1 * mu2 + SSIM_C1) * (2 * s12 + SSIM_C2)) / ((mu1.pow(2) + mu2.pow(2) + SSIM_C1) * (s1 + s2 + SSIM_C2))
    total = m.sum()
    gx, = _grad(total, [x])
    return {"sum": total.detach(), "grad": gx}


# ---- edge-aware smoothness ------------------------------------------------------------------------------------------------------------
def _edge_sum(data, guide):
    """first_order_edge_aware_loss(data, guide) * (its mean's count): sum_{c,d} |G_d data_c| exp(-|G_d guide_c|), [C,H,W] maps (one
    data channel against three guide channels broadcasts, as in train_step)."""
    return (sobel(data).abs() * torch.exp(-sobel(guide).abs())).sum()


def _adjoint_abs(ev):
    """Scale of the stencil's adjoint: sum over the nine taps of |weight| * ev (ev [C,2,H,W] >= 0) -> [C,H,W]."""
    leaf = torch.zeros(1, ev.shape[0], ev.shape[2], ev.shape[3], dtype=ev.dtype).requires_grad_(True)
    with torch.enable_grad():
        g, = _grad((_sobel_abs(leaf)[0] * ev).sum(), [leaf])
    return g[0]


def _abs_stencil(v):
    return _sobel_abs(v.abs()[None])[0]


def stage2_smooth(W, H, opacity, feature, n_contrib, gt, mask, w_base, w_rough, w_light):
    """r3dg_stage2_smooth_forward + _backward / r3dg_stage2_smooth_fused on flattened maps (opacity [HW], feature [16,HW], gt [3,HW],
    mask [HW] or None): the three unweighted sums of the ACTIVE terms and the terms' gradients dL_dopacity [HW] and planes 5..14 of
    dL_dfeature [10,HW] (what the kernels add to / write over the buffers they are handed).  The diffuse-light guide is the rendered
    normal and is not detached."""
    opacity, feature = _leaf(opacity), _leaf(feature)
    img = lambda t: t.reshape(-1, H, W)
    feat, sc, opc = divided(opacity, feature, n_contrib)
    mk = torch.ones_like(opacity) if mask is None else mask
    xb, xl = feat[8:11], feat[12:15]
    base, rough, light, normal = img(rgb_to_srgb(xb) * mk), img(feat[11:12] * mk), img(rgb_to_srgb(xl) * mk), img(feat[5:8])
    g3 = img(gt)
    sums, L = {}, opacity.sum() * 0.0
    if w_base != 0.0:
        sums["sum_base"] = _edge_sum(base, g3)
        L = L + w_base * sums["sum_base"]
    if w_rough != 0.0:
        sums["sum_rough"] = _edge_sum(rough, g3)
        L = L + w_rough * sums["sum_rough"]
    if w_light != 0.0:
        sums["sum_light"] = _edge_sum(light, normal)
        L = L + w_light * sums["sum_light"]
    dsr_b, dsr_l = _grad(rgb_to_srgb(xb).sum() + rgb_to_srgb(xl).sum(), [xb, xl], retain_graph=True)
    go, gf = _grad(L, [opacity, feature])
    with torch.no_grad():
        flat = lambda t: t.reshape(t.shape[0], -1)
        e = torch.exp(-sobel(g3).abs())                                    # [3,2,H,W]
        gn = torch.exp(-sobel(normal).abs())
        on = lambda v: torch.sign(v).abs()
        dsc = torch.where((n_contrib > 0) & (opacity >= OP_MIN), 1.0 / (opc * opc), torch.zeros_like(opc))
        s_g = torch.zeros(10, W * H, dtype=opacity.dtype)                  # scale of dL / d (divided map), planes 5..14
        out = {}
        if w_base != 0.0:
            s_g[3:6] = flat(_adjoint_abs(abs(w_base) * on(sobel(base)) * e)) * mk.abs() * dsr_b.abs()
            out["sum_base"] = (sums["sum_base"].detach(), (_abs_stencil(base) * e).sum())
        if w_rough != 0.0:
            es = e.sum(0, keepdim=True)
            s_g[6:7] = flat(_adjoint_abs(abs(w_rough) * on(sobel(rough)) * es)) * mk.abs()
            out["sum_rough"] = (sums["sum_rough"].detach(), (_abs_stencil(rough) * es).sum())
        if w_light != 0.0:
            s_g[7:10] = flat(_adjoint_abs(abs(w_light) * on(sobel(light)) * gn)) * mk.abs() * dsr_l.abs()
            # the guide's edge value -w |G dl| exp(-|G n|) sign(G n): |G dl| is itself rounded against the stencil's absolute sum
            s_g[0:3] = flat(_adjoint_abs(abs(w_light) * _abs_stencil(light) * gn * on(sobel(normal))))
            out["sum_light"] = (sums["sum_light"].detach(), (_abs_stencil(light) * gn).sum())
        out["dL_dfeature"] = (gf[5:15], s_g * sc)
        out["dL_dopacity"] = (go, (s_g * feature[5:15].abs() * dsc).sum(0))
        return out


def stage1_depth_smooth(W, H, opacity, feature, n_contrib, gt, w_smooth):
    """r3dg_stage1_depth_smooth on the S = 5 feature image [5,HW]: depth = map 3, ONE data channel against the target's three;
    the unweighted sum, dL_dopacity [HW] and dL_dfeature [5,HW] (only map 3 is not 0) -- the terms the kernel ADDS."""
    opacity, feature = _leaf(opacity), _leaf(feature)
    feat, sc, opc = divided(opacity, feature, n_contrib)
    depth, g3 = feat[3:4].reshape(1, H, W), gt.reshape(3, H, W)
    total = _edge_sum(depth, g3)
    go, gf = _grad(w_smooth * total, [opacity, feature])
    with torch.no_grad():
        es = torch.exp(-sobel(g3).abs()).sum(0, keepdim=True)
        s_d = _adjoint_abs(abs(w_smooth) * torch.sign(sobel(depth)).abs() * es).reshape(1, -1)
        dsc = torch.where((n_contrib > 0) & (opacity >= OP_MIN), 1.0 / (opc * opc), torch.zeros_like(opc))
        s_gf = torch.zeros_like(gf)
        s_gf[3:4] = s_d * sc
        return {"sum_depth": (total.detach(), (_abs_stencil(depth) * es).sum()), "dL_dfeature": (gf, s_gf),
                "dL_dopacity": (go, s_d[0] * feature[3].abs() * dsc)}
