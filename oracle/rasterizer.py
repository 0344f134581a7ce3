"""CPU oracle for the rasterizer op -- TEST INFRASTRUCTURE ONLY.

Python face of oracle/rasterizer_oracle.c.  `rasterize_gaussians` / `rasterize_gaussians_backward`
take the same arguments as the reference's `_C.rasterize_gaussians` / `_C.rasterize_gaussians_backward`
(r3dg-rasterization/rasterize_points.h:18-71) on CPU tensors / numpy arrays, and return the same tuples,
except that the three opaque byte buffers are replaced by one dict of named intermediates (the reference
keeps their layout private).

The product package never imports this module.
"""
import ctypes as C

import numpy as np

from . import _build

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(_build.build())
        _lib.r3dgo_scan.restype = C.c_int64
        _lib.r3dgo_getHigherMsb.restype = C.c_uint32
        _lib.r3dgo_render_backward_bounds.restype = None
    return _lib


def _np(t, dtype=np.float32):
    if t is None:
        return None
    if hasattr(t, "detach"):
        t = t.detach().cpu().numpy()
    a = np.ascontiguousarray(t, dtype=dtype)
    return a


def _p(a):
    if a is None or a.size == 0:
        return None
    return a.ctypes.data_as(C.c_void_p)


def _opt(t):
    a = _np(t)
    if a is None or a.size == 0:
        return None
    return a


def rasterize_gaussians(bg, means3D, features, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                        viewmatrix, projmatrix, tan_fovx, tan_fovy, cx, cy, image_height, image_width, sh, degree,
                        campos, prefiltered=False, computer_pseudo_normal=True, debug=False, want_margin=False):
    L = lib()
    means3D = _np(means3D)
    P = means3D.shape[0]
    H, W = int(image_height), int(image_width)
    features = _np(features).reshape(P, -1)
    S = features.shape[1]
    colors, scales, rotations, cov3D_precomp, sh = map(_opt, (colors, scales, rotations, cov3D_precomp, sh))
    opacity = _np(opacity).reshape(-1)
    bg, viewmatrix, projmatrix, campos = map(_np, (bg, viewmatrix, projmatrix, campos))
    M = sh.shape[1] if sh is not None else 0
    N = H * W
    gx, gy = (W + 15) // 16, (H + 15) // 16
    T = gx * gy

    st = dict(P=P, S=S, M=M, H=H, W=W)
    radii = np.zeros(P, np.int32)
    means2D = np.zeros((P, 2), np.float32)
    depths = np.zeros(P, np.float32)
    cov3D = np.zeros((P, 6), np.float32)
    rgb = np.zeros((P, 3), np.float32)
    conic_opacity = np.zeros((P, 4), np.float32)
    tiles_touched = np.zeros(P, np.uint32)
    clamped = np.zeros((P, 3), np.uint8)
    out_color = np.zeros((3, H, W), np.float32)
    out_opacity = np.zeros((1, H, W), np.float32)
    out_depth = np.zeros((1, H, W), np.float32)
    out_feature = np.zeros((S, H, W), np.float32)
    out_normal = np.zeros((3, H, W), np.float32)
    out_xyz = np.zeros((3, H, W), np.float32)
    weights = np.zeros(P, np.float64)
    n_contrib = np.zeros((H, W), np.uint32)
    final_T = np.zeros((H, W), np.float32)
    ranges = np.zeros((T, 2), np.uint32)
    num_rendered = 0
    if P != 0:
        L.r3dgo_preprocess(P, int(degree), M, _p(means3D), _p(scales), C.c_float(scale_modifier), _p(rotations),
                           _p(opacity), _p(sh), _p(cov3D_precomp), _p(colors), _p(viewmatrix), _p(projmatrix),
                           _p(campos), W, H, C.c_float(tan_fovx), C.c_float(tan_fovy), _p(radii), _p(means2D),
                           _p(depths), _p(cov3D), _p(rgb), _p(conic_opacity), _p(tiles_touched), _p(clamped))
        offsets = np.zeros(P, np.uint32)
        num_rendered = int(L.r3dgo_scan(P, _p(tiles_touched), _p(offsets)))
        R = num_rendered
        keys_u = np.zeros(R, np.uint64)
        vals_u = np.zeros(R, np.uint32)
        keys = np.zeros(R, np.uint64)
        vals = np.zeros(R, np.uint32)
        L.r3dgo_duplicate_with_keys(P, _p(means2D), _p(depths), _p(offsets), _p(radii), W, H, _p(keys_u), _p(vals_u))
        bit = int(L.r3dgo_getHigherMsb(C.c_uint32(T)))
        L.r3dgo_sort_pairs(C.c_int64(R), _p(keys_u), _p(vals_u), _p(keys), _p(vals), 32 + bit)
        L.r3dgo_identify_tile_ranges(C.c_int64(R), _p(keys), T, _p(ranges))
        colors_ptr = colors if colors is not None else rgb
        margin = np.zeros((H, W), np.float32) if want_margin else None
        L.r3dgo_render_forward(W, H, S, _p(ranges), _p(vals), _p(means2D), _p(depths), _p(features),
                               _p(colors_ptr), _p(conic_opacity), _p(bg), _p(final_T), _p(n_contrib), _p(out_color),
                               _p(out_opacity), _p(out_depth), _p(out_feature), _p(weights), _p(margin))
        if computer_pseudo_normal:
            fx = np.float32(W) / (np.float32(2.0) * np.float32(tan_fovx))
            fy = np.float32(H) / (np.float32(2.0) * np.float32(tan_fovy))
            L.r3dgo_pseudo_normal(W, H, _p(viewmatrix), C.c_float(fx), C.c_float(fy), C.c_float(cx), C.c_float(cy),
                                  _p(out_opacity), _p(out_depth), _p(out_normal), _p(out_xyz))
        st.update(offsets=offsets, keys_unsorted=keys_u, vals_unsorted=vals_u, keys=keys, point_list=vals,
                  sort_bits=32 + bit, margin=margin)
    st.update(radii=radii, means2D=means2D, depths=depths, cov3D=cov3D, rgb=rgb, conic_opacity=conic_opacity,
              tiles_touched=tiles_touched, clamped=clamped, final_T=final_T, n_contrib=n_contrib, ranges=ranges,
              num_rendered=num_rendered)
    return (num_rendered, n_contrib.astype(np.int32), out_color, out_opacity, out_depth, out_feature, out_normal,
            out_xyz, weights.reshape(P, 1), radii, st)


def rasterize_gaussians_backward(bg, means3D, features, radii, colors, scales, rotations, scale_modifier,
                                 cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color,
                                 dL_dout_opacity, dL_dout_depth, dL_dout_feature, sh, degree, campos, state,
                                 backward_geometry=True, debug=False, want_bounds=False, sum_mode=0, perturb=0.0,
                                 seed=0):
    """Returns the reference's 9-tuple (rasterize_points.cu:234) as float64 (accumulated in double) arrays, then dL_dconic.

    `want_bounds=True` appends a dict with the rounding scale of every tile-pass sum (r3dgo_render_backward_bounds):
    "E" -- per array ("mean2D" [P,3], "conic" [P,4], "opacity" [P,1], "colors" [P,3], "feature" [P,S]) the weighted absolute sum
    of the element's terms in units of one fp32 rounding (multiply by U = 2**-24); "count" -- the same keys, the number of terms;
    "E_pixel_form" [P,2] -- dL_dmean2D.xy's weighted absolute sum in the reference's per-pixel form (E holds the moment form).
    `sum_mode` / `perturb` / `seed` select that entry point's stand-ins for another correct fp32 implementation (fp32 sums in
    pixel order 1, reverse 2, per 8x8 block 3; perturbed exp / T / accum_rec steps); the per-Gaussian stage then runs on them."""
    L = lib()
    st = state
    means3D = _np(means3D)
    P, S, H, W = st["P"], st["S"], st["H"], st["W"]
    features = _np(features).reshape(P, -1)
    colors, scales, rotations, cov3D_precomp, sh = map(_opt, (colors, scales, rotations, cov3D_precomp, sh))
    bg, viewmatrix, projmatrix, campos = map(_np, (bg, viewmatrix, projmatrix, campos))
    M = sh.shape[1] if sh is not None else 0
    dC, dO, dD, dF = map(_np, (dL_dout_color, dL_dout_opacity, dL_dout_depth, dL_dout_feature))
    radii = _np(radii, np.int32)

    d_mean2D = np.zeros((P, 3), np.float64)
    d_conic = np.zeros((P, 4), np.float64)
    d_opacity = np.zeros((P, 1), np.float64)
    d_colors = np.zeros((P, 3), np.float64)
    d_feature = np.zeros((P, S), np.float64)
    d_means3D = np.zeros((P, 3), np.float32)
    d_cov3D = np.zeros((P, 6), np.float32)
    d_sh = np.zeros((P, M, 3), np.float32)
    d_scales = np.zeros((P, 3), np.float32)
    d_rot = np.zeros((P, 4), np.float32)
    if P != 0:
        color_ptr = colors if colors is not None else st["rgb"]
        if want_bounds or sum_mode or perturb:
            NC = 11 + S
            sums, E = np.zeros((P, NC), np.float64), np.zeros((P, NC), np.float64)
            e_pix, count = np.zeros((P, 2), np.float64), np.zeros(P, np.int32)
            L.r3dgo_render_backward_bounds(P, W, H, S, _p(st["ranges"]), _p(st["point_list"]), _p(bg), _p(st["means2D"]),
                                           _p(st["depths"]), _p(st["conic_opacity"]), _p(color_ptr), _p(features),
                                           _p(st["final_T"]), _p(st["n_contrib"]), _p(dC), _p(dO), _p(dD), _p(dF),
                                           int(bool(backward_geometry)), int(sum_mode), C.c_float(perturb),
                                           C.c_uint32(seed), _p(sums), _p(E), _p(e_pix), _p(count))
            cols = dict(mean2D=slice(0, 3), conic=slice(3, 7), opacity=slice(7, 8), colors=slice(8, 11),
                        feature=slice(11, NC))
            d_mean2D, d_conic, d_opacity, d_colors, d_feature = (
                np.ascontiguousarray(sums[:, cols[k]]) for k in ("mean2D", "conic", "opacity", "colors", "feature"))
            bounds = dict(E={k: np.ascontiguousarray(E[:, c]) for k, c in cols.items()},
                          count={k: np.repeat(count[:, None], c.stop - c.start, 1) for k, c in cols.items()},
                          E_pixel_form=e_pix)
            bounds["count"]["conic"][:, 2] = 0
        else:
            L.r3dgo_render_backward(W, H, S, _p(st["ranges"]), _p(st["point_list"]), _p(bg), _p(st["means2D"]),
                                    _p(st["depths"]), _p(st["conic_opacity"]), _p(color_ptr), _p(features),
                                    _p(st["final_T"]), _p(st["n_contrib"]), _p(dC), _p(dO), _p(dD), _p(dF),
                                    int(bool(backward_geometry)), _p(d_mean2D), _p(d_conic), _p(d_opacity),
                                    _p(d_colors), _p(d_feature))
        fx = np.float32(W) / (np.float32(2.0) * np.float32(tan_fovx))
        fy = np.float32(H) / (np.float32(2.0) * np.float32(tan_fovy))
        cov_ptr = cov3D_precomp if cov3D_precomp is not None else st["cov3D"]
        d_conic32 = d_conic.astype(np.float32)
        d_mean2D32 = d_mean2D.astype(np.float32)
        d_colors32 = d_colors.astype(np.float32)
        L.r3dgo_cov2d_backward(P, _p(means3D), _p(radii), _p(cov_ptr), C.c_float(fx), C.c_float(fy),
                               C.c_float(tan_fovx), C.c_float(tan_fovy), _p(viewmatrix), _p(d_conic32),
                               _p(d_mean2D32), _p(d_means3D), _p(d_cov3D))
        L.r3dgo_preprocess_backward(P, int(degree), M, _p(means3D), _p(radii), _p(sh), _p(st["clamped"]),
                                    _p(scales), _p(rotations), C.c_float(scale_modifier), _p(projmatrix),
                                    _p(campos), _p(d_mean2D32), _p(d_means3D), _p(d_colors32), _p(d_cov3D),
                                    _p(d_sh), _p(d_scales), _p(d_rot))
    res = (d_mean2D, d_colors, d_opacity, d_means3D, d_feature, d_cov3D, d_sh, d_scales, d_rot, d_conic)
    if want_bounds:
        if P == 0:
            z = lambda n: np.zeros((0, n), np.float64)
            bounds = dict(E=dict(mean2D=z(3), conic=z(4), opacity=z(1), colors=z(3), feature=z(S)),
                          count=dict(mean2D=z(3), conic=z(4), opacity=z(1), colors=z(3), feature=z(S)), E_pixel_form=z(2))
        return res + (bounds,)
    return res


def mark_visible(means3D, viewmatrix, projmatrix=None):
    means3D = _np(means3D)
    P = means3D.shape[0]
    present = np.zeros(P, np.uint8)
    if P:
        lib().r3dgo_mark_visible(P, _p(means3D), _p(_np(viewmatrix)), _p(present))
    return present.astype(bool)


# ---- the per-Gaussian stage on its own, in float64 -------------------------------------------------------------------------
def per_gaussian_backward_f64(means3D, scales, rotations, scale_modifier, cov3D_precomp, sh, degree, viewmatrix, projmatrix,
                              tan_fovx, tan_fovy, campos, W, H, radii, clamped, d_mean2D, d_conic, d_colors, jitter=None):
    """The chain behind the tile pass -- conic -> 2-D -> 3-D covariance -> scales / rotations, projection -> dL_dmeans3D, SH
    backward under the forward's clamp mask (backward.cu:20-398) -- in float64, from GIVEN tile-pass results: d_mean2D [P,3]
    (xy the viewspace gradient, z the depth side channel), d_conic [P,4] in the op's convention (x, y, -, w with y the
    HALVED off-diagonal sum, backward.cu:601) and d_colors [P,3].  autograd of oracle/torch_rasterizer.preprocess supplies the
    vector-Jacobian products; the reference's deliberate deviations from the true derivative are kept: no gradient through the
    +-1.3 tan_fov clamp, the quaternion un-normalised, 1 / (denom^2 + 1e-7) in the conic's backward (backward.cu:207) -- that
    step is evaluated by the reference's formulas and fed back as the cotangent of the 2-D covariance -- and dL_dscales with
    respect to scale_modifier * scale (backward.cu:316-319 do not multiply by the modifier).
    `jitter=(seed, rel)`: every input element (means, scales and rotations or cov3D, matrices, camera centre, SH coefficients,
    the three sums) is multiplied by 1 + rel * r, r uniform in [-1, 1] -- the input conditioning of the stage.
    Returns float64 arrays dict(means3D [P,3], cov3D [P,6], sh [P,M,3], scales [P,3], rot [P,4]); rows with radii <= 0 are 0."""
    import torch

    from . import torch_rasterizer as trz
    gen = torch.Generator().manual_seed(int(jitter[0])) if jitter is not None else None

    def t64(a):
        if a is None:
            return None
        t = torch.from_numpy(np.array(_np(a, np.float64), dtype=np.float64))
        if gen is not None:
            t = t * (1.0 + float(jitter[1]) * (2.0 * torch.rand(t.shape, generator=gen, dtype=torch.float64) - 1.0))
        return t
    means = t64(means3D).requires_grad_(True)
    P = means.shape[0]
    cov_in, s_eff, rot = None, None, None
    scales, rotations, cov3D_precomp, sh = map(_opt, (scales, rotations, cov3D_precomp, sh))
    if cov3D_precomp is not None:
        cov_in = t64(cov3D_precomp).requires_grad_(True)
    else:
        s_eff = (t64(scales) * float(np.float32(scale_modifier))).requires_grad_(True)
        rot = t64(rotations).requires_grad_(True)
    shs = t64(sh).requires_grad_(True) if sh is not None else None
    vm, pm, cam = t64(viewmatrix), t64(projmatrix), t64(campos)
    g2, gcon, gcol = t64(d_mean2D), t64(d_conic), t64(d_colors)
    vis = torch.from_numpy(_np(radii, np.int32) > 0)
    pre = trz.preprocess(means, s_eff, 1.0, rot, None, None, 0, cov_in, torch.zeros(P, 3, dtype=torch.float64), vm, pm, cam,
                         int(W), int(H), float(tan_fovx), float(tan_fovy))
    cov3D = pre["cov3D"]
    if cov_in is None:
        cov3D.retain_grad()
    con = pre["conic"]
    det_c = con[:, 0] * con[:, 2] - con[:, 1] * con[:, 1]
    a, b, c = con[:, 2] / det_c, -con[:, 1] / det_c, con[:, 0] / det_c
    with torch.no_grad():                                              # backward.cu:200-216
        denom = a * c - b * b
        d2i = 1.0 / (denom * denom + 0.0000001)
        dcx, dcy, dcw = gcon[:, 0], gcon[:, 1], gcon[:, 3]
        dL_da = d2i * (-c * c * dcx + 2 * b * c * dcy + (denom - a * c) * dcw)
        dL_dc = d2i * (-a * a * dcw + 2 * a * b * dcy + (denom - a * c) * dcx)
        dL_db = d2i * 2 * (b * c * dcx - (denom + 2 * b * b) * dcy + a * b * dcw)
    zero = torch.zeros((), dtype=torch.float64)
    loss = torch.where(vis, a * dL_da + b * dL_db + c * dL_dc, zero).sum()
    loss = loss + torch.where(vis[:, None], pre["p_proj_xy"] * g2[:, :2], zero).sum()
    loss = loss + torch.where(vis, pre["depths"] * g2[:, 2], zero).sum()
    if shs is not None:
        d = means - cam[None]
        d = d / d.norm(dim=-1, keepdim=True)
        raw = trz.sh_to_rgb(int(degree), shs, d)
        live = vis[:, None] & ~torch.from_numpy(_np(clamped, np.uint8).reshape(P, 3) != 0)
        loss = loss + torch.where(live, raw * gcol, zero).sum()
    loss.backward()

    def out(t, shape):
        if t is None or t.grad is None:
            return np.zeros(shape, np.float64)
        g = t.grad.numpy().reshape(P, -1).copy()
        g[~vis.numpy()] = 0.0
        return g.reshape(shape)
    M = shs.shape[1] if shs is not None else 0
    return dict(means3D=out(means, (P, 3)), cov3D=out(cov3D if cov_in is None else cov_in, (P, 6)), sh=out(shs, (P, M, 3)),
                scales=out(s_eff, (P, 3)), rot=out(rot, (P, 4)))


def per_gaussian_sigma(*args, n=8, rel=2.0 ** -23, base=None):
    """Input conditioning of the per-Gaussian stage: the largest change of every output element of
    per_gaussian_backward_f64(*args) over `n` seeded evaluations with every input perturbed by at most one fp32 ulp (relative
    2^-23).  Returns (unperturbed outputs, sigma), two dicts with the same keys."""
    if base is None:
        base = per_gaussian_backward_f64(*args)
    sigma = {k: np.zeros_like(v) for k, v in base.items()}
    for seed in range(n):
        p = per_gaussian_backward_f64(*args, jitter=(1000 + seed, rel))
        for k in sigma:
            sigma[k] = np.maximum(sigma[k], np.abs(p[k] - base[k]))
    return base, sigma
