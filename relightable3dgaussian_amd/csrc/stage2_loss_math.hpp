// Per-pixel arithmetic of the stage-2 image-space loss (neilf.py:190-318), compiled by every kernel that forms it:
// s2_pbr_srgb_kernel / s2_normals_srgb_kernel / s2_loss_kernel (stage2_glue.hip) and the fused tail (image_tail.hip).
#pragma once
#include "glue_math.hpp"

namespace r3dg {

// feat = feature * scale with scale = (n_contrib > 0) / max(opacity, 1e-5), and d scale / d opacity (the clamp passes no gradient)
struct S2Divide {
    float scale, dscale_dop;
};
__device__ __forceinline__ float s2_divide_scale(float op, int nc) { return nc > 0 ? 1.f / fmaxf(op, 1e-5f) : 0.f; }
__device__ __forceinline__ S2Divide s2_divide(float op, int nc)
{
    const bool mask = nc > 0;
    const float opc = fmaxf(op, 1e-5f);
    S2Divide d;
    d.scale = mask ? 1.f / opc : 0.f;
    d.dscale_dop = (mask && op >= 1e-5f) ? -1.f / (opc * opc) : 0.f;
    return d;
}

// one channel of the sRGB-mapped PBR image: pbr_img = feat * op + (1 - op) * bg, rgb_to_srgb with its clip
// (utils/graphics_utils.py:207-213)
__device__ __forceinline__ float s2_pbr_srgb_pixel(float F, float scale, float op, float bgc)
{
    const float v0 = F * scale * op + (1.f - op) * bgc;
    const float v = v0 <= 0.0031308f ? 12.92f * v0 : 1.055f * srgb_pow(fmaxf(v0, 0.0031308f), 1.f / 2.4f) - 0.055f;
    return fminf(fmaxf(v, 0.f), 1.f);
}

// L1 on the SH image, one channel: -> dL/dimage; extra = the gradient of further terms on the same image (the SSIM term)
__device__ __forceinline__ float s2_loss_image(float im, float g, float w_l1, float extra, float& s_l1)
{
    const float d0 = im - g;
    s_l1 += fabsf(d0);
    return w_l1 * signf_(d0) + extra;
}

// L1 on the sRGB-mapped PBR image, one channel: -> dL/dfeature[2 + c], its share of dL/dopacity added to g_op
__device__ __forceinline__ float s2_loss_pbr(float F, float g, float op, float bgc, const S2Divide dv, float w_pbr, float extra,
                                             float& s_pbr, float& g_op)
{
    const float scale = dv.scale;
    const float r = F * scale;
    const float x = r * op + (1.f - op) * bgc;
    const bool lin = x <= 0.0031308f;
    const float xs = fmaxf(x, 0.0031308f);
    // rgb_to_srgb with clip=True (utils/graphics_utils.py:207-213): the curve, then clamp to [0,1]; the clamp passes
    // the gradient only where 0 <= curve <= 1 (torch.clamp), so saturated HDR highlights stop pulling
    const float curve = lin ? 12.92f * x : 1.055f * srgb_pow(xs, 1.f / 2.4f) - 0.055f;
    const bool unclipped = curve >= 0.f && curve <= 1.f;
    const float srgb = fminf(fmaxf(curve, 0.f), 1.f);
    const float d1 = srgb - g;
    s_pbr += fabsf(d1);
    const float dsrgb = !unclipped ? 0.f : (lin ? 12.92f : 1.055f / 2.4f * srgb_pow(xs, 1.f / 2.4f - 1.f));
    const float gx = (w_pbr * signf_(d1) + extra) * dsrgb;   // dL/dx
    g_op += gx * (r - bgc + op * F * dv.dscale_dop);
    return gx * op * scale;
}

// normal consistency, one channel: mse(normal * m, pseudo_normal * m), m = the view's object mask (neilf.py:258-264)
// -> dL/dfeature[5 + c], its share of dL/dopacity added to g_op
__device__ __forceinline__ float s2_loss_normal(float Fn, float pn, float mk, const S2Divide dv, float w_normal, float& s_n, float& g_op)
{
    const float dn = (Fn * dv.scale - pn) * mk;
    s_n += dn * dn;
    const float gn = 2.f * w_normal * dn * mk;
    g_op += gn * Fn * dv.dscale_dop;
    return gn * dv.scale;
}

}  // namespace r3dg
