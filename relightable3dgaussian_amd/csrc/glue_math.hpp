// Scalar helpers of the glue kernels (stage2_glue.hip, stage1_glue.hip, smooth.hip, relight.hip, eval_capture.hip,
// scene_assembly.hip, training_sheet.hip): the sRGB curve, the 8-bit quantisation, sigmoid, sign,
// F.normalize and its backward, the adjoint weight of the replicate-padded Sobel stencil.
#pragma once
#include "common.hpp"

namespace r3dg {

// x^y for the sRGB curve (x >= 0.0031308): v_log_f32 * y -> v_exp_f32, 3 instructions and ~4 ulp.  HIP's __powf is the
// full-precision library routine (~155 instructions, a software logarithm): 18 of them per pixel were three quarters of the
// smoothness kernels' instructions and most of s2_pbr_srgb_kernel.  (torch.pow in the reference's rgb_to_srgb,
// utils/graphics_utils.py, is itself good to ~2 ulp; the parity tolerances are 1e-5 and wider.)
__device__ __forceinline__ float srgb_pow(float x, float y) { return __builtin_amdgcn_exp2f(y * __builtin_amdgcn_logf(x)); }

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + __expf(-x)); }

// F.normalize(v, eps): v / max(|v|, eps)
__device__ __forceinline__ void normalize3(const float v[3], float eps, float out[3], float& inv)
{
    const float n = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    inv = 1.f / fmaxf(n, eps);
    out[0] = v[0] * inv; out[1] = v[1] * inv; out[2] = v[2] * inv;
}
// backward of v / max(|v|, eps): (g - n (n.g)) / |v| when |v| >= eps, g / eps below it (clamp passes no gradient)
__device__ __forceinline__ void normalize3_backward(const float v[3], float eps, const float g[3], float out[3])
{
    const float n = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (n > eps) {
        const float inv = 1.f / n;
        const float u[3] = {v[0] * inv, v[1] * inv, v[2] * inv};
        const float d = u[0] * g[0] + u[1] * g[1] + u[2] * g[2];
#pragma unroll
        for (int c = 0; c < 3; c++) out[c] = (g[c] - u[c] * d) * inv;
    } else {
        const float inv = 1.f / eps;
#pragma unroll
        for (int c = 0; c < 3; c++) out[c] = g[c] * inv;
    }
}

__device__ __forceinline__ float signf_(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }

// rgb_to_srgb with clip=True (utils/graphics_utils.py:207-213) and its derivative (0 where the clamp is active)
__device__ __forceinline__ float srgb_clip(float x)
{
    const float curve = x <= 0.0031308f ? 12.92f * x : 1.055f * srgb_pow(fmaxf(x, 0.0031308f), 1.f / 2.4f) - 0.055f;
    return fminf(fmaxf(curve, 0.f), 1.f);
}
__device__ __forceinline__ float srgb_clip_derivative(float x)
{
    const bool lin = x <= 0.0031308f;
    const float xs = fmaxf(x, 0.0031308f);
    const float curve = lin ? 12.92f * x : 1.055f * srgb_pow(xs, 1.f / 2.4f) - 0.055f;
    if (!(curve >= 0.f && curve <= 1.f)) return 0.f;
    return lin ? 12.92f : 1.055f / 2.4f * srgb_pow(xs, 1.f / 2.4f - 1.f);
}

// the same curve as the relight / eval frame's kernels write it (relight.hip, eval_capture.hip): one comparison, no derivative
__device__ __forceinline__ float srgb_of(float x)
{
    // rgb_to_srgb (utils/graphics_utils.py:207-213), clip=True
    // (x^(1/2.4) as v_log_f32 * y -> v_exp_f32, ~4 ulp: the library powf is ~155 instructions per channel of every pixel)
    const float p = __builtin_amdgcn_exp2f((1.0f / 2.4f) * __builtin_amdgcn_logf(fmaxf(x, 0.0031308f)));
    const float y = x > 0.0031308f ? p * 1.055f - 0.055f : 12.92f * x;
    return fminf(fmaxf(y, 0.f), 1.f);
}

// a value for an 8-bit image file as torchvision's save_image quantises it: clamp(x * 255 + 0.5, 0, 255) truncated, the product
// and the sum rounded separately; NaN -> 0 (r3dg_relight_quantize, r3dg_training_sheet)
__device__ __forceinline__ uint8_t quantize_byte(float x)
{
    const float v = __fadd_rn(__fmul_rn(x, 255.f), 0.5f);
    return (uint8_t)(int)fminf(fmaxf(v, 0.f), 255.f);
}

// sum_d [clamp(q + d, 0, n-1) == p] * k[d+1]: weight with which position q's replicate-padded 1-D stencil reads position p
__device__ __forceinline__ float s1_adj1(int q, int p, int n, float km, float k0, float kp)
{
    float w = (q == p) ? k0 : 0.f;
    const int qm = q > 0 ? q - 1 : 0, qp = q < n - 1 ? q + 1 : n - 1;
    w += (qm == p) ? km : 0.f;
    w += (qp == p) ? kp : 0.f;
    return w;
}

}  // namespace r3dg
