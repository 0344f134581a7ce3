// The SSIM arithmetic every kernel that forms it compiles (ssim.hip: forward, backward, held-out metrics; image_tail.hip: the
// fused stage-2 tail): the eleven taps, the two kinds of separable pass -- the five window averages of an image pair, one plain
// map -- and the per-pixel function with its three partial derivatives.  Tiling and storage belong to the kernels.
#pragma once
#include "common.hpp"

namespace r3dg {

constexpr int SSIM_R = 5;                    // window radius (window_size 11)

// gaussian(11, 1.5) / sum, the fp32 values the reference's create_window produces (loss_utils.py:20-29)
inline __constant__ float kSsimWin[11] = {1.028380124e-03f, 7.598758209e-03f, 3.600077331e-02f, 1.093606874e-01f,
                                          2.130055279e-01f, 2.660117149e-01f, 2.130055279e-01f, 1.093606874e-01f,
                                          3.600077331e-02f, 7.598758209e-03f, 1.028380124e-03f};

__device__ __forceinline__ void ssim_load_window(float (&w)[11])
{
#pragma unroll
    for (int k = 0; k < 11; k++) w[k] = kSsimWin[k];
}

// first pass over an image pair: eleven taps of x, y, x^2, y^2, xy at xv[0..10], yv[0..10]
__device__ __forceinline__ void ssim_taps_pair(const float (&w)[11], const float* xv, const float* yv, float& a0, float& a1,
                                               float& a2, float& a3, float& a4)
{
    a0 = 0.f; a1 = 0.f; a2 = 0.f; a3 = 0.f; a4 = 0.f;
#pragma unroll
    for (int k = 0; k < 11; k++) {
        const float wx = w[k] * xv[k], wy = w[k] * yv[k];
        a0 += wx; a1 += wy; a2 += wx * xv[k]; a3 += wy * yv[k]; a4 += wx * yv[k];
    }
}

// eleven taps of a plain map at v[0..10] (the second pass of the forward, both passes of the backward); T = float, or float2v
// for two maps side by side: the same operations per component, as packed instructions
typedef float float2v __attribute__((ext_vector_type(2)));
template <class T>
__device__ __forceinline__ T ssim_taps(const float (&w)[11], const T* v)
{
    T a = 0.f;
#pragma unroll
    for (int k = 0; k < 11; k++) a += w[k] * v[k];
    return a;
}

// ssim_taps_pair on interleaved pairs xy[k] = (x, y): (a0, a1), (a2, a3) and a4 by the same operations per component
__device__ __forceinline__ void ssim_taps_pair_packed(const float (&w)[11], const float2v* xy, float2v& a01, float2v& a23, float& a4)
{
    a01 = 0.f; a23 = 0.f; a4 = 0.f;
#pragma unroll
    for (int k = 0; k < 11; k++) {
        const float2v wxy = w[k] * xy[k];
        a01 += wxy; a23 += wxy * xy[k]; a4 += wxy.x * xy[k].y;
    }
}

// SSIM of one pixel from its five window averages, and its partial derivatives w.r.t. mu1, E[x^2], E[xy] (treated as
// independent window averages)
template <bool PARTIALS>
__device__ __forceinline__ float ssim_pixel(float mu1, float mu2, float e11, float e22, float e12, float& p0, float& p1, float& p2)
{
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    const float A = 2.f * mu1 * mu2 + C1;
    const float B = 2.f * (e12 - mu1 * mu2) + C2;
    const float C = mu1 * mu1 + mu2 * mu2 + C1;
    const float D = (e11 - mu1 * mu1) + (e22 - mu2 * mu2) + C2;
    const float inv = 1.f / (C * D);
    const float ssim = A * B * inv;
    if constexpr (PARTIALS) {
        p0 = 2.f * mu2 * (B - A) * inv - ssim * 2.f * mu1 * (D - C) * inv;
        p1 = -ssim / D;
        p2 = 2.f * A * inv;
    }
    return ssim;
}

// the backward's last step for one pixel: the three window-averaged partial maps a0..a2 at a pixel with values x, y
__device__ __forceinline__ float ssim_grad_pixel(float scale, float a0, float a1, float a2, float x, float y)
{
    return scale * (a0 + 2.f * x * a1 + y * a2);
}

}  // namespace r3dg
