// Capture maps of an eval / relight frame (gaussian_renderer/neilf.py:146-182, the maps the reference's --capture_list and its
// evaluation scripts read) for gfx950, from the rasterizer's raw 28-channel feature image in ONE streaming pass:
//
//   relight_capture_kernel   per pixel x = feature / max(opacity, 1e-5) * (num_contrib > 0); base_color, diffuse, specular,
//                            lights, local_lights, global_lights through rgb_to_srgb with its clip; roughness, visibility,
//                            normal as rendered; depth_var = depth2 - depth^2; pbr = srgb(pbr * opacity + (1 - opacity) * bg).
//                            With a mask every map but depth_var is then composited as x * mask + (1 - mask) * bg
//                            (eval_relighting_syn4.py:161-167).  Any output may be NULL: its channels are not read.
//
// Lane = pixel, every channel a coalesced row read of the [28,HW] image (channel layout: relight_pack_features_kernel); each
// channel is read once and nothing is kept across channels but the pixel's divisor, so there is nothing to spill.
// Parity target: evaluate.capture_reference (PyTorch).
#include "capture_math.hpp"
#include "launchers.hpp"

namespace r3dg {

// x * mask + (1 - mask) * bg, each operation rounded on its own as the PyTorch expression is (no contraction into an FMA)
__device__ __forceinline__ float over_background(float x, float m, float bg)
{
#pragma clang fp contract(off)
    const float a = x * m, b = (1.f - m) * bg;
    return a + b;
}
// (variance_of, normalised, capture_divisor, pbr_over_background: capture_math.hpp, shared with training_sheet.hip)

template <int N, bool SRGB>
__device__ __forceinline__ void capture_group(const float* __restrict__ feature, int c0, size_t HW, size_t i, float den,
                                              bool masked, float m, const float* __restrict__ bg, float* __restrict__ out)
{
    if (out == nullptr) return;
#pragma unroll
    for (int c = 0; c < N; c++) {
        const float x = normalised(feature[(size_t)(c0 + c) * HW + i], den);
        float v = SRGB ? srgb_of(x) : x;
        if (masked) v = over_background(v, m, bg[N == 1 ? 0 : c]);
        out[(size_t)c * HW + i] = v;
    }
}

__global__ void __launch_bounds__(256)
relight_capture_kernel(int HW_, const float* __restrict__ feature, const float* __restrict__ opacity,
                       const int* __restrict__ n_contrib, const float* __restrict__ background,
                       const float* __restrict__ mask, CaptureMaps maps)
{
    const size_t HW = (size_t)HW_, i = (size_t)blockIdx.x * 256 + threadIdx.x;     // (HW may lie within 256 of 2^31)
    if (i >= HW) return;
    const float op = opacity[i];
    const float den = capture_divisor(op, n_contrib[i]);             // rendered_feature / opacity * mask (neilf.py:146-147)
    const bool masked = mask != nullptr;
    const float m = masked ? mask[i] : 1.f;
    float bg[3] = {0.f, 0.f, 0.f};
    if (background != nullptr) { bg[0] = background[0]; bg[1] = background[1]; bg[2] = background[2]; }
    if (maps.depth_var != nullptr) {
        const float d = normalised(feature[i], den), d2 = normalised(feature[HW + i], den);
        maps.depth_var[i] = variance_of(d, d2);
    }
    if (maps.pbr != nullptr) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float pbr = normalised(feature[(size_t)(2 + c) * HW + i], den);
            float v = pbr_over_background(pbr, op, bg[c]);
            if (masked) v = over_background(v, m, bg[c]);
            maps.pbr[(size_t)c * HW + i] = v;
        }
    }
    capture_group<3, false>(feature, 5, HW, i, den, masked, m, bg, maps.normal);
    capture_group<3, true>(feature, 8, HW, i, den, masked, m, bg, maps.base_color);
    capture_group<1, false>(feature, 11, HW, i, den, masked, m, bg, maps.roughness);
    capture_group<3, true>(feature, 12, HW, i, den, masked, m, bg, maps.diffuse);
    capture_group<3, true>(feature, 15, HW, i, den, masked, m, bg, maps.specular);
    capture_group<3, true>(feature, 18, HW, i, den, masked, m, bg, maps.lights);
    capture_group<3, true>(feature, 21, HW, i, den, masked, m, bg, maps.local_lights);
    capture_group<3, true>(feature, 24, HW, i, den, masked, m, bg, maps.global_lights);
    capture_group<1, false>(feature, 27, HW, i, den, masked, m, bg, maps.visibility);
}

void launch_relight_capture(hipStream_t s, int W, int H, const float* feature, const float* opacity, const int* n_contrib,
                            const float* background, const float* mask, const CaptureMaps& maps)
{
    const int HW = W * H;
    relight_capture_kernel<<<(unsigned)(((size_t)HW + 255) / 256), 256, 0, s>>>(HW, feature, opacity, n_contrib, background, mask, maps);
    check_launch(s, false, "relight_capture_kernel");
}

}  // namespace r3dg
