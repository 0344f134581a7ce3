// Stage-2 edge-aware smoothness terms in two formulations -- three passes through global memory, and the same streamed
// through registers as one kernel -- and their launchers.
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "launchers.hpp"
#include "glue_math.hpp"
#include "r3dg_hip.h"

namespace r3dg {

// ---- stage-2 edge-aware smoothness terms (Synthetic4Relight / DTU objective) ------------------------------------------
// neilf.py:275-292 with the flags of script/run_syn4.sh:34-36 / run_dtu.sh:36-38:
//   lambda_base_color_smooth * first_order_edge_aware_loss(base_color * m, gt)
// + lambda_roughness_smooth  * first_order_edge_aware_loss(roughness  * m, gt)        (1 channel against 3: broadcast)
// + lambda_light_smooth      * first_order_edge_aware_loss(diffuse    * m, rendered_normal)   (the guide is NOT detached)
// first_order_edge_aware_loss(data, img) = mean_{c,y,x} sum_d |G_d data_c| exp(-|G_d img_c|), G = Sobel / 8 with replicate
// padding (see the stage-1 comment above); X = feature_X / max(opacity, 1e-5) * (n_contrib > 0), m = the view's object mask.
// Three passes: (0) s2_smooth_maps_kernel materialises the ten divided (and masked) maps the stencils read; (A)
// s2_smooth_edge_kernel evaluates the stencils, adds the three sums and writes, per pixel, the 20 values the adjoint needs
// (weights folded in); (B) s2_smooth_backward_kernel gathers the adjoint of the replicate-padded stencil (no atomics) and
// applies the chain rule of the division into the feature-gradient maps and the opacity gradient r3dg_stage2_loss left.
// The base-colour and diffuse-light maps enter through the sRGB curve and its clip to [0,1] -- the loss reads
// results["base_color"] = rgb_to_srgb(rendered_base_color), results["diffuse"] likewise (neilf.py:153-155); the clip passes no
// gradient outside [0,1] -- the roughness map as rendered.
// rend layout [10][HW]: srgb(base_color)*m 0..2 | roughness*m 3 | srgb(diffuse)*m 4..6 | normal 7..9
// edge layout [20][HW]: base 2c+d (0..5) | roughness d (6,7) | diffuse 8+2c+d | normal guide 14+2c+d      (d: 0 = x, 1 = y)

// One tap of the stencils' adjoint and the chain rule behind it, shared by the three formulations of the smoothness terms below
// (three passes / LDS tiles / streamed): written with contraction off, so that the formulations agree bit for bit whatever
// contraction the compiler would pick for a * b + c * d in each context.
__device__ __forceinline__ float smooth_tap(float d, float wx, float ex, float wy, float ey)
{
#pragma clang fp contract(off)          // (HIP's __fmul_rn / __fadd_rn are inline operators that still fuse: this pins the roundings)
    const float t = wx * ex;
    const float u = __builtin_fmaf(wy, ey, t);
    return d + u;
}
// d[0..9]: dL / d (rend 0..9) of s2_smooth_maps_kernel at one pixel; f[0..9]: feature 5..14 there.  gf[0..9]: dL / d feature 5..14
// (normal 3 | base colour 3 | roughness | diffuse light 3; entries of absent terms untouched), returns dL / d opacity.
__device__ __forceinline__ float smooth_chain(bool base, bool rough, bool light, const float (&d)[10], float op, int nc, float m,
                                              const float (&f)[10], float (&gf)[10])
{
#pragma clang fp contract(off)
    const bool mask = nc > 0;
    const float opc = fmaxf(op, 1e-5f);
    const float scale = mask ? 1.f / opc : 0.f;
    const float dscale_dop = (mask && op >= 1e-5f) ? -1.f / (opc * opc) : 0.f;
    float g_op = 0.f;
    if (base) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float F = f[3 + c];
            const float g = d[c] * m * srgb_clip_derivative(F * scale);       // dL / d (linear base colour map)
            gf[3 + c] = g * scale;
            const float t = g * F * dscale_dop;
            g_op = g_op + t;
        }
    }
    if (rough) {
        const float g = d[3] * m;
        gf[6] = g * scale;
        const float t = g * f[6] * dscale_dop;
        g_op = g_op + t;
    }
    if (light) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float Fd = f[7 + c];
            const float g = d[4 + c] * m * srgb_clip_derivative(Fd * scale);   // dL / d (linear diffuse map)
            gf[7 + c] = g * scale;
            const float t = g * Fd * dscale_dop;
            g_op = g_op + t;
            const float gn = d[7 + c];
            gf[c] = gn * scale;
            const float u = gn * f[c] * dscale_dop;
            g_op = g_op + u;
        }
    }
    return g_op;
}

// `old_normal`: the three values the normal maps' gradient already holds at this pixel when the caller has read them ahead of
// time (the streamed kernel requests them before its nine taps: a load used straight away costs a wave its full latency), else NULL
__device__ __forceinline__ void smooth_store(bool base, bool rough, bool light, int accumulate_normal, const float (&gf)[10],
                                             size_t HW, size_t i, float* dL_dfeature,
                                             const float* old_normal = nullptr)
{
#pragma clang fp contract(off)
    if (base) {
#pragma unroll
        for (int c = 0; c < 3; c++) dL_dfeature[(size_t)(8 + c) * HW + i] = gf[3 + c];
    }
    if (rough) dL_dfeature[(size_t)11 * HW + i] = gf[6];
    if (light) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            dL_dfeature[(size_t)(12 + c) * HW + i] = gf[7 + c];
            const size_t o = (size_t)(5 + c) * HW + i;
            const float old = accumulate_normal ? (old_normal != nullptr ? old_normal[c] : dL_dfeature[o]) : 0.f;
            dL_dfeature[o] = old + gf[c];
        }
    }
}

__global__ void __launch_bounds__(256)
s2_smooth_maps_kernel(int HW, const float* __restrict__ opacity, const float* __restrict__ feature,
                      const int* __restrict__ n_contrib, const float* __restrict__ image_mask, float* __restrict__ rend)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= HW) return;
    const float scale = n_contrib[i] > 0 ? 1.f / fmaxf(opacity[i], 1e-5f) : 0.f;
    const float m = image_mask ? image_mask[i] : 1.f;
#pragma unroll
    for (int c = 0; c < 7; c++) {
        const float x = feature[(size_t)(8 + c) * HW + i] * scale;
        // results["base_color"] / results["diffuse"] are rgb_to_srgb(.) with its clip to [0,1] (neilf.py:153-155); roughness is not
        rend[(size_t)c * HW + i] = (c == 3 ? x : srgb_clip(x)) * m;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) rend[(size_t)(7 + c) * HW + i] = feature[(size_t)(5 + c) * HW + i] * scale;
}

__device__ __forceinline__ void sobel3(const float* __restrict__ map, int W, const int (&ys)[3], const int (&xs)[3],
                                       float& gx, float& gy)
{
    float v[3][3];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) v[a][b] = map[(size_t)ys[a] * W + xs[b]];
    gx = ((v[0][2] - v[0][0]) + 2.f * (v[1][2] - v[1][0]) + (v[2][2] - v[2][0])) * 0.125f;
    gy = ((v[2][0] - v[0][0]) + 2.f * (v[2][1] - v[0][1]) + (v[2][2] - v[0][2])) * 0.125f;
}

__global__ void __launch_bounds__(256)
s2_smooth_edge_kernel(int W, int H, const float* __restrict__ rend, const float* __restrict__ gt, float w_base,
                      float w_rough, float w_light, float* __restrict__ edge, float* __restrict__ sums3)
{
    __shared__ float s_part[4];
    const size_t HW = (size_t)W * H;
    float a_base = 0.f, a_rough = 0.f, a_light = 0.f;
    for (size_t i = blockIdx.x * 256 + threadIdx.x; i < HW; i += (size_t)gridDim.x * 256) {
        const int y = (int)(i / W), x = (int)(i % W);
        const int ys[3] = {y > 0 ? y - 1 : 0, y, y < H - 1 ? y + 1 : H - 1};
        const int xs[3] = {x > 0 ? x - 1 : 0, x, x < W - 1 ? x + 1 : W - 1};
        float ex[3], ey[3];                       // exp(-|G_d gt_c|)
        if (w_base != 0.f || w_rough != 0.f) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                float gx, gy;
                sobel3(gt + (size_t)c * HW, W, ys, xs, gx, gy);
                ex[c] = __expf(-fabsf(gx));
                ey[c] = __expf(-fabsf(gy));
            }
        }
        if (w_base != 0.f) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                float dx, dy;
                sobel3(rend + (size_t)c * HW, W, ys, xs, dx, dy);
                a_base += fabsf(dx) * ex[c] + fabsf(dy) * ey[c];
                edge[(size_t)(2 * c) * HW + i] = w_base * signf_(dx) * ex[c];
                edge[(size_t)(2 * c + 1) * HW + i] = w_base * signf_(dy) * ey[c];
            }
        }
        if (w_rough != 0.f) {
            float dx, dy;
            sobel3(rend + (size_t)3 * HW, W, ys, xs, dx, dy);
            const float sx = ex[0] + ex[1] + ex[2], sy = ey[0] + ey[1] + ey[2];
            a_rough += fabsf(dx) * sx + fabsf(dy) * sy;
            edge[(size_t)6 * HW + i] = w_rough * signf_(dx) * sx;
            edge[(size_t)7 * HW + i] = w_rough * signf_(dy) * sy;
        }
        if (w_light != 0.f) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                float dx, dy, nx, ny;
                sobel3(rend + (size_t)(4 + c) * HW, W, ys, xs, dx, dy);
                sobel3(rend + (size_t)(7 + c) * HW, W, ys, xs, nx, ny);
                const float gx = __expf(-fabsf(nx)), gy = __expf(-fabsf(ny));
                a_light += fabsf(dx) * gx + fabsf(dy) * gy;
                edge[(size_t)(8 + 2 * c) * HW + i] = w_light * signf_(dx) * gx;
                edge[(size_t)(9 + 2 * c) * HW + i] = w_light * signf_(dy) * gy;
                // d/d(G_d n_c) of |G_d dl_c| exp(-|G_d n_c|)
                edge[(size_t)(14 + 2 * c) * HW + i] = -w_light * fabsf(dx) * gx * signf_(nx);
                edge[(size_t)(15 + 2 * c) * HW + i] = -w_light * fabsf(dy) * gy * signf_(ny);
            }
        }
    }
    const float t0 = block_sum_256(a_base, s_part);
    __syncthreads();
    const float t1 = block_sum_256(a_rough, s_part);
    __syncthreads();
    const float t2 = block_sum_256(a_light, s_part);
    if (threadIdx.x == 0) {
        atomicAdd(sum_slot(sums3 + 0 * R3DG_SUM_SLOTS), t0);
        atomicAdd(sum_slot(sums3 + 1 * R3DG_SUM_SLOTS), t1);
        atomicAdd(sum_slot(sums3 + 2 * R3DG_SUM_SLOTS), t2);
    }
}

__global__ void __launch_bounds__(256)
s2_smooth_backward_kernel(int W, int H, const float* __restrict__ opacity, const float* __restrict__ feature,
                          const int* __restrict__ n_contrib, const float* __restrict__ image_mask,
                          const float* __restrict__ edge, int has_base, int has_rough, int has_light,
                          int accumulate_normal, float* __restrict__ dL_dopacity, float* __restrict__ dL_dfeature)
{
    const size_t HW = (size_t)W * H;
    for (size_t i = blockIdx.x * 256 + threadIdx.x; i < HW; i += (size_t)gridDim.x * 256) {
        const int y = (int)(i / W), x = (int)(i % W);
        // adjoint of the replicate-padded stencils: d[k] = dL / d rend_k at this pixel
        float d[10];
#pragma unroll
        for (int k = 0; k < 10; k++) d[k] = 0.f;
#pragma unroll
        for (int a = -1; a <= 1; a++) {
            const int qy = y + a;
            if (qy < 0 || qy >= H) continue;
            const float sy = s1_adj1(qy, y, H, 1.f, 2.f, 1.f), dy = s1_adj1(qy, y, H, -1.f, 0.f, 1.f);
#pragma unroll
            for (int b = -1; b <= 1; b++) {
                const int qx = x + b;
                if (qx < 0 || qx >= W) continue;
                const float sx = s1_adj1(qx, x, W, 1.f, 2.f, 1.f), dx = s1_adj1(qx, x, W, -1.f, 0.f, 1.f);
                const float wx = sy * dx * 0.125f, wy = dy * sx * 0.125f;
                const size_t q = (size_t)qy * W + qx;
                auto E = [&](int k) { return edge[(size_t)k * HW + q]; };
                if (has_base) {
#pragma unroll
                    for (int c = 0; c < 3; c++) d[c] = smooth_tap(d[c], wx, E(2 * c), wy, E(2 * c + 1));
                }
                if (has_rough) d[3] = smooth_tap(d[3], wx, E(6), wy, E(7));
                if (has_light) {
#pragma unroll
                    for (int c = 0; c < 3; c++) {
                        d[4 + c] = smooth_tap(d[4 + c], wx, E(8 + 2 * c), wy, E(9 + 2 * c));
                        d[7 + c] = smooth_tap(d[7 + c], wx, E(14 + 2 * c), wy, E(15 + 2 * c));
                    }
                }
            }
        }
        float f[10], gf[10];
#pragma unroll
        for (int c = 0; c < 10; c++) {
            const bool used = (c < 3) ? has_light : (c < 6) ? has_base : (c == 6) ? has_rough : has_light;
            f[c] = used ? feature[(size_t)(5 + c) * HW + i] : 0.f;
        }
        const float g_op = smooth_chain(has_base, has_rough, has_light, d, opacity[i], n_contrib[i],
                                        image_mask ? image_mask[i] : 1.f, f, gf);
        smooth_store(has_base, has_rough, has_light, accumulate_normal, gf, HW, i, dL_dfeature);
        dL_dopacity[i] += g_op;
    }
}

// ---- the three passes above as ONE kernel, streamed through registers (round 4) -------------------------------------------------
// maps -> edge -> backward move, per pixel, 10 divided maps out and back in, 20 adjoint inputs out and -- nine times, through the
// caches -- back in: 0.41 ms of the 2.0 ms DTU iteration (1600x1200).  None of that has to exist in HBM.  (A
// first fused version staged 32 x 8 pixel tiles + halo in 50 KB of LDS: 1.69x the loads for the halo of 2, two thirds empty
// second rounds, three barriers per 256 pixels, three workgroups per CU -- 0.148 ms where this one takes 0.102; deleted.)
// Nothing of the stencil needs a tile: lane = COLUMN, the wave walks DOWN the image.  The left / right neighbours of a value are one DPP lane shift away (wave_shr:1 / wave_shl:1 fold
// into the consuming instruction), the rows above live in registers:
//   per input row   13 maps of this column (divided / masked / sRGB-mapped as in s2_smooth_maps_kernel), their horizontal
//                   differences; with the two rows before: the Sobel pair of the row in the middle (gx from the three rows'
//                   differences, gy from the lane-shifted difference of the outer rows -- the reference expression, term by term),
//                   its 20 adjoint inputs;
//   two rows later  the adjoint of the row whose three edge rows are now complete: nine (row, lane shift) taps in the order of
//                   s2_smooth_backward_kernel, then the chain rule, written once.
// A wave owns 60 columns (lanes 2..61; the two lanes either side are the halo of the two stencil levels) x `rows` rows (+4 rows
// of run-in); replicate padding = clamped load coordinates.  No LDS, no barrier, every load a full 256-byte row segment.
constexpr int SS_OWN = 60;

__device__ __forceinline__ float lane_left(float v)      // the value of lane - 1 (wave_shr:1)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138, 0xF, 0xF, true));
}
__device__ __forceinline__ float lane_right(float v)     // the value of lane + 1 (wave_shl:1)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x130, 0xF, 0xF, true));
}

struct SmoothRow {            // what one pixel of a row contributes, as loaded
    float op, mk;
    int nc;
    float f[10];              // feature 5..14: normal 3 | base colour 3 | roughness | diffuse light 3
    float t[3];               // target
};

template <bool BASE, bool ROUGH, bool LIGHT, bool TARGET>
__device__ __forceinline__ SmoothRow smooth_load_row(size_t i, size_t HW, const float* __restrict__ opacity,
                                                     const float* __restrict__ feature, const int* __restrict__ n_contrib,
                                                     const float* __restrict__ gt, const float* __restrict__ image_mask)
{
    SmoothRow r;
    r.op = opacity[i];
    r.nc = n_contrib[i];
    r.mk = image_mask ? image_mask[i] : 1.f;
#pragma unroll
    for (int c = 0; c < 10; c++) {
        const bool used = (c < 3) ? LIGHT : (c < 6) ? BASE : (c == 6) ? ROUGH : LIGHT;
        r.f[c] = used ? feature[(size_t)(5 + c) * HW + i] : 0.f;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) r.t[c] = (TARGET && (BASE || ROUGH)) ? gt[(size_t)c * HW + i] : 0.f;
    return r;
}

template <bool BASE, bool ROUGH, bool LIGHT>
__global__ void __launch_bounds__(256, 2)      // (two waves per SIMD: all three terms together hold ~250 registers)
s2_smooth_stream_kernel(int W, int H, int rows, int strips_x, const float* __restrict__ opacity,
                        const float* __restrict__ feature, const int* __restrict__ n_contrib, const float* __restrict__ gt,
                        const float* __restrict__ image_mask, float w_base, float w_rough, float w_light, int accumulate_normal,
                        float* dL_dopacity, float* dL_dfeature, float* __restrict__ sums3)
{
    // dL_dopacity and dL_dfeature (planes 5-7 with accumulate_normal) are READ-MODIFY-WRITE: every element is read before it is
    // written, by the one lane that owns the pixel, and never read again.  They carry no __restrict__ (rounds 4-5 passed each buffer
    // a second time under a second restrict-qualified name for the reads -- outside the language's guarantees): the
    // compiler must now keep a row's stores in front of the next row's loads from the same array, which is the order the source
    // has them in anyway -- the old values are requested at the top of part (3), a full row of arithmetic ahead of their use.
    const int lane = threadIdx.x & 63;
    const int wid = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int strip = wid % strips_x, y0 = (wid / strips_x) * rows;
    if (y0 >= H) return;                                   // (whole waves; nothing below synchronises a workgroup)
    const int y1 = min(y0 + rows, H);
    const int x = strip * SS_OWN - 2 + lane;               // this lane's column; lanes 0, 1, 62, 63 are halo
    const int xc = min(max(x, 0), W - 1);
    const bool own_col = lane >= 2 && lane < 2 + SS_OWN && x < W;
    const size_t HW = (size_t)W * H;
    constexpr int NM = 13;                                 // rend 0..9 (layout of s2_smooth_maps_kernel), target 10..12
    auto used = [](int m) { return m < 3 ? BASE : m == 3 ? ROUGH : m < 10 ? LIGHT : (BASE || ROUGH); };
    // weights with which the stencils of columns x-1, x, x+1 read column x (replicate padding folded in); 0 outside the image
    float sxw[3], dxw[3];
#pragma unroll
    for (int b = -1; b <= 1; b++) {
        const int qx = x + b;
        const bool in = qx >= 0 && qx < W;
        sxw[b + 1] = in ? s1_adj1(qx, x, W, 1.f, 2.f, 1.f) : 0.f;
        dxw[b + 1] = in ? s1_adj1(qx, x, W, -1.f, 0.f, 1.f) : 0.f;
    }
    // three rows in flight: values, right - left, adjoint inputs.  Row r lives in slot r % 3; the loop is unrolled by three so
    // that the slots are compile-time names (registers), not copies
    float V[3][NM], D[3][NM], E[3][20];
#pragma unroll
    for (int q = 0; q < 3; q++) {
#pragma unroll
        for (int m = 0; m < NM; m++) V[q][m] = D[q][m] = 0.f;
#pragma unroll
        for (int k = 0; k < 20; k++) E[q][k] = 0.f;
    }
    float a_base = 0.f, a_rough = 0.f, a_light = 0.f;
    const int nrows = y1 - y0;
    SmoothRow nxt = smooth_load_row<BASE, ROUGH, LIGHT, true>((size_t)min(max(y0 - 2, 0), H - 1) * W + xc, HW, opacity, feature,
                                                              n_contrib, gt, image_mask);
    auto step = [&](auto slot, int r) {
        constexpr int P2 = decltype(slot)::value, P1 = (P2 + 2) % 3, P0 = (P2 + 1) % 3;
        float (&v2)[NM] = V[P2], (&v0)[NM] = V[P0];
        float (&h2)[NM] = D[P2], (&h1)[NM] = D[P1], (&h0)[NM] = D[P0];
        float (&E2)[20] = E[P2], (&E1)[20] = E[P1], (&E0)[20] = E[P0];
        const int yy = y0 - 2 + r;                         // incoming row; edge row yy - 1; adjoint row yy - 2
        const SmoothRow in = nxt;
        // (unconditionally -- the row index is clamped anyway: under `if (r + 1 < total)` the compiler merges the loaded
        // registers with the untouched ones INSIDE the branch, i.e. waits for the loads it has just issued: 44 % of the
        // wave-cycles of the first version)
        nxt = smooth_load_row<BASE, ROUGH, LIGHT, true>((size_t)min(max(yy + 1, 0), H - 1) * W + xc, HW, opacity, feature,
                                                        n_contrib, gt, image_mask);
        const int py = yy - 2;
        const bool adjoint = r >= 4 && own_col && py < y1;
        // (1) the incoming row's maps
        {
            const float scale = in.nc > 0 ? 1.f / fmaxf(in.op, 1e-5f) : 0.f;
#pragma unroll
            for (int c = 0; c < 7; c++) {
                const float xv = in.f[3 + c] * scale;
                v2[c] = (c == 3 ? xv : srgb_clip(xv)) * in.mk;
            }
#pragma unroll
            for (int c = 0; c < 3; c++) {
                v2[7 + c] = in.f[c] * scale;
                v2[10 + c] = in.t[c];
            }
#pragma unroll
            for (int m = 0; m < NM; m++) h2[m] = used(m) ? lane_right(v2[m]) - lane_left(v2[m]) : 0.f;
        }
        // (2) the edge row in the middle of the three
        const int cy = yy - 1;
        if (r >= 2 && cy >= 0 && cy < H) {
            const bool own = own_col && cy >= y0 && cy < y1;
            auto sobel = [&](int m, float& gx_, float& gy_) {
                const float vd = v2[m] - v0[m];
                gx_ = ((h0[m]) + 2.f * (h1[m]) + (h2[m])) * 0.125f;
                gy_ = ((lane_left(vd)) + 2.f * (vd) + (lane_right(vd))) * 0.125f;
            };
            float ex[3], ey3[3];
            if (BASE || ROUGH) {
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    float gx1, gy1;
                    sobel(10 + c, gx1, gy1);
                    ex[c] = __expf(-fabsf(gx1));
                    ey3[c] = __expf(-fabsf(gy1));
                }
            }
            if (BASE) {
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    float dx, dy;
                    sobel(c, dx, dy);
                    if (own) a_base += fabsf(dx) * ex[c] + fabsf(dy) * ey3[c];
                    E2[2 * c] = w_base * signf_(dx) * ex[c];
                    E2[2 * c + 1] = w_base * signf_(dy) * ey3[c];
                }
            }
            if (ROUGH) {
                float dx, dy;
                sobel(3, dx, dy);
                const float sx = ex[0] + ex[1] + ex[2], sy = ey3[0] + ey3[1] + ey3[2];
                if (own) a_rough += fabsf(dx) * sx + fabsf(dy) * sy;
                E2[6] = w_rough * signf_(dx) * sx;
                E2[7] = w_rough * signf_(dy) * sy;
            }
            if (LIGHT) {
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    float dx, dy, nx, ny;
                    sobel(4 + c, dx, dy);
                    sobel(7 + c, nx, ny);
                    const float gx1 = __expf(-fabsf(nx)), gy1 = __expf(-fabsf(ny));
                    if (own) a_light += fabsf(dx) * gx1 + fabsf(dy) * gy1;
                    E2[8 + 2 * c] = w_light * signf_(dx) * gx1;
                    E2[9 + 2 * c] = w_light * signf_(dy) * gy1;
                    E2[14 + 2 * c] = -w_light * fabsf(dx) * gx1 * signf_(nx);
                    E2[15 + 2 * c] = -w_light * fabsf(dy) * gy1 * signf_(ny);
                }
            }
        }
        // (3) the adjoint of row yy - 2 and the chain rule
        if (r >= 4 && py < y1) {
            // the adjoint row's own pixel again (cache hits; requested here, used after the nine taps)
            const SmoothRow pr = smooth_load_row<BASE, ROUGH, LIGHT, false>((size_t)py * W + xc, HW, opacity, feature, n_contrib,
                                                                            gt, image_mask);
            // ... and what the two read-modify-write outputs hold there (requested now, used after the nine taps: read where
            // they are used, these loads were 44 % of the wave-cycles -- `s_waitcnt` with two waves per SIMD to cover it)
            const float old_dop = dL_dopacity[(size_t)py * W + xc];
            float old_n[3] = {0.f, 0.f, 0.f};
            if (LIGHT && accumulate_normal) {
#pragma unroll
                for (int c = 0; c < 3; c++) old_n[c] = dL_dfeature[(size_t)(5 + c) * HW + (size_t)py * W + xc];
            }
            float d[10];
#pragma unroll
            for (int k = 0; k < 10; k++) d[k] = 0.f;
#pragma unroll
            for (int a = -1; a <= 1; a++) {
                const int qy = py + a;
                if (qy < 0 || qy >= H) continue;
                const float sy = s1_adj1(qy, py, H, 1.f, 2.f, 1.f), dy = s1_adj1(qy, py, H, -1.f, 0.f, 1.f);
                const float (&Er)[20] = a < 0 ? E0 : a == 0 ? E1 : E2;
#pragma unroll
                for (int b = -1; b <= 1; b++) {
                    const float wx = sy * dxw[b + 1] * 0.125f, wy = dy * sxw[b + 1] * 0.125f;
                    auto tap = [&](int k) { return b < 0 ? lane_left(Er[k]) : b == 0 ? Er[k] : lane_right(Er[k]); };
                    if (BASE) {
#pragma unroll
                        for (int c = 0; c < 3; c++) d[c] = smooth_tap(d[c], wx, tap(2 * c), wy, tap(2 * c + 1));
                    }
                    if (ROUGH) d[3] = smooth_tap(d[3], wx, tap(6), wy, tap(7));
                    if (LIGHT) {
#pragma unroll
                        for (int c = 0; c < 3; c++) {
                            d[4 + c] = smooth_tap(d[4 + c], wx, tap(8 + 2 * c), wy, tap(9 + 2 * c));
                            d[7 + c] = smooth_tap(d[7 + c], wx, tap(14 + 2 * c), wy, tap(15 + 2 * c));
                        }
                    }
                }
            }
            if (adjoint) {
                const size_t i = (size_t)py * W + x;
                float gf[10];
                const float g_op = smooth_chain(BASE, ROUGH, LIGHT, d, pr.op, pr.nc, pr.mk, pr.f, gf);
                smooth_store(BASE, ROUGH, LIGHT, accumulate_normal, gf, HW, i, dL_dfeature, old_n);
                dL_dopacity[i] = old_dop + g_op;
            }
        }
    };
    // nrows + 4 steps, rounded up to whole rounds of three: a step past the end loads clamped rows and stores nothing, and a
    // straight-line round has no control-flow merge in it -- at a merge the compiler copies the prefetched row's registers, which
    // means waiting for everything in flight including the stores just issued (a write round trip per step)
    const int total = (nrows + 4 + 2) / 3 * 3;
    for (int r = 0; r < total; r += 3) {
        step(std::integral_constant<int, 0>{}, r);
        step(std::integral_constant<int, 1>{}, r + 1);
        step(std::integral_constant<int, 2>{}, r + 2);
    }
    a_base = wave_sum_to_lane63(a_base);
    a_rough = wave_sum_to_lane63(a_rough);
    a_light = wave_sum_to_lane63(a_light);
    if (lane == 63) {
        if (BASE) atomicAdd(sum_slot(sums3 + 0 * R3DG_SUM_SLOTS), a_base);
        if (ROUGH) atomicAdd(sum_slot(sums3 + 1 * R3DG_SUM_SLOTS), a_rough);
        if (LIGHT) atomicAdd(sum_slot(sums3 + 2 * R3DG_SUM_SLOTS), a_light);
    }
}

// ---- launchers ------------------------------------------------------------------------------------------------------
void launch_s2_smooth_forward(hipStream_t s, int W, int H, const float* opacity, const float* feature, const int* n_contrib,
                              const float* gt, const float* image_mask, float w_base, float w_rough, float w_light,
                              float* scratch, float* sums3)
{
    const long long HW = (long long)W * H;
    float* rend = scratch;
    float* edge = scratch + 10 * HW;
    s2_smooth_maps_kernel<<<(int)((HW + 255) / 256), 256, 0, s>>>((int)HW, opacity, feature, n_contrib, image_mask, rend);
    check_launch(s, false, "s2_smooth_maps_kernel");
    s2_smooth_edge_kernel<<<(int)min((HW + 255) / 256, (long long)2048), 256, 0, s>>>(W, H, rend, gt, w_base, w_rough, w_light,
                                                                                 edge, sums3);
    check_launch(s, false, "s2_smooth_edge_kernel");
}

void launch_s2_smooth_backward(hipStream_t s, int W, int H, const float* opacity, const float* feature, const int* n_contrib,
                               const float* image_mask, const float* scratch, int has_base, int has_rough, int has_light,
                               int accumulate_normal, float* dL_dopacity, float* dL_dfeature)
{
    const long long HW = (long long)W * H;
    s2_smooth_backward_kernel<<<(int)min((HW + 255) / 256, (long long)2048), 256, 0, s>>>(
        W, H, opacity, feature, n_contrib, image_mask, scratch + 10 * HW, has_base, has_rough, has_light, accumulate_normal,
        dL_dopacity, dL_dfeature);
    check_launch(s, false, "s2_smooth_backward_kernel");
}

template <bool BASE, bool ROUGH, bool LIGHT>
static void launch_s2_smooth_stream_t(hipStream_t s, int W, int H, int rows, const float* opacity, const float* feature,
                                      const int* n_contrib, const float* gt, const float* image_mask, float w_base, float w_rough,
                                      float w_light, int accumulate_normal, float* dL_dopacity, float* dL_dfeature, float* sums3)
{
    const int strips_x = (W + SS_OWN - 1) / SS_OWN, strips_y = (H + rows - 1) / rows;
    const int waves = strips_x * strips_y;
    s2_smooth_stream_kernel<BASE, ROUGH, LIGHT><<<(waves + 3) / 4, 256, 0, s>>>(
        W, H, rows, strips_x, opacity, feature, n_contrib, gt, image_mask, w_base, w_rough, w_light, accumulate_normal,
        dL_dopacity, dL_dfeature, sums3);
}

void launch_s2_smooth_fused(hipStream_t s, int W, int H, const float* opacity, const float* feature, const int* n_contrib,
                            const float* gt, const float* image_mask, float w_base, float w_rough, float w_light,
                            int accumulate_normal, float* dL_dopacity, float* dL_dfeature, float* sums3)
{
    // rows per wave: every wave pays 4 rows of run-in; one full round of two waves per SIMD is ~2048 waves
    static const int rows_env = getenv("R3DG_SMOOTH_ROWS") ? atoi(getenv("R3DG_SMOOTH_ROWS")) : 0;
    const int strips_x = (W + SS_OWN - 1) / SS_OWN;
    int rows = rows_env > 0 ? rows_env : (int)std::min<long long>(32, std::max<long long>(8, ((long long)strips_x * H + 2047) / 2048));
    rows = std::max(1, std::min(rows, H));
    const int sel = (w_base != 0.f ? 1 : 0) | (w_rough != 0.f ? 2 : 0) | (w_light != 0.f ? 4 : 0);
#define R3DG_SMOOTH_CASE(n, B, R, L)                                                                                        \
    case n:                                                                                                                 \
        launch_s2_smooth_stream_t<B, R, L>(s, W, H, rows, opacity, feature, n_contrib, gt, image_mask, w_base, w_rough,     \
                                           w_light, accumulate_normal, dL_dopacity, dL_dfeature, sums3);                    \
        break;
    switch (sel) {
        R3DG_SMOOTH_CASE(1, true, false, false)
        R3DG_SMOOTH_CASE(2, false, true, false)
        R3DG_SMOOTH_CASE(3, true, true, false)
        R3DG_SMOOTH_CASE(4, false, false, true)
        R3DG_SMOOTH_CASE(5, true, false, true)
        R3DG_SMOOTH_CASE(6, false, true, true)
        R3DG_SMOOTH_CASE(7, true, true, true)
        default: return;                             // no term: nothing to add
    }
#undef R3DG_SMOOTH_CASE
    check_launch(s, false, "s2_smooth_stream_kernel");
}

}  // namespace r3dg
