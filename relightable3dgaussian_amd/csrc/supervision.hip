// Loss terms of the reference's OptimizationParams that none of the four run scripts switches on, for the two fused iterations:
// the MVS depth / normal supervision of stage 2 (DTU and Tanks-and-Temples captures ship filtered Vis-MVSNet depth maps and the
// normals derived from them, Camera.depth / Camera.normal), the edge-aware depth smoothness and the per-Gaussian regularisers of
// stage 1.  Each is a memory-bound streaming pass that runs BESIDE the existing loss kernels: it adds to the gradient buffers
// they wrote (r3dg_stage2_loss / r3dg_stage2_smooth_fused, r3dg_stage1_loss, the rasterizer backward) and to sum slots of its own.
// With the terms' weights at zero (the default) nothing of this unit is launched.  Kernels, launchers and their C ABI live here.
#include <algorithm>

#include "capi_internal.hpp"
#include "glue_math.hpp"
#include "wave_reduce.hpp"
#include "r3dg_hip.h"

namespace r3dg {

// one add per WAVE: the slot of the wave's linear index (sum_slot(), common.hpp, spreads whole workgroups the same way)
__device__ __forceinline__ float* wave_sum_slot(float* sum)
{
    const unsigned w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    return sum + (w & (unsigned)(R3DG_SUM_SLOTS - 1));
}

// ---- ~sur_mask of neilf.py:243-247: pixels where the object mask and the MVS depth's validity agree -------------------
// Integer adds only: the count is the same bits on every run.
__global__ void __launch_bounds__(256)
sup_count_kernel(int HW, const float* __restrict__ gt_depth, const float* __restrict__ image_mask,
                 uint32_t* __restrict__ count)
{
    uint32_t c = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += gridDim.x * 256) {
        const bool m = image_mask ? image_mask[i] != 0.f : true;
        c += (m == (gt_depth[i] > 0.f)) ? 1u : 0u;
    }
    c = wave_sum_u32(c);
    if (lane_id() == 0 && c != 0) atomicAdd(count, c);
}

// ---- stage 2: lambda_depth (neilf.py:241-249) and lambda_normal_mvs_depth (neilf.py:266-273) ----------------------------------
//   w_depth * 1/count * sum_sel |depth - gt_depth|,  sel = (image_mask != 0) == (gt_depth > 0), count = #sel (sup_count_kernel)
// + w_normal * sum_c (normal_c dm - mvs_normal_c dm)^2,  dm = (gt_depth > 0)                 (w_normal carries the 1 / (3 H W))
// with depth = feature 0 and normal = features 5..7 of the S=16 image, each / max(opacity, 1e-5) * (n_contrib > 0): the quotient
// rule and the clamp convention of s2_loss_kernel's normal term.  sign(0) = 0 as in PyTorch's L1 backward; count == 0 gives a
// zero term (PyTorch: the mean of nothing, NaN).
__global__ void __launch_bounds__(256)
s2_supervision_kernel(int HW, const float* __restrict__ opacity, const float* __restrict__ feature,
                      const int* __restrict__ n_contrib, const float* __restrict__ gt_depth,
                      const float* __restrict__ mvs_normal, const float* __restrict__ image_mask,
                      const uint32_t* __restrict__ count, float w_depth, float w_normal, int accumulate_normal,
                      float* __restrict__ dL_dopacity, float* __restrict__ dL_dfeature, float* __restrict__ sums2)
{
    __shared__ float s_part[4];
    float s_d = 0.f, s_n = 0.f;
    float wd = 0.f;
    if (w_depth != 0.f) {
        const uint32_t n = *count;
        wd = n != 0 ? w_depth / (float)n : 0.f;
    }
    for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += gridDim.x * 256) {
        const float op = opacity[i];
        const bool mask = n_contrib[i] > 0;
        const float opc = fmaxf(op, 1e-5f);
        const float scale = mask ? 1.f / opc : 0.f;                 // feat = feature * scale
        const float dscale_dop = (mask && op >= 1e-5f) ? -1.f / (opc * opc) : 0.f;
        const float gd = gt_depth[i];
        const bool dm = gd > 0.f;
        float g_op = 0.f;
        if (w_depth != 0.f) {
            const bool m = image_mask ? image_mask[i] != 0.f : true;
            const float F = feature[i];
            const float diff = F * scale - gd;
            float g = 0.f;
            if (m == dm) {
                s_d += fabsf(diff);
                g = wd * signf_(diff);
            }
            dL_dfeature[i] = g * scale;
            g_op += g * F * dscale_dop;
        }
        if (w_normal != 0.f) {
            const float mk = dm ? 1.f : 0.f;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const size_t o = (size_t)(5 + c) * HW + i;
                const float Fn = feature[o];
                const float dn = (Fn * scale - mvs_normal[(size_t)c * HW + i]) * mk;
                s_n += dn * dn;
                const float gn = 2.f * w_normal * dn * mk;
                const float old = accumulate_normal ? dL_dfeature[o] : 0.f;
                dL_dfeature[o] = old + gn * scale;
                g_op += gn * Fn * dscale_dop;
            }
        }
        dL_dopacity[i] += g_op;
    }
    const float t0 = block_sum_256(s_d, s_part);
    __syncthreads();
    const float t1 = block_sum_256(s_n, s_part);
    if (threadIdx.x == 0) {
        if (w_depth != 0.f) atomicAdd(sum_slot(sums2), t0);
        if (w_normal != 0.f) atomicAdd(sum_slot(sums2 + R3DG_SUM_SLOTS), t1);
    }
}

// ---- stage 1: lambda_depth_smooth * first_order_edge_aware_loss(depth, gt) (render.py:175-179) ------------------------------
// depth = feature 3 of the S=5 image / max(opacity, 1e-5) * (n_contrib > 0); ONE data channel against the three of the target:
//   mean_{c,y,x} sum_d |G_d depth| exp(-|G_d gt_c|),  G = Sobel / 8 with replicate padding (the stencil of s1_edge_kernel).
// Pass A: per pixel sign(G_d depth) * sum_c exp(-|G_d gt_c|) for d = x, y, and the loss sum.  Pass B: the adjoint of the
// replicate-padded stencil, gathered (s1_adj1, as s1_loss_kernel gathers the normal term's), ADDED to what r3dg_stage1_loss wrote.
// (sup_depth is s1_rendered of stage1_glue.hip for map 3, restated: that unit and the headers it includes stay byte for byte what
// the committed counter files were collected from, kernel_sources.py)
__device__ __forceinline__ float sup_depth(const float* __restrict__ feature, const float* __restrict__ opacity,
                                           const int* __restrict__ n_contrib, size_t HW, size_t pix)
{
    const float opc = fmaxf(opacity[pix], 1e-5f);
    return n_contrib[pix] > 0 ? feature[3 * HW + pix] / opc : 0.f;
}

__global__ void __launch_bounds__(256)
s1_depth_edge_kernel(int W, int H, const float* __restrict__ feature, const float* __restrict__ opacity,
                     const int* __restrict__ n_contrib, const float* __restrict__ gt, float* __restrict__ edge_g /*[2][HW]*/,
                     float* __restrict__ sum_out)
{
    __shared__ float s_part[4];
    const size_t HW = (size_t)W * H;
    float acc = 0.f;
    for (size_t i = blockIdx.x * 256 + threadIdx.x; i < HW; i += (size_t)gridDim.x * 256) {
        const int y = (int)(i / W), x = (int)(i % W);
        const int ys[3] = {y > 0 ? y - 1 : 0, y, y < H - 1 ? y + 1 : H - 1};
        const int xs[3] = {x > 0 ? x - 1 : 0, x, x < W - 1 ? x + 1 : W - 1};
        float n[3][3];
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int b = 0; b < 3; b++) n[a][b] = sup_depth(feature, opacity, n_contrib, HW, (size_t)ys[a] * W + xs[b]);
        const float nx = ((n[0][2] - n[0][0]) + 2.f * (n[1][2] - n[1][0]) + (n[2][2] - n[2][0])) * 0.125f;
        const float ny = ((n[2][0] - n[0][0]) + 2.f * (n[2][1] - n[0][1]) + (n[2][2] - n[0][2])) * 0.125f;
        float ex = 0.f, ey = 0.f;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            float g[3][3];
#pragma unroll
            for (int a = 0; a < 3; a++)
#pragma unroll
                for (int b = 0; b < 3; b++) g[a][b] = gt[(size_t)c * HW + (size_t)ys[a] * W + xs[b]];
            const float gx = ((g[0][2] - g[0][0]) + 2.f * (g[1][2] - g[1][0]) + (g[2][2] - g[2][0])) * 0.125f;
            const float gy = ((g[2][0] - g[0][0]) + 2.f * (g[2][1] - g[0][1]) + (g[2][2] - g[0][2])) * 0.125f;
            ex += __expf(-fabsf(gx));
            ey += __expf(-fabsf(gy));
        }
        acc += fabsf(nx) * ex + fabsf(ny) * ey;
        edge_g[i] = signf_(nx) * ex;
        edge_g[HW + i] = signf_(ny) * ey;
    }
    const float t = block_sum_256(acc, s_part);
    if (threadIdx.x == 0) atomicAdd(sum_slot(sum_out), t);
}

__global__ void __launch_bounds__(256)
s1_depth_adjoint_kernel(int W, int H, const float* __restrict__ feature, const float* __restrict__ opacity,
                        const int* __restrict__ n_contrib, const float* __restrict__ edge_g, float w_smooth,
                        float* __restrict__ dL_dopacity, float* __restrict__ dL_dfeature)
{
    const size_t HW = (size_t)W * H;
    for (size_t i = blockIdx.x * 256 + threadIdx.x; i < HW; i += (size_t)gridDim.x * 256) {
        const int y = (int)(i / W), x = (int)(i % W);
        float dsm = 0.f;
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
                const size_t q = (size_t)qy * W + qx;
                dsm += sy * dx * 0.125f * edge_g[q] + dy * sx * 0.125f * edge_g[HW + q];
            }
        }
        const float op = opacity[i];
        const bool mask = n_contrib[i] > 0;
        const float opc = fmaxf(op, 1e-5f);
        const float scale = mask ? 1.f / opc : 0.f;
        const float dscale_dop = (mask && op >= 1e-5f) ? -1.f / (opc * opc) : 0.f;
        const float gD = w_smooth * dsm;                            // dL / d rendered depth
        dL_dfeature[3 * HW + i] += gD * scale;
        dL_dopacity[i] += gD * feature[3 * HW + i] * dscale_dop;
    }
}

// ---- stage 1: the per-Gaussian terms (render.py:181-197, :215-219) -----------------------------------------------------------
//   w_entropy     * sum_p w_p (-o log(o + 1e-10) - (1 - o) log(1 - o + 1e-10))          lambda_point_entropy
// + w_orientation * sum_p min(w_p, 1) max(n_p . d_p, 0),  d = F.normalize(xyz - campos)  lambda_orientation
// + w_scaling     * sum_p sum_axis |s - mean_axis s|                                      lambda_scaling
// (each weight carries the 1 / P of the reference's mean; w_p = the rasterizer's blend weights, a constant).  The gradients are
// ADDED to the activated-space rows r3dg_stage1_activate_backward consumes: dL_dopacity, dL_dscales, dL_dmeans3D (the
// orientation term through d) and columns 0..2 of dL_dfeatures [P,5] -- the feature row's normal columns ARE the activated
// normal, the only path to the raw normal's gradient.  One thread per Gaussian, one transposing wave reduction of the three
// sums, one add per wave and term.
__global__ void __launch_bounds__(256)
s1_gaussian_terms_kernel(int P, const float* __restrict__ weights, const float* __restrict__ opacity,
                         const float* __restrict__ normal, const float* __restrict__ scales, const float* __restrict__ xyz,
                         const float* __restrict__ campos, float w_entropy, float w_orientation, float w_scaling,
                         float* __restrict__ dL_dopacity, float* __restrict__ dL_dfeatures, float* __restrict__ dL_dscales,
                         float* __restrict__ dL_dmeans3D, float* __restrict__ sums3)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (i < P) {                     // (no early return: the reduction below exchanges between ALL lanes of the wave)
        const size_t i3 = 3 * (size_t)i;
        const float w = (w_entropy != 0.f || w_orientation != 0.f) ? weights[i] : 0.f;
        if (w_entropy != 0.f) {
            const float o = opacity[i];
            const float a = o + 1e-10f, b = 1.f - o + 1e-10f;
            const float la = logf(a), lb = logf(b);
            v[0] = w * (-o * la - (1.f - o) * lb);
            dL_dopacity[i] += w_entropy * w * (-la - o / a + lb + (1.f - o) / b);
        }
        if (w_orientation != 0.f) {
            const float n[3] = {normal[i3], normal[i3 + 1], normal[i3 + 2]};
            const float r[3] = {xyz[i3] - campos[0], xyz[i3 + 1] - campos[1], xyz[i3 + 2] - campos[2]};
            float d[3], inv;
            normalize3(r, 1e-12f, d, inv);
            const float nd = n[0] * d[0] + n[1] * d[1] + n[2] * d[2];
            const float wc = fminf(w, 1.f);
            v[1] = wc * fmaxf(nd, 0.f);
            if (nd >= 0.f) {             // (clamp_min passes the gradient at the bound itself, as torch does)
                const float g = w_orientation * wc;
                const float gd[3] = {g * n[0], g * n[1], g * n[2]};
                float gr[3];
                normalize3_backward(r, 1e-12f, gd, gr);
                float* gf = dL_dfeatures + 5 * (size_t)i;
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    gf[c] += g * d[c];
                    dL_dmeans3D[i3 + c] += gr[c];
                }
            }
        }
        if (w_scaling != 0.f) {
            const float s[3] = {scales[i3], scales[i3 + 1], scales[i3 + 2]};
            const float m = (s[0] + s[1] + s[2]) / 3.f;
            const float sg[3] = {signf_(s[0] - m), signf_(s[1] - m), signf_(s[2] - m)};
            const float sm = (sg[0] + sg[1] + sg[2]) / 3.f;
            v[2] = fabsf(s[0] - m) + fabsf(s[1] - m) + fabsf(s[2] - m);
#pragma unroll
            for (int c = 0; c < 3; c++) dL_dscales[i3 + c] += w_scaling * (sg[c] - sm);
        }
    }
    const float total = transpose_reduce<4, true>(v);            // every lane: the wave's total of ONE of the four channels
    const int lane = lane_id(), chan = transposed_channel<4>(lane);
    if (transposed_owner<4>(lane) && chan < 3) {
        const float wt = chan == 0 ? w_entropy : (chan == 1 ? w_orientation : w_scaling);
        if (wt != 0.f) atomicAdd(wave_sum_slot(sums3 + chan * R3DG_SUM_SLOTS), total);
    }
}

// ---- launchers ------------------------------------------------------------------------------------------------------
static int pixel_blocks(long long HW, int cap) { return (int)std::min((HW + 255) / 256, (long long)cap); }

static void launch_sup_count(hipStream_t s, int HW, const float* gt_depth, const float* image_mask, uint32_t* count)
{
    R3DG_HIP(hipMemsetAsync(count, 0, sizeof(uint32_t), s));
    sup_count_kernel<<<pixel_blocks(HW, 256), 256, 0, s>>>(HW, gt_depth, image_mask, count);
    check_launch(s, false, "sup_count_kernel");
}

static void launch_s2_supervision(hipStream_t s, int HW, const float* opacity, const float* feature, const int* n_contrib,
                                  const float* gt_depth, const float* mvs_normal, const float* image_mask,
                                  const uint32_t* count, float w_depth, float w_normal, int accumulate_normal,
                                  float* dL_dopacity, float* dL_dfeature, float* sums2)
{
    s2_supervision_kernel<<<pixel_blocks(HW, 768), 256, 0, s>>>(HW, opacity, feature, n_contrib, gt_depth, mvs_normal,
                                                                image_mask, count, w_depth, w_normal, accumulate_normal,
                                                                dL_dopacity, dL_dfeature, sums2);
    check_launch(s, false, "s2_supervision_kernel");
}

static void launch_s1_depth_smooth(hipStream_t s, int W, int H, const float* opacity, const float* feature,
                                   const int* n_contrib, const float* gt, float w_smooth, float* edge_g, float* dL_dopacity,
                                   float* dL_dfeature, float* sum_out)
{
    const int nb = pixel_blocks((long long)W * H, 2048);
    s1_depth_edge_kernel<<<nb, 256, 0, s>>>(W, H, feature, opacity, n_contrib, gt, edge_g, sum_out);
    check_launch(s, false, "s1_depth_edge_kernel");
    s1_depth_adjoint_kernel<<<nb, 256, 0, s>>>(W, H, feature, opacity, n_contrib, edge_g, w_smooth, dL_dopacity, dL_dfeature);
    check_launch(s, false, "s1_depth_adjoint_kernel");
}

static void launch_s1_gaussian_terms(hipStream_t s, int P, const float* weights, const float* opacity, const float* normal,
                                     const float* scales, const float* xyz, const float* campos, float w_entropy,
                                     float w_orientation, float w_scaling, float* dL_dopacity, float* dL_dfeatures,
                                     float* dL_dscales, float* dL_dmeans3D, float* sums3)
{
    s1_gaussian_terms_kernel<<<(P + 255) / 256, 256, 0, s>>>(P, weights, opacity, normal, scales, xyz, campos, w_entropy,
                                                            w_orientation, w_scaling, dL_dopacity, dL_dfeatures, dL_dscales,
                                                            dL_dmeans3D, sums3);
    check_launch(s, false, "s1_gaussian_terms_kernel");
}

}  // namespace r3dg

using namespace r3dg;

extern "C" {

int r3dg_supervision_count(void* stream_, int width, int height, const float* gt_depth, const float* image_mask,
                           uint32_t* count)
{
    if (width < 0 || height < 0) return invalid("supervision_count: bad image size");
    if ((long long)width * height > 0x7fffffffLL) return invalid("supervision_count: image too large");
    if (!count) return invalid("supervision_count: null buffer");
    if ((long long)width * height != 0 && !gt_depth) return invalid("supervision_count: null buffer");
    return guarded([&]() -> int {
        if ((long long)width * height == 0) {
            R3DG_HIP(hipMemsetAsync(count, 0, sizeof(uint32_t), (hipStream_t)stream_));
            return R3DG_OK;
        }
        StageTimer t((hipStream_t)stream_, ST_S2_LOSS);
        launch_sup_count((hipStream_t)stream_, width * height, gt_depth, image_mask, count);
        return R3DG_OK;
    });
}

int r3dg_stage2_supervision(void* stream_, int width, int height, const float* opacity, const float* feature,
                            const int32_t* n_contrib, const float* gt_depth, const float* mvs_normal,
                            const float* image_mask, const uint32_t* count, float w_depth, float w_normal_mvs,
                            int accumulate_normal, float* dL_dopacity, float* dL_dfeature, float* sums2)
{
    if (width < 0 || height < 0) return invalid("stage2_supervision: bad image size");
    if ((long long)width * height > 0x7fffffffLL) return invalid("stage2_supervision: image too large");
    if ((long long)width * height == 0 || (w_depth == 0.f && w_normal_mvs == 0.f)) return R3DG_OK;
    if (!opacity || !feature || !n_contrib || !gt_depth || !dL_dopacity || !dL_dfeature || !sums2)
        return invalid("stage2_supervision: null buffer");
    if (w_depth != 0.f && !count) return invalid("stage2_supervision: the depth term needs the count of r3dg_supervision_count");
    if (w_normal_mvs != 0.f && !mvs_normal) return invalid("stage2_supervision: the normal term needs the MVS normal map");
    return guarded([&]() -> int {
        StageTimer t((hipStream_t)stream_, ST_S2_LOSS);
        launch_s2_supervision((hipStream_t)stream_, width * height, opacity, feature, n_contrib, gt_depth, mvs_normal,
                              image_mask, count, w_depth, w_normal_mvs, accumulate_normal, dL_dopacity, dL_dfeature, sums2);
        return R3DG_OK;
    });
}

int r3dg_stage1_depth_smooth(void* stream_, int width, int height, const float* opacity, const float* feature,
                             const int32_t* n_contrib, const float* gt, float w_depth_smooth, float* edge_scratch,
                             float* dL_dopacity, float* dL_dfeature, float* sum)
{
    if (width < 0 || height < 0) return invalid("stage1_depth_smooth: bad image size");
    if ((long long)width * height == 0 || w_depth_smooth == 0.f) return R3DG_OK;
    if (!opacity || !feature || !n_contrib || !gt || !edge_scratch || !dL_dopacity || !dL_dfeature || !sum)
        return invalid("stage1_depth_smooth: null buffer");
    return guarded([&]() -> int {
        StageTimer t((hipStream_t)stream_, ST_S2_LOSS);
        launch_s1_depth_smooth((hipStream_t)stream_, width, height, opacity, feature, n_contrib, gt, w_depth_smooth,
                               edge_scratch, dL_dopacity, dL_dfeature, sum);
        return R3DG_OK;
    });
}

int r3dg_stage1_gaussian_terms(void* stream_, int P, const float* weights, const float* opacity, const float* normal,
                               const float* scales, const float* xyz, const float* campos, float w_point_entropy,
                               float w_orientation, float w_scaling, float* dL_dopacity, float* dL_dfeatures,
                               float* dL_dscales, float* dL_dmeans3D, float* sums3)
{
    if (P < 0) return invalid("stage1_gaussian_terms: bad P");
    if (P == 0 || (w_point_entropy == 0.f && w_orientation == 0.f && w_scaling == 0.f)) return R3DG_OK;
    if (!sums3) return invalid("stage1_gaussian_terms: null buffer");
    if ((w_point_entropy != 0.f || w_orientation != 0.f) && !weights)
        return invalid("stage1_gaussian_terms: the entropy and orientation terms need the blend weights");
    if (w_point_entropy != 0.f && (!opacity || !dL_dopacity)) return invalid("stage1_gaussian_terms: null opacity buffer");
    if (w_orientation != 0.f && (!normal || !xyz || !campos || !dL_dfeatures || !dL_dmeans3D))
        return invalid("stage1_gaussian_terms: null orientation buffer");
    if (w_scaling != 0.f && (!scales || !dL_dscales)) return invalid("stage1_gaussian_terms: null scale buffer");
    return guarded([&]() -> int {
        StageTimer t((hipStream_t)stream_, ST_S2_ACTIVATE_BWD);
        launch_s1_gaussian_terms((hipStream_t)stream_, P, weights, opacity, normal, scales, xyz, campos, w_point_entropy,
                                 w_orientation, w_scaling, dL_dopacity, dL_dfeatures, dL_dscales, dL_dmeans3D, sums3);
        return R3DG_OK;
    });
}

}  // extern "C"
