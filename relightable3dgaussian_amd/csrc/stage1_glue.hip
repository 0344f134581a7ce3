// Glue of the stage-1 (plain 3DGS + normals) training iteration: feature pack, the edge-aware normal smoothness pass, the
// image-space loss with its gradients, the activations' chain rule -- and their launchers.
#include "launchers.hpp"
#include "glue_math.hpp"
#include "r3dg_hip.h"

namespace r3dg {

// ---- stage 1 (plain 3DGS + normals, gaussian_renderer/render.py:15-130): S = 5 feature row [normal, depth, depth^2] ---
__global__ void __launch_bounds__(256)
s1_pack_features_kernel(int P, const float* __restrict__ xyz, const float* __restrict__ viewmatrix,
                        const float* __restrict__ normal, float* __restrict__ features)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const size_t i3 = 3 * (size_t)i;
    const float depth = xyz[i3] * viewmatrix[2] + xyz[i3 + 1] * viewmatrix[6] + xyz[i3 + 2] * viewmatrix[10] +
                        viewmatrix[14];
    float* f = features + 5 * (size_t)i;
    f[0] = normal[i3]; f[1] = normal[i3 + 1]; f[2] = normal[i3 + 2];
    f[3] = depth; f[4] = depth * depth;
}

// ---- stage-1 objective (gaussian_renderer/render.py:137-223 with the flags of script/run_nerf.sh:7-14) ---------------------
//   L = (1-l)*L1(image, gt) [+ l*(1-SSIM): csrc/ssim.hip, gradient arrives in extra_dimage]
//     + lambda_mask_entropy        * -mean(m log o + (1-m) log(1-o)),  o = clamp(opacity, 1e-6, 1-1e-6)      (:156-160)
//     + lambda_normal_render_depth * mse(normal*m, pseudo_normal*m)                                           (:162-167)
//     + lambda_normal_smooth       * first_order_edge_aware_loss(normal, gt)                                  (:169-173)
//     + lambda_depth_var(iter)     * mean sqrt(max(depth2 - depth^2, 1e-6))                                   (:199-205)
// with [normal, depth, depth2] = feature / max(opacity, 1e-5) * (n_contrib > 0) (:107-112) and m the view's object mask.
// first_order_edge_aware_loss (utils/loss_utils.py:104-105) = mean_{c,y,x} sum_{d in {x,y}} |G_d normal_c| exp(-|G_d gt_c|) with
// G = kornia.filters.spatial_gradient(order=1) of kornia 0.6.12 (readme.md:31-32; the package is not in this image, its
// published algorithm is restated): 3x3 Sobel cross-correlation, kernels [[-1,0,1],[-2,0,2],[-1,0,1]] and its transpose,
// normalised by the sum of absolute values (/8), replicate padding.
// Pass A (s1_edge_kernel): per pixel the six values sign(G_d normal_c) * exp(-|G_d gt_c|) and the loss sum.
// Pass B (inside s1_loss_kernel): the adjoint of the replicate-padded stencil, gathered (no atomics).
__device__ __forceinline__ float s1_rendered(const float* __restrict__ feature, const float* __restrict__ opacity,
                                             const int* __restrict__ n_contrib, size_t HW, int ch, size_t pix)
{
    const float opc = fmaxf(opacity[pix], 1e-5f);
    return n_contrib[pix] > 0 ? feature[(size_t)ch * HW + pix] / opc : 0.f;
}

__global__ void __launch_bounds__(256)
s1_edge_kernel(int W, int H, const float* __restrict__ feature, const float* __restrict__ opacity,
               const int* __restrict__ n_contrib, const float* __restrict__ gt, float* __restrict__ edge_g /*[3][2][HW]*/,
               float* __restrict__ sum_out)
{
    __shared__ float s_part[4];
    const size_t HW = (size_t)W * H;
    float acc = 0.f;
    for (size_t i = blockIdx.x * 256 + threadIdx.x; i < HW; i += (size_t)gridDim.x * 256) {
        const int y = (int)(i / W), x = (int)(i % W);
        const int ys[3] = {y > 0 ? y - 1 : 0, y, y < H - 1 ? y + 1 : H - 1};
        const int xs[3] = {x > 0 ? x - 1 : 0, x, x < W - 1 ? x + 1 : W - 1};
#pragma unroll
        for (int c = 0; c < 3; c++) {
            float n[3][3], g[3][3];
#pragma unroll
            for (int a = 0; a < 3; a++)
#pragma unroll
                for (int b = 0; b < 3; b++) {
                    const size_t q = (size_t)ys[a] * W + xs[b];
                    n[a][b] = s1_rendered(feature, opacity, n_contrib, HW, c, q);
                    g[a][b] = gt[(size_t)c * HW + q];
                }
            const float nx = ((n[0][2] - n[0][0]) + 2.f * (n[1][2] - n[1][0]) + (n[2][2] - n[2][0])) * 0.125f;
            const float ny = ((n[2][0] - n[0][0]) + 2.f * (n[2][1] - n[0][1]) + (n[2][2] - n[0][2])) * 0.125f;
            const float gx = ((g[0][2] - g[0][0]) + 2.f * (g[1][2] - g[1][0]) + (g[2][2] - g[2][0])) * 0.125f;
            const float gy = ((g[2][0] - g[0][0]) + 2.f * (g[2][1] - g[0][1]) + (g[2][2] - g[0][2])) * 0.125f;
            const float ex = __expf(-fabsf(gx)), ey = __expf(-fabsf(gy));
            acc += fabsf(nx) * ex + fabsf(ny) * ey;
            edge_g[(size_t)(2 * c) * HW + i] = signf_(nx) * ex;
            edge_g[(size_t)(2 * c + 1) * HW + i] = signf_(ny) * ey;
        }
    }
    const float t = block_sum_256(acc, s_part);
    if (threadIdx.x == 0) atomicAdd(sum_slot(sum_out), t);
}

// sums[0] += sum|image-gt|, [1] += sum m^2 (normal - pseudo)^2, [2] += sum -(m log o + (1-m) log(1-o)), [5] += sum sqrt(var)
// (sums[3] is the SSIM slot, sums[4] the edge-aware sum of s1_edge_kernel); image_mask == nullptr means all ones.
__global__ void __launch_bounds__(256)
s1_loss_kernel(int W, int H, const float* __restrict__ image, const float* __restrict__ opacity,
               const float* __restrict__ feature, const float* __restrict__ pseudo_normal,
               const int* __restrict__ n_contrib, const float* __restrict__ gt, const float* __restrict__ image_mask,
               float w_l1, float w_entropy, float w_normal, float w_smooth, float w_var,
               const float* __restrict__ extra_dimage, const float* __restrict__ edge_g, float* __restrict__ dL_dimage,
               float* __restrict__ dL_dopacity, float* __restrict__ dL_dfeature, float* __restrict__ sums)
{
    __shared__ float s_part[4];
    const size_t HW = (size_t)W * H;
    float s_l1 = 0.f, s_n = 0.f, s_e = 0.f, s_v = 0.f;
    for (size_t i = blockIdx.x * 256 + threadIdx.x; i < HW; i += (size_t)gridDim.x * 256) {
        const float op = opacity[i];
        const bool mask = n_contrib[i] > 0;
        const float opc = fmaxf(op, 1e-5f);
        const float scale = mask ? 1.f / opc : 0.f;
        const float dscale_dop = (mask && op >= 1e-5f) ? -1.f / (opc * opc) : 0.f;
        const float m = image_mask ? image_mask[i] : 1.f;
        // mask entropy
        const float o = fminf(fmaxf(op, 1e-6f), 1.f - 1e-6f);
        s_e -= m * __logf(o) + (1.f - m) * __logf(1.f - o);
        float g_op = (op >= 1e-6f && op <= 1.f - 1e-6f) ? -w_entropy * (m / o - (1.f - m) / (1.f - o)) : 0.f;
        // adjoint of the edge-aware stencil: weights of the (up to) 9 neighbours q whose stencil reads this pixel
        float dsm[3] = {0.f, 0.f, 0.f};
        if (edge_g != nullptr && w_smooth != 0.f) {
            const int y = (int)(i / W), x = (int)(i % W);
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
#pragma unroll
                    for (int c = 0; c < 3; c++)
                        dsm[c] += wx * edge_g[(size_t)(2 * c) * HW + q] + wy * edge_g[(size_t)(2 * c + 1) * HW + q];
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float d0 = image[(size_t)c * HW + i] - gt[(size_t)c * HW + i];
            s_l1 += fabsf(d0);
            dL_dimage[(size_t)c * HW + i] = w_l1 * signf_(d0) + (extra_dimage ? extra_dimage[(size_t)c * HW + i] : 0.f);
            const float Fn = feature[(size_t)c * HW + i];
            const float dn = (Fn * scale - pseudo_normal[(size_t)c * HW + i]) * m;
            s_n += dn * dn;
            const float gn = 2.f * w_normal * dn * m + w_smooth * dsm[c];       // dL / d rendered_normal_c
            dL_dfeature[(size_t)c * HW + i] = gn * scale;
            g_op += gn * Fn * dscale_dop;
        }
        // depth variance
        const float F3 = feature[(size_t)3 * HW + i], F4 = feature[(size_t)4 * HW + i];
        const float D = F3 * scale, D2 = F4 * scale;
        const float var = D2 - D * D;
        const float sd = sqrtf(fmaxf(var, 1e-6f));
        s_v += sd;
        const float dvar = var >= 1e-6f ? w_var * 0.5f / sd : 0.f;
        const float gD = -2.f * D * dvar;
        dL_dfeature[(size_t)3 * HW + i] = gD * scale;
        dL_dfeature[(size_t)4 * HW + i] = dvar * scale;
        g_op += (gD * F3 + dvar * F4) * dscale_dop;
        dL_dopacity[i] = g_op;
    }
    const float t0 = block_sum_256(s_l1, s_part);
    __syncthreads();
    const float t1 = block_sum_256(s_n, s_part);
    __syncthreads();
    const float t2 = block_sum_256(s_e, s_part);
    __syncthreads();
    const float t3 = block_sum_256(s_v, s_part);
    if (threadIdx.x == 0) {
        atomicAdd(sum_slot(sums + 0 * R3DG_SUM_SLOTS), t0);
        atomicAdd(sum_slot(sums + 1 * R3DG_SUM_SLOTS), t1);
        atomicAdd(sum_slot(sums + 2 * R3DG_SUM_SLOTS), t2);
        atomicAdd(sum_slot(sums + 5 * R3DG_SUM_SLOTS), t3);
    }
}

__global__ void __launch_bounds__(256)
s1_activate_backward_kernel(int P, const float* __restrict__ xyz, const float* __restrict__ scaling_raw,
                            const float* __restrict__ rotation_raw, const float* __restrict__ opacity_raw,
                            const float* __restrict__ normal_raw, const float* __restrict__ viewmatrix,
                            const float* __restrict__ dL_dfeatures, const float* __restrict__ dL_dscales,
                            const float* __restrict__ dL_drot, const float* __restrict__ dL_dopacity,
                            const float* __restrict__ dL_dmeans3D, float* __restrict__ g_xyz,
                            float* __restrict__ g_scaling, float* __restrict__ g_rotation,
                            float* __restrict__ g_opacity, float* __restrict__ g_normal)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const size_t i3 = 3 * (size_t)i, i4 = 4 * (size_t)i;
    const float* gf = dL_dfeatures + 5 * (size_t)i;
#pragma unroll
    for (int c = 0; c < 3; c++) g_scaling[i3 + c] = dL_dscales[i3 + c] * __expf(scaling_raw[i3 + c]);
    {
        const float q[4] = {rotation_raw[i4], rotation_raw[i4 + 1], rotation_raw[i4 + 2], rotation_raw[i4 + 3]};
        const float g[4] = {dL_drot[i4], dL_drot[i4 + 1], dL_drot[i4 + 2], dL_drot[i4 + 3]};
        const float n = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        if (n > 1e-12f) {
            // u = q / n by DIVISION: a quaternion along one axis gives u = +-1 exactly, so its radial gradient g - u (u.g) is exactly
            // 0, as in exact arithmetic (q * (1/n) * (1/n) left a rounding residue of 1e-7 |g| there: tests/test_glue_kernels_gpu.py)
            const float inv = 1.f / n;
            const float u[4] = {q[0] / n, q[1] / n, q[2] / n, q[3] / n};
            const float d = u[0] * g[0] + u[1] * g[1] + u[2] * g[2] + u[3] * g[3];
#pragma unroll
            for (int c = 0; c < 4; c++) g_rotation[i4 + c] = (g[c] - u[c] * d) * inv;
        } else {
#pragma unroll
            for (int c = 0; c < 4; c++) g_rotation[i4 + c] = g[c] * 1e12f;
        }
    }
    {
        const float sg = sigmoidf_(opacity_raw[i]);
        g_opacity[i] = dL_dopacity[i] * sg * (1.f - sg);
    }
    {
        const float v[3] = {normal_raw[i3], normal_raw[i3 + 1], normal_raw[i3 + 2]};
        const float g[3] = {gf[0], gf[1], gf[2]};
        float o[3];
        normalize3_backward(v, 1e-3f, g, o);
        g_normal[i3] = o[0]; g_normal[i3 + 1] = o[1]; g_normal[i3 + 2] = o[2];
    }
    {
        const float depth = xyz[i3] * viewmatrix[2] + xyz[i3 + 1] * viewmatrix[6] + xyz[i3 + 2] * viewmatrix[10] +
                            viewmatrix[14];
        const float gd = gf[3] + 2.f * depth * gf[4];
        g_xyz[i3] = dL_dmeans3D[i3] + gd * viewmatrix[2];
        g_xyz[i3 + 1] = dL_dmeans3D[i3 + 1] + gd * viewmatrix[6];
        g_xyz[i3 + 2] = dL_dmeans3D[i3 + 2] + gd * viewmatrix[10];
    }
}

// ---- launchers ------------------------------------------------------------------------------------------------------
void launch_s1_pack(hipStream_t s, int P, const float* xyz, const float* viewmatrix, const float* normal, float* features)
{
    s1_pack_features_kernel<<<(P + 255) / 256, 256, 0, s>>>(P, xyz, viewmatrix, normal, features);
    check_launch(s, false, "s1_pack_features_kernel");
}

void launch_s1_edge(hipStream_t s, int W, int H, const float* feature, const float* opacity, const int* n_contrib,
                    const float* gt, float* edge_g, float* sum_out)
{
    const long long HW = (long long)W * H;
    s1_edge_kernel<<<(int)min((HW + 255) / 256, (long long)4096), 256, 0, s>>>(W, H, feature, opacity, n_contrib, gt, edge_g,
                                                                           sum_out);
    check_launch(s, false, "s1_edge_kernel");
}

void launch_s1_loss(hipStream_t s, int W, int H, const float* image, const float* opacity, const float* feature,
                    const float* pseudo_normal, const int* n_contrib, const float* gt, const float* image_mask, float w_l1,
                    float w_entropy, float w_normal, float w_smooth, float w_var, const float* extra_dimage,
                    const float* edge_g, float* dL_dimage, float* dL_dopacity, float* dL_dfeature, float* sums)
{
    const long long HW = (long long)W * H;
    s1_loss_kernel<<<(int)min((HW + 255) / 256, (long long)2048), 256, 0, s>>>(
        W, H, image, opacity, feature, pseudo_normal, n_contrib, gt, image_mask, w_l1, w_entropy, w_normal, w_smooth, w_var,
        extra_dimage, edge_g, dL_dimage, dL_dopacity, dL_dfeature, sums);
    check_launch(s, false, "s1_loss_kernel");
}

void launch_s1_activate_backward(hipStream_t s, int P, const float* xyz, const float* scaling_raw,
                                 const float* rotation_raw, const float* opacity_raw, const float* normal_raw,
                                 const float* viewmatrix, const float* dL_dfeatures, const float* dL_dscales,
                                 const float* dL_drot, const float* dL_dopacity, const float* dL_dmeans3D, float* g_xyz,
                                 float* g_scaling, float* g_rotation, float* g_opacity, float* g_normal)
{
    s1_activate_backward_kernel<<<(P + 255) / 256, 256, 0, s>>>(P, xyz, scaling_raw, rotation_raw, opacity_raw,
                                                              normal_raw, viewmatrix, dL_dfeatures, dL_dscales, dL_drot,
                                                              dL_dopacity, dL_dmeans3D, g_xyz, g_scaling, g_rotation,
                                                              g_opacity, g_normal);
    check_launch(s, false, "s1_activate_backward_kernel");
}

}  // namespace r3dg
