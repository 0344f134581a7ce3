// Fused glue of the stage-2 (neilf) training iteration for gfx950 -- SURVEY.md 8(f) rows n1/n2: the elementwise code the
// reference runs as ~250 tiny PyTorch kernels per iteration either side of the hot ops, restated as a few HBM-bound
// kernels (every one a single streaming pass, one thread per Gaussian / pixel / parameter):
//   s2_activate_kernel            GaussianModel.get_* activations (scene/gaussian_model.py:183-232) + view directions
//                                 (gaussian_renderer/neilf.py:74-76)
//   s2_pack_features_kernel       the S=16 feature row (neilf.py:115-122) + the light-smoothness L1 (neilf.py:286-292)
//   s2_unpack_kernel              its backward: rasterizer feature gradients -> shading-op upstream gradients
//   s2_activate_backward_kernel   chain rule of every activation, summed with the rasterizer / shading gradients,
//                                 straight into the raw-parameter gradient buffers
//   s2_loss_kernel                image-space loss terms AND their gradients in one pass (neilf.py:212-318: L1 on the
//                                 SH image, L1 on the sRGB-mapped PBR image, normal-vs-pseudo-normal MSE)
// (the stage-1 kernels are stage1_glue.hip, the smoothness terms smooth.hip, the multi-group Adam step adam.hip)
// Parity target: the plain-PyTorch restatement in relightable3dgaussian_amd/train_step.py (Stage2Step), fp32 tolerance.
#include "launchers.hpp"
#include "glue_math.hpp"
#include "stage2_loss_math.hpp"
#include "pseudo_normal.hpp"
#include "r3dg_hip.h"

namespace r3dg {

// Side jobs of the activation kernel: microseconds of work that would otherwise be launches of their own on the iteration's critical
// stream (5-20 us each there).  They ride as EXTRA WORKGROUPS behind the nb_main workgroups of the Gaussians:
//   * env[i] = softplus(env_raw[i]) for the n_env floats of the environment texture (DirectLightMap.get_env,
//     scene/direct_light_map.py:18-23; torch's softplus: beta 1, threshold 20);
//   * zero[0..n_zero) = 0 (the iteration's loss sums).
struct ActivateSide {
    int nb_main;
    int n_env;
    const float* env_raw;
    float* env;
    float* zero;
    int n_zero;
};

__global__ void __launch_bounds__(256)
s2_activate_kernel(int P, const float* __restrict__ xyz, const float* __restrict__ scaling_raw,
                   const float* __restrict__ rotation_raw, const float* __restrict__ opacity_raw,
                   const float* __restrict__ normal_raw, const float* __restrict__ base_raw,
                   const float* __restrict__ rough_raw, const float* __restrict__ campos,
                   float* __restrict__ scales, float* __restrict__ rot, float* __restrict__ opacity,
                   float* __restrict__ normal, float* __restrict__ base_color, float* __restrict__ roughness,
                   float* __restrict__ viewdirs, const float* __restrict__ viewmatrix, float* __restrict__ features,
                   ActivateSide side)
{
    if ((int)blockIdx.x >= side.nb_main) {
        const int nb_side = (int)gridDim.x - side.nb_main;
        for (int k = ((int)blockIdx.x - side.nb_main) * 256 + (int)threadIdx.x; k < side.n_env; k += nb_side * 256) {
            const float r = side.env_raw[k];
            side.env[k] = r > 20.f ? r : log1pf(expf(r));
        }
        for (int k = ((int)blockIdx.x - side.nb_main) * 256 + (int)threadIdx.x; k < side.n_zero; k += nb_side * 256)
            side.zero[k] = 0.f;
        return;
    }
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const size_t i3 = 3 * (size_t)i, i4 = 4 * (size_t)i;
#pragma unroll
    for (int c = 0; c < 3; c++) scales[i3 + c] = __expf(scaling_raw[i3 + c]);
    {
        const float q[4] = {rotation_raw[i4], rotation_raw[i4 + 1], rotation_raw[i4 + 2], rotation_raw[i4 + 3]};
        const float inv = 1.f / fmaxf(sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]), 1e-12f);
#pragma unroll
        for (int c = 0; c < 4; c++) rot[i4 + c] = q[c] * inv;
    }
    opacity[i] = sigmoidf_(opacity_raw[i]);
    float inv, nrm[3];
    {
        const float v[3] = {normal_raw[i3], normal_raw[i3 + 1], normal_raw[i3 + 2]};
        normalize3(v, 1e-3f, nrm, inv);
        normal[i3] = nrm[0]; normal[i3 + 1] = nrm[1]; normal[i3 + 2] = nrm[2];
    }
    if (base_raw != nullptr) {
        float bc[3];
#pragma unroll
        for (int c = 0; c < 3; c++) base_color[i3 + c] = bc[c] = 0.03f + 0.77f * sigmoidf_(base_raw[i3 + c]);
        const float rg = 0.09f + 0.9f * sigmoidf_(rough_raw[i]);
        roughness[i] = rg;
        const float p[3] = {xyz[i3], xyz[i3 + 1], xyz[i3 + 2]};
        const float d[3] = {campos[0] - p[0], campos[1] - p[1], campos[2] - p[2]};
        float o[3];
        normalize3(d, 1e-12f, o, inv);
        viewdirs[i3] = o[0]; viewdirs[i3 + 1] = o[1]; viewdirs[i3 + 2] = o[2];
        if (features != nullptr) {
            // the columns of the S=16 feature row that do not wait for the shading integral (s2_pack_features_kernel's, value for
            // value): depth, depth^2 | . . . | normal | base colour | roughness | . . . .   The shading kernels fill in the rest
            const float depth = p[0] * viewmatrix[2] + p[1] * viewmatrix[6] + p[2] * viewmatrix[10] + viewmatrix[14];
            float* f = features + 16 * (size_t)i;
            *reinterpret_cast<float2*>(f) = make_float2(depth, depth * depth);
            f[5] = nrm[0]; f[6] = nrm[1]; f[7] = nrm[2];
            *reinterpret_cast<float4*>(f + 8) = make_float4(bc[0], bc[1], bc[2], rg);
        }
    }
}

// features[P,16] = depth, depth^2, pbr(3), normal(3), base_color(3), roughness, diffuse_light(3), mean visibility
__global__ void __launch_bounds__(256)
s2_pack_features_kernel(int P, const float* __restrict__ xyz, const float* __restrict__ viewmatrix,
                        const float* __restrict__ normal, const float* __restrict__ base_color,
                        const float* __restrict__ roughness, const float* __restrict__ shade_out,
                        float* __restrict__ features, float* __restrict__ light_l1_sum)
{
    __shared__ float s_part[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    float l1 = 0.f;
    if (i < P) {
        const size_t i3 = 3 * (size_t)i;
        const float depth = xyz[i3] * viewmatrix[2] + xyz[i3 + 1] * viewmatrix[6] + xyz[i3 + 2] * viewmatrix[10] +
                            viewmatrix[14];
        const float* so = shade_out + 19 * (size_t)i;
        const float dl[3] = {so[3], so[4], so[5]};
        float4* f = reinterpret_cast<float4*>(features + 16 * (size_t)i);
        f[0] = make_float4(depth, depth * depth, so[0], so[1]);
        f[1] = make_float4(so[2], normal[i3], normal[i3 + 1], normal[i3 + 2]);
        f[2] = make_float4(base_color[i3], base_color[i3 + 1], base_color[i3 + 2], roughness[i]);
        f[3] = make_float4(dl[0], dl[1], dl[2], so[18]);
        const float m = (dl[0] + dl[1] + dl[2]) / 3.f;
        l1 = fabsf(dl[0] - m) + fabsf(dl[1] - m) + fabsf(dl[2] - m);
    }
    const float tot = block_sum_256(l1, s_part);
    if (threadIdx.x == 0 && light_l1_sum != nullptr) atomicAdd(sum_slot(light_l1_sum), tot);
}


// dL_dpbr / dL_ddiffuse_light for the shading op: the rasterizer's feature gradients (cols 2-4 / 12-14) plus the gradient of
// light_weight * sum_c |dl_c - mean(dl)|
// block_absmax (may be NULL): [gridDim.x] floats, max |upstream gradient| of the block's rows, +inf if any is not finite --
// the scale of the shading backward's fixed-point texture accumulation (shading.hip), so that op needs no reduction pass
// `rec` (UnpackRecords; rows == NULL: the [P,16] array dL_dfeatures is the source): the six columns straight from the tile backward's
// gradient record rows -- a run-time choice of where the six loads go, uniform over the grid; everything behind them is one stream
struct UnpackRecords {
    const float* rows;
    int nvp;
    int ch[6];          // record channel of columns 2, 3, 4, 12, 13, 14; -1: the column was not carried and reads as +0.f
};

__global__ void __launch_bounds__(256)
s2_unpack_kernel(int P, const float* __restrict__ dL_dfeatures, const float* __restrict__ shade_out, float light_weight,
                 float* __restrict__ dL_dpbr, float* __restrict__ dL_ddiffuse, float* __restrict__ block_absmax,
                 float* __restrict__ light_l1_sum, UnpackRecords rec)
{
    __shared__ float s_m[4];
    __shared__ float s_l1[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    float m = 0.f, l1 = 0.f;
    bool bad = false;
    if (i < P) {
        float4 g0, g1, g3;
        if (rec.rows == nullptr) {
            const float4* g = reinterpret_cast<const float4*>(dL_dfeatures + 16 * (size_t)i);
            g0 = g[0]; g1 = g[1]; g3 = g[3];
        } else {
            const float* r = rec.rows + (size_t)i * rec.nvp;
            g0.x = g0.y = g1.y = g1.z = g1.w = g3.w = 0.f;        // (not read)
            g0.z = rec.ch[0] < 0 ? 0.f : r[rec.ch[0]];
            g0.w = rec.ch[1] < 0 ? 0.f : r[rec.ch[1]];
            g1.x = rec.ch[2] < 0 ? 0.f : r[rec.ch[2]];
            g3.x = rec.ch[3] < 0 ? 0.f : r[rec.ch[3]];
            g3.y = rec.ch[4] < 0 ? 0.f : r[rec.ch[4]];
            g3.z = rec.ch[5] < 0 ? 0.f : r[rec.ch[5]];
        }
        const size_t i3 = 3 * (size_t)i;
        dL_dpbr[i3] = g0.z; dL_dpbr[i3 + 1] = g0.w; dL_dpbr[i3 + 2] = g1.x;
        const float* so = shade_out + 19 * (size_t)i;
        const float dl[3] = {so[3], so[4], so[5]};
        const float mean = (dl[0] + dl[1] + dl[2]) / 3.f;
        const float s[3] = {signf_(dl[0] - mean), signf_(dl[1] - mean), signf_(dl[2] - mean)};
        const float sm = (s[0] + s[1] + s[2]) / 3.f;
        l1 = fabsf(dl[0] - mean) + fabsf(dl[1] - mean) + fabsf(dl[2] - mean);
        const float d0 = g3.x + light_weight * (s[0] - sm), d1 = g3.y + light_weight * (s[1] - sm),
                    d2 = g3.z + light_weight * (s[2] - sm);
        dL_ddiffuse[i3] = d0; dL_ddiffuse[i3 + 1] = d1; dL_ddiffuse[i3 + 2] = d2;
        const float v[6] = {fabsf(g0.z), fabsf(g0.w), fabsf(g1.x), fabsf(d0), fabsf(d1), fabsf(d2)};
#pragma unroll
        for (int c = 0; c < 6; c++) {
            bad = bad || !(v[c] <= 3.0e38f);
            m = fmaxf(m, v[c]);
        }
    }
    if (light_l1_sum != nullptr) {      // the term's VALUE, when no s2_pack_features_kernel ran in front (it adds the same sum)
        const float tot = block_sum_256(l1, s_l1);
        if (threadIdx.x == 0) atomicAdd(sum_slot(light_l1_sum), tot);
    }
    if (block_absmax == nullptr) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if (__ballot(bad) != 0ull) m = __uint_as_float(0x7f800000u);
    if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) block_absmax[blockIdx.x] = fmaxf(fmaxf(s_m[0], s_m[1]), fmaxf(s_m[2], s_m[3]));
}

// DirectLightMap: env = softplus(raw) (direct_light_map.py:18-23) and the total-variation smoothness term on it
// (neilf.py:294-300): g_raw = (dL_denv + w_tv * dTV/denv) * softplus'(raw); *tv_sum += TV(env) (unweighted).
// env layout [He,We,3]; TV = mean (d/dh)^2 + mean (d/dw)^2 over the 3 x He x We image (the reference's tv_loss,
// utils/loss_utils.py:113-117, pinned by tests/golden/ssim_reference.npz).
// One workgroup of 256 threads per 256 texture floats (`block` = its index); a launch of its own (s2_env_backward_kernel) or the
// extra workgroups of s2_activate_backward_kernel (the texture is 1536 floats: six workgroups that took 11-20 us as a launch on
// the critical stream between the activation chain rule and Adam).
struct EnvBackward {
    int He, We;
    const float* raw;
    const float* env;
    float* dL_denv;
    float w_tv;
    float* g_raw;
    float* tv_sum;
    int consume;
};

__device__ __forceinline__ void env_backward_block(int block, const EnvBackward& a)
{
    __shared__ float s_part[4];
    const int He = a.He, We = a.We;
    const int n = He * We * 3;
    const int i = block * 256 + threadIdx.x;
    float tv = 0.f;
    if (i < n) {
        const int w = (i / 3) % We, h = i / (3 * We);
        const float inv_v = He > 1 ? 1.f / (3.f * (He - 1) * We) : 0.f, inv_h = We > 1 ? 1.f / (3.f * He * (We - 1)) : 0.f;
        const float x = a.env[i];
        float g = 0.f;
        // tv_loss (utils/loss_utils.py:113-117): mean SQUARED forward difference along h plus the same along w
        if (h > 0) g += inv_v * 2.f * (x - a.env[i - 3 * We]);
        if (h < He - 1) { const float d = a.env[i + 3 * We] - x; g -= inv_v * 2.f * d; tv += inv_v * d * d; }
        if (w > 0) g += inv_h * 2.f * (x - a.env[i - 3]);
        if (w < We - 1) { const float d = a.env[i + 3] - x; g -= inv_h * 2.f * d; tv += inv_h * d * d; }
        const float r = a.raw[i];
        const float dsoft = r > 20.f ? 1.f : sigmoidf_(r);
        a.g_raw[i] = (a.dL_denv[i] + a.w_tv * g) * dsoft;
        if (a.consume) a.dL_denv[i] = 0.f;        // the accumulator is handed back zeroed for the next shading backward
    }
    const float tot = block_sum_256(tv, s_part);
    if (threadIdx.x == 0 && a.tv_sum != nullptr) atomicAdd(sum_slot(a.tv_sum), tot);
}

__global__ void __launch_bounds__(256)
s2_env_backward_kernel(EnvBackward a)
{
    env_backward_block((int)blockIdx.x, a);
}

// `rec` (ActivateRecords; rows == NULL: the arrays dL_dfeatures [P,16] and dL_dopacity are the source): the opacity gradient and the
// nine feature columns this kernel reads, straight from the tile backward's 16-float gradient record rows.  A run-time choice of
// where the loads go, uniform over the grid.  This kernel is the LAST reader of the rows (the unpack kernel ran in front of it on
// the same stream, the per-Gaussian geometry backward has been joined): behind its loads each thread writes its row back as
// zeros, which is the state the tile backward expects to find.
struct ActivateRecords {
    float* rows;
    int opacity;
    int col[12];        // record channel of feature column c (0, 1, 5..11 are read); -1: not carried, reads as +0.f
};

__global__ void __launch_bounds__(256)
s2_activate_backward_kernel(int P, const float* __restrict__ xyz, const float* __restrict__ scaling_raw,
                            const float* __restrict__ rotation_raw, const float* __restrict__ opacity_raw,
                            const float* __restrict__ normal_raw, const float* __restrict__ base_raw,
                            const float* __restrict__ rough_raw, const float* __restrict__ viewmatrix,
                            const float* __restrict__ campos, const float* __restrict__ dL_dfeatures,
                            const float* __restrict__ dL_dbase_shade, const float* __restrict__ dL_drough_shade,
                            const float* __restrict__ dL_dviewdirs, const float* __restrict__ dL_dscales,
                            const float* __restrict__ dL_drot, const float* __restrict__ dL_dopacity,
                            const float* __restrict__ dL_dmeans3D, float* __restrict__ g_xyz,
                            float* __restrict__ g_scaling, float* __restrict__ g_rotation,
                            float* __restrict__ g_opacity, float* __restrict__ g_normal, float* __restrict__ g_base,
                            float* __restrict__ g_rough, int nb_main, EnvBackward env_job, ActivateRecords rec)
{
    if ((int)blockIdx.x >= nb_main) {             // side job: the environment texture's chain rule (EnvBackward)
        env_backward_block((int)blockIdx.x - nb_main, env_job);
        return;
    }
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const size_t i3 = 3 * (size_t)i, i4 = 4 * (size_t)i;
    float4 f0, f1, f2;
    float g_op_rec = 0.f;
    if (rec.rows == nullptr) {
        const float4* gf = reinterpret_cast<const float4*>(dL_dfeatures + 16 * (size_t)i);
        f0 = gf[0]; f1 = gf[1]; f2 = gf[2];
    } else {
        float* r = rec.rows + 16 * (size_t)i;
        auto column = [&](int c) { return rec.col[c] < 0 ? 0.f : r[rec.col[c]]; };
        f0.x = column(0); f0.y = column(1);
        f0.z = f0.w = f1.x = 0.f;                                  // (not read)
        f1.y = column(5); f1.z = column(6); f1.w = column(7);
        f2.x = column(8); f2.y = column(9); f2.z = column(10); f2.w = column(11);
        g_op_rec = r[rec.opacity];
        float4* z = reinterpret_cast<float4*>(r);
        z[0] = z[1] = z[2] = z[3] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // base_color = 0.03 + 0.77 sigmoid(raw), roughness = 0.09 + 0.9 sigmoid(raw): feature row + shading op
    {
        const float gfeat[3] = {f2.x, f2.y, f2.z};
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float s = sigmoidf_(base_raw[i3 + c]);
            g_base[i3 + c] = (gfeat[c] + dL_dbase_shade[i3 + c]) * 0.77f * s * (1.f - s);
        }
        const float s = sigmoidf_(rough_raw[i]);
        g_rough[i] = (f2.w + dL_drough_shade[i]) * 0.9f * s * (1.f - s);
    }
    // frozen geometry (g_xyz == NULL, wave-uniform): base colour and roughness are the only per-Gaussian groups that train
    if (g_xyz == nullptr) return;

    // scales = exp(raw)
#pragma unroll
    for (int c = 0; c < 3; c++) g_scaling[i3 + c] = dL_dscales[i3 + c] * __expf(scaling_raw[i3 + c]);
    // rotation = q / max(|q|, 1e-12)
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
    // opacity = sigmoid(raw)
    {
        const float s = sigmoidf_(opacity_raw[i]);
        g_opacity[i] = (rec.rows == nullptr ? dL_dopacity[i] : g_op_rec) * s * (1.f - s);
    }
    // normal = raw / max(|raw|, 1e-3); only the feature row carries its gradient (the shading op sees normal.detach())
    {
        const float v[3] = {normal_raw[i3], normal_raw[i3 + 1], normal_raw[i3 + 2]};
        const float g[3] = {f1.y, f1.z, f1.w};
        float o[3];
        normalize3_backward(v, 1e-3f, g, o);
        g_normal[i3] = o[0]; g_normal[i3 + 1] = o[1]; g_normal[i3 + 2] = o[2];
    }
    // xyz: rasterizer + depth / depth^2 feature columns + view direction
    {
        const float p[3] = {xyz[i3], xyz[i3 + 1], xyz[i3 + 2]};
        const float depth = p[0] * viewmatrix[2] + p[1] * viewmatrix[6] + p[2] * viewmatrix[10] + viewmatrix[14];
        const float gd = f0.x + 2.f * depth * f0.y;
        const float d[3] = {campos[0] - p[0], campos[1] - p[1], campos[2] - p[2]};
        const float gv[3] = {dL_dviewdirs[i3], dL_dviewdirs[i3 + 1], dL_dviewdirs[i3 + 2]};
        float gdd[3];
        normalize3_backward(d, 1e-12f, gv, gdd);
        g_xyz[i3] = dL_dmeans3D[i3] + gd * viewmatrix[2] - gdd[0];
        g_xyz[i3 + 1] = dL_dmeans3D[i3 + 1] + gd * viewmatrix[6] - gdd[1];
        g_xyz[i3 + 2] = dL_dmeans3D[i3 + 2] + gd * viewmatrix[10] - gdd[2];
    }
}

// sRGB-mapped PBR image (neilf.py:190-200: feat = feature / max(opacity,1e-5) * mask, pbr_img = feat[2:5]*op + (1-op)*bg,
// linear -> sRGB), materialised for the SSIM term
__global__ void __launch_bounds__(256)
s2_pbr_srgb_kernel(int HW, const float* __restrict__ opacity, const float* __restrict__ feature,
                   const int* __restrict__ n_contrib, const float* __restrict__ bg, float* __restrict__ srgb)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= HW) return;
    const float op = opacity[i];
    const float scale = s2_divide_scale(op, n_contrib[i]);
#pragma unroll
    for (int c = 0; c < 3; c++)
        srgb[(size_t)c * HW + i] = s2_pbr_srgb_pixel(feature[(size_t)(2 + c) * HW + i], scale, op, bg[c]);
}

// pseudo_normal_kernel (the rasterizer forward's K9 + K10, pseudo_normal.hpp) and s2_pbr_srgb_kernel as ONE launch, pixel by pixel:
// the two are independent per-pixel passes over the tile forward's outputs that followed each other on the critical stream (10 + 7
// us at 800x800).  Same values as the two kernels (same device functions).
__global__ void __launch_bounds__(256)
s2_normals_srgb_kernel(int W, int H, float focal_x, float focal_y, float cx, float cy, const float* __restrict__ vm,
                       const float* __restrict__ opacity, const float* __restrict__ depths, float* __restrict__ normals,
                       float* __restrict__ surface_xyz, const float* __restrict__ feature, const int* __restrict__ n_contrib,
                       const float* __restrict__ bg, float* __restrict__ srgb)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const int HW = W * H, i = y * W + x;
    {
        const float op = opacity[i];
        const float scale = s2_divide_scale(op, n_contrib[i]);
#pragma unroll
        for (int c = 0; c < 3; c++)
            srgb[(size_t)c * HW + i] = s2_pbr_srgb_pixel(feature[(size_t)(2 + c) * HW + i], scale, op, bg[c]);
    }
    pseudo_normal_pixel(x, y, W, H, focal_x, focal_y, cx, cy, vm, opacity, depths, normals, surface_xyz);
}

// Image-space loss + gradient in one pass.  sums[0..2] += sum|image-gt|, sum|srgb(pbr)-gt|, sum (n_render - n_pseudo)^2
// (unweighted); gradients carry the weights w_* (already divided by the element counts).
// SPARSE: only the feature-gradient maps that carry a loss term are written (2-4; 5-7 when w_normal != 0) -- for callers
// whose rasterizer backward reads exactly those (active_features); with w_normal == 0 the normal maps are not even read.
template <bool SPARSE>
__global__ void __launch_bounds__(256)
s2_loss_kernel(int HW, const float* __restrict__ image, const float* __restrict__ opacity,
               const float* __restrict__ feature, const float* __restrict__ pseudo_normal,
               const int* __restrict__ n_contrib, const float* __restrict__ gt, const float* __restrict__ bg,
               const float* __restrict__ image_mask, float w_l1, float w_pbr, float w_normal,
               const float* __restrict__ extra_dimage,
               const float* __restrict__ extra_dsrgb, float* __restrict__ dL_dimage,
               float* __restrict__ dL_dopacity, float* __restrict__ dL_dfeature, float* __restrict__ sums)
{
    __shared__ float s_part[4];
    float s_l1 = 0.f, s_pbr = 0.f, s_n = 0.f;
    // grid-stride: a few hundred blocks, so the three same-address atomics per block do not serialise the kernel
    for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += gridDim.x * 256) {
        // every load of the pixel first (up to 20 of them, no branch around any: as written per channel -- load, use, store, next
        // channel -- the compiler kept that order and the kernel waited for memory eight times per pixel: tools/isa_waits.py)
        const float op = opacity[i];
        const int nc = n_contrib[i];
        float v_gt[3], v_im[3], v_ei[3], v_F[3], v_es[3], v_Fn[3], v_pn[3];
        const bool normal_on = !SPARSE || w_normal != 0.f;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            v_gt[c] = gt[(size_t)c * HW + i];
            v_im[c] = image[(size_t)c * HW + i];
            v_F[c] = feature[(size_t)(2 + c) * HW + i];
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {
            v_ei[c] = extra_dimage ? extra_dimage[(size_t)c * HW + i] : 0.f;
            v_es[c] = extra_dsrgb ? extra_dsrgb[(size_t)c * HW + i] : 0.f;
        }
        float mk = 1.f;
        if (normal_on) {
            mk = image_mask ? image_mask[i] : 1.f;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                v_Fn[c] = feature[(size_t)(5 + c) * HW + i];
                v_pn[c] = pseudo_normal[(size_t)c * HW + i];
            }
        }
        const S2Divide dv = s2_divide(op, nc);
        float g_op = 0.f;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            // extra_*: gradients of further terms on the same two images (the SSIM terms, r3dg_ssim_backward)
            dL_dimage[(size_t)c * HW + i] = s2_loss_image(v_im[c], v_gt[c], w_l1, v_ei[c], s_l1);
            dL_dfeature[(size_t)(2 + c) * HW + i] = s2_loss_pbr(v_F[c], v_gt[c], op, bg[c], dv, w_pbr, v_es[c], s_pbr, g_op);
            if (normal_on)       // (image_mask NULL = all ones)
                dL_dfeature[(size_t)(5 + c) * HW + i] = s2_loss_normal(v_Fn[c], v_pn[c], mk, dv, w_normal, s_n, g_op);
        }
        dL_dopacity[i] = g_op;
        if (!SPARSE) {
            dL_dfeature[i] = 0.f;
            dL_dfeature[(size_t)HW + i] = 0.f;
#pragma unroll
            for (int c = 8; c < 16; c++) dL_dfeature[(size_t)c * HW + i] = 0.f;
        }
    }
    const float t0 = block_sum_256(s_l1, s_part);
    __syncthreads();
    const float t1 = block_sum_256(s_pbr, s_part);
    __syncthreads();
    const float t2 = block_sum_256(s_n, s_part);
    if (threadIdx.x == 0) {
        atomicAdd(sum_slot(sums + 0 * R3DG_SUM_SLOTS), t0);
        atomicAdd(sum_slot(sums + 1 * R3DG_SUM_SLOTS), t1);
        atomicAdd(sum_slot(sums + 2 * R3DG_SUM_SLOTS), t2);
    }
}

// ---- launchers ------------------------------------------------------------------------------------------------------
void launch_s2_activate(hipStream_t s, int P, const float* xyz, const float* scaling_raw, const float* rotation_raw,
                        const float* opacity_raw, const float* normal_raw, const float* base_raw,
                        const float* rough_raw, const float* campos, float* scales, float* rot, float* opacity,
                        float* normal, float* base_color, float* roughness, float* viewdirs, const float* viewmatrix,
                        float* features, int n_env, const float* env_raw, float* env, float* zero, int n_zero)
{
    ActivateSide side;
    side.nb_main = (P + 255) / 256;
    side.n_env = env_raw != nullptr && env != nullptr ? n_env : 0;
    side.env_raw = env_raw;
    side.env = env;
    side.zero = zero;
    side.n_zero = zero != nullptr ? n_zero : 0;
    const int work = side.n_env > side.n_zero ? side.n_env : side.n_zero;
    const int nb_side = work > 0 ? (work + 255) / 256 < 8 ? (work + 255) / 256 : 8 : 0;
    s2_activate_kernel<<<side.nb_main + nb_side, 256, 0, s>>>(P, xyz, scaling_raw, rotation_raw, opacity_raw, normal_raw,
                                                              base_raw, rough_raw, campos, scales, rot, opacity, normal,
                                                              base_color, roughness, viewdirs, viewmatrix, features, side);
    check_launch(s, false, "s2_activate_kernel");
}

void launch_s2_pack(hipStream_t s, int P, const float* xyz, const float* viewmatrix, const float* normal,
                    const float* base_color, const float* roughness, const float* shade_out, float* features,
                    float* light_l1_sum)
{
    s2_pack_features_kernel<<<(P + 255) / 256, 256, 0, s>>>(P, xyz, viewmatrix, normal, base_color, roughness,
                                                            shade_out, features, light_l1_sum);
    check_launch(s, false, "s2_pack_features_kernel");
}

void launch_s2_unpack(hipStream_t s, int P, const float* dL_dfeatures, const float* shade_out, float light_weight,
                      float* dL_dpbr, float* dL_ddiffuse, float* block_absmax, float* light_l1_sum, const float* records,
                      const GradRecordLayout* layout)
{
    UnpackRecords rec = {nullptr, 0, {-1, -1, -1, -1, -1, -1}};
    if (records != nullptr && layout != nullptr) {
        const int cols[6] = {2, 3, 4, 12, 13, 14};
        rec.rows = records;
        rec.nvp = layout->nvp;
        for (int k = 0; k < 6; k++) rec.ch[k] = layout->feature[cols[k]];
    }
    s2_unpack_kernel<<<(P + 255) / 256, 256, 0, s>>>(P, dL_dfeatures, shade_out, light_weight, dL_dpbr, dL_ddiffuse,
                                                    block_absmax, light_l1_sum, rec);
    check_launch(s, false, "s2_unpack_kernel");
}

void launch_s2_activate_backward(hipStream_t s, int P, const float* xyz, const float* scaling_raw,
                                 const float* rotation_raw, const float* opacity_raw, const float* normal_raw,
                                 const float* base_raw, const float* rough_raw, const float* viewmatrix,
                                 const float* campos, const float* dL_dfeatures, const float* dL_dbase_shade,
                                 const float* dL_drough_shade, const float* dL_dviewdirs, const float* dL_dscales,
                                 const float* dL_drot, const float* dL_dopacity, const float* dL_dmeans3D, float* g_xyz,
                                 float* g_scaling, float* g_rotation, float* g_opacity, float* g_normal, float* g_base,
                                 float* g_rough, int He, int We, const float* env_raw, const float* env, float* dL_denv,
                                 float w_tv, float* g_env_raw, float* tv_sum, int consume, float* records,
                                 const GradRecordLayout* layout)
{
    ActivateRecords rec = {nullptr, 0, {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}};
    if (records != nullptr && layout != nullptr) {      // (the C-ABI wrapper checked: 16-float rows)
        rec.rows = records;
        rec.opacity = layout->opacity;
        for (int c = 0; c < 12; c++) rec.col[c] = layout->feature[c];
    }
    EnvBackward job;
    job.He = He; job.We = We; job.raw = env_raw; job.env = env; job.dL_denv = dL_denv; job.w_tv = w_tv; job.g_raw = g_env_raw;
    job.tv_sum = tv_sum; job.consume = consume;
    const int nb_main = (P + 255) / 256;
    const int nb_env = env_raw != nullptr ? (He * We * 3 + 255) / 256 : 0;
    s2_activate_backward_kernel<<<nb_main + nb_env, 256, 0, s>>>(
        P, xyz, scaling_raw, rotation_raw, opacity_raw, normal_raw, base_raw, rough_raw, viewmatrix, campos,
        dL_dfeatures, dL_dbase_shade, dL_drough_shade, dL_dviewdirs, dL_dscales, dL_drot, dL_dopacity, dL_dmeans3D, g_xyz,
        g_scaling, g_rotation, g_opacity, g_normal, g_base, g_rough, nb_main, job, rec);
    check_launch(s, false, "s2_activate_backward_kernel");
    if (rec.rows != nullptr) gradient_records_zeroed(records);
}

void launch_s2_normals_srgb(hipStream_t s, int W, int H, const float* vm, float focal_x, float focal_y, float cx, float cy,
                            const float* opacity, const float* depths, float* normals, float* surface_xyz, const float* feature,
                            const int* n_contrib, const float* bg, float* srgb)
{
    dim3 grid((W + 63) / 64, (H + 3) / 4);
    s2_normals_srgb_kernel<<<grid, 256, 0, s>>>(W, H, focal_x, focal_y, cx, cy, vm, opacity, depths, normals, surface_xyz,
                                                feature, n_contrib, bg, srgb);
    check_launch(s, false, "s2_normals_srgb_kernel");
}

void launch_s2_pbr_srgb(hipStream_t s, int HW, const float* opacity, const float* feature, const int* n_contrib,
                        const float* bg, float* srgb)
{
    s2_pbr_srgb_kernel<<<(HW + 255) / 256, 256, 0, s>>>(HW, opacity, feature, n_contrib, bg, srgb);
    check_launch(s, false, "s2_pbr_srgb_kernel");
}

// grid of the stage-2 loss kernel: 768 workgroups measured best (1536: +4 us, 2500: +5 us even with the slot-spread sums)
constexpr int LOSS_BLOCKS = 768;

void launch_s2_loss(hipStream_t s, int HW, const float* image, const float* opacity, const float* feature,
                    const float* pseudo_normal, const int* n_contrib, const float* gt, const float* bg,
                    const float* image_mask, float w_l1, float w_pbr, float w_normal, const float* extra_dimage,
                    const float* extra_dsrgb, float* dL_dimage, float* dL_dopacity, float* dL_dfeature, float* sums,
                    int sparse)
{
    if (sparse)
        s2_loss_kernel<true><<<min((HW + 255) / 256, LOSS_BLOCKS), 256, 0, s>>>(
            HW, image, opacity, feature, pseudo_normal, n_contrib, gt, bg, image_mask, w_l1, w_pbr, w_normal, extra_dimage,
            extra_dsrgb, dL_dimage, dL_dopacity, dL_dfeature, sums);
    else
        s2_loss_kernel<false><<<min((HW + 255) / 256, LOSS_BLOCKS), 256, 0, s>>>(
            HW, image, opacity, feature, pseudo_normal, n_contrib, gt, bg, image_mask, w_l1, w_pbr, w_normal, extra_dimage,
            extra_dsrgb, dL_dimage, dL_dopacity, dL_dfeature, sums);
    check_launch(s, false, "s2_loss_kernel");
}

void launch_s2_env_backward(hipStream_t s, int He, int We, const float* raw, const float* env, float* dL_denv,
                            float w_tv, float* g_raw, float* tv_sum, int consume)
{
    EnvBackward job;
    job.He = He; job.We = We; job.raw = raw; job.env = env; job.dL_denv = dL_denv; job.w_tv = w_tv; job.g_raw = g_raw;
    job.tv_sum = tv_sum; job.consume = consume;
    s2_env_backward_kernel<<<(He * We * 3 + 255) / 256, 256, 0, s>>>(job);
    check_launch(s, false, "s2_env_backward_kernel");
}

}  // namespace r3dg
