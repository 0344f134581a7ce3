// Multi-group Adam step: all parameter groups in one launch (gaussian_model.py:465-497).
#include <cmath>

#include "adam_update.hpp"
#include "launchers.hpp"
#include "r3dg_hip.h"

namespace r3dg {

struct AdamTable {
    r3dg_adam_group g[R3DG_ADAM_MAX_GROUPS];
    unsigned int first_block[R3DG_ADAM_MAX_GROUPS + 1];
    int n_groups;
};

// One float4 per thread and array (ADAM_UNROLL = 1) with NONTEMPORAL accesses for what is touched once per iteration -- the
// gradient and both moments: measured cold (tools/kbench_adam.py: the last-level cache evicted between launches, 958 MB per launch
// at 300k Gaussians): 0.180 ms = 5.33 TB/s = 0.67 of the HBM peak with plain accesses (rounds 1-5), 0.154 ms = 6.21 TB/s = 0.78
// with nontemporal ones -- the rate the guide measures as achievable for a streaming kernel.  More floats per thread do NOT help
// (2 / 4 / 8 float4 per thread and array, all loads issued first: 0.164 / 0.168 / 0.178 ms -- fewer, longer workgroups leave a
// longer tail); the knob stays for the A/B (tools/build_variant.py, -DR3DG_ADAM_UNROLL=n).
#ifndef R3DG_ADAM_UNROLL
#define R3DG_ADAM_UNROLL 1
#endif
constexpr int ADAM_UNROLL = R3DG_ADAM_UNROLL;
constexpr int ADAM_BLOCK_FLOATS = 1024 * ADAM_UNROLL;

__global__ void __launch_bounds__(256)
adam_kernel(AdamTable t, float beta1, float beta2, float eps, float bias1, float inv_sqrt_bias2, float grad_scale,
            const float* __restrict__ skip_flag)
{
    // the gradients belong to a frame the bounded forward dropped on the device (r3dg_rasterize_forward_begin_bounded):
    // no update; the host hears about it later and does not count the step
    if (skip_flag != nullptr && *skip_flag != 0.0f) return;
    int gi = 0;
#pragma unroll 1
    while (gi + 1 < t.n_groups && blockIdx.x >= t.first_block[gi + 1]) gi++;
    const r3dg_adam_group grp = t.g[gi];
    const size_t block_base = (size_t)(blockIdx.x - t.first_block[gi]) * ADAM_BLOCK_FLOATS + threadIdx.x * 4;
    float* __restrict__ p = grp.param;
    const float* __restrict__ g = grp.grad;
    float* __restrict__ m = grp.exp_avg;
    float* __restrict__ v = grp.exp_avg_sq;
    float pv[ADAM_UNROLL][4], gv[ADAM_UNROLL][4], mv[ADAM_UNROLL][4], vv[ADAM_UNROLL][4];
    // every full float4 of this thread first (four arrays x ADAM_UNROLL loads in flight), the ragged tail element-wise
#pragma unroll
    for (int u = 0; u < ADAM_UNROLL; u++) {
        const size_t base = block_base + (size_t)u * 1024;
        if (base + 4 <= grp.n) {
            *reinterpret_cast<float4*>(pv[u]) = *reinterpret_cast<const float4*>(p + base);
            *reinterpret_cast<float4*>(gv[u]) = adam_load(g + base, true);
            *reinterpret_cast<float4*>(mv[u]) = adam_load(m + base, true);
            *reinterpret_cast<float4*>(vv[u]) = adam_load(v + base, true);
        } else {
            for (int k = 0; k < 4; k++)
                if (base + k < grp.n) { pv[u][k] = p[base + k]; gv[u][k] = g[base + k]; mv[u][k] = m[base + k]; vv[u][k] = v[base + k]; }
        }
    }
#pragma unroll
    for (int u = 0; u < ADAM_UNROLL; u++) {
        const size_t base = block_base + (size_t)u * 1024;
        if (base >= grp.n) continue;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            // (the rate by column and the update itself: adam_update.hpp, shared with the projection backward's fused variant)
            const float lr = adam_rate((unsigned int)(base + k), grp.lr, grp.lr_tail, grp.period, grp.split);   // n < 2^32
            adam_update(pv[u][k], gv[u][k], mv[u][k], vv[u][k], lr, beta1, beta2, eps, bias1, inv_sqrt_bias2, grad_scale);
        }
        if (base + 4 <= grp.n) {
            *reinterpret_cast<float4*>(p + base) = *reinterpret_cast<float4*>(pv[u]);
            adam_store(m + base, mv[u], true);
            adam_store(v + base, vv[u], true);
        } else {
            for (int k = 0; k < 4; k++)
                if (base + k < grp.n) { p[base + k] = pv[u][k]; m[base + k] = mv[u][k]; v[base + k] = vv[u][k]; }
        }
    }
}

AdamBias adam_bias(float beta1, float beta2, int step)
{
    const double b1 = 1.0 - pow((double)beta1, (double)step), b2 = 1.0 - pow((double)beta2, (double)step);
    return {(float)b1, (float)(1.0 / sqrt(b2))};
}

void launch_adam(hipStream_t s, int n_groups, const r3dg_adam_group* groups, float beta1, float beta2, float eps,
                 int step, float grad_scale, const float* skip_flag)
{
    AdamTable t;
    t.n_groups = n_groups;
    unsigned int blocks = 0;
    for (int i = 0; i < n_groups; i++) {
        t.g[i] = groups[i];
        t.first_block[i] = blocks;
        blocks += (unsigned int)((groups[i].n + ADAM_BLOCK_FLOATS - 1) / ADAM_BLOCK_FLOATS);
    }
    t.first_block[n_groups] = blocks;
    if (blocks == 0) return;
    const AdamBias b = adam_bias(beta1, beta2, step);
    adam_kernel<<<blocks, 256, 0, s>>>(t, beta1, beta2, eps, b.bias1, b.inv_sqrt_bias2, grad_scale, skip_flag);
    check_launch(s, false, "adam_kernel");
}

}  // namespace r3dg
