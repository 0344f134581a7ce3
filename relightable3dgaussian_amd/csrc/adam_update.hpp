// The Adam update of one element and the nontemporal float4 accesses of the moments: ONE definition for adam_kernel (adam.hip)
// and for the projection backward that applies the SH colour group's Adam itself (rasterizer_preprocess_bwd.hip).  Both units are
// built with the same flags (build.py: no per-file extras), so the statements below compile to the same instructions in both and
// parameters and moments come out bit for bit the same whichever kernel applies the update.
#pragma once
#include <hip/hip_runtime.h>

namespace r3dg {

#ifndef R3DG_ADAM_NT
#define R3DG_ADAM_NT 1              // the moments are read and written ONCE per iteration: nontemporal accesses
#endif

__device__ __forceinline__ float4 adam_load(const float* p, bool nt)
{
    if (nt && R3DG_ADAM_NT) {
        const float4* q = reinterpret_cast<const float4*>(p);
        return make_float4(__builtin_nontemporal_load(&q->x), __builtin_nontemporal_load(&q->y), __builtin_nontemporal_load(&q->z),
                           __builtin_nontemporal_load(&q->w));
    }
    return *reinterpret_cast<const float4*>(p);
}
__device__ __forceinline__ void adam_store(float* p, const float (&v)[4], bool nt)
{
    if (nt && R3DG_ADAM_NT) {
        float4* q = reinterpret_cast<float4*>(p);
        __builtin_nontemporal_store(v[0], &q->x);
        __builtin_nontemporal_store(v[1], &q->y);
        __builtin_nontemporal_store(v[2], &q->z);
        __builtin_nontemporal_store(v[3], &q->w);
        return;
    }
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}

// two learning rates per group: elements whose index modulo `period` is below `split` use lr, the rest lr_tail
// (one [P,16,3] SH tensor = dc columns + rest columns with different rates, gaussian_model.py:470-471); index < 2^32
__device__ __forceinline__ float adam_rate(unsigned int index, float lr, float lr_tail, unsigned int period, unsigned int split)
{
    return (period != 0 && (index % period) >= split) ? lr_tail : lr;
}

// torch.optim.Adam's update of one element (no weight decay / amsgrad); bias1 = 1 - beta1^step, inv_sqrt_bias2 =
// 1 / sqrt(1 - beta2^step), formed on the host in double (adam_bias).  With gk = g * grad_scale (e.g. 1 / world_size after a sum
// all-reduce):
//     m = m + (gk - m) * (1 - beta1)      v = beta2 * v + (1 - beta2) * gk * gk      p -= (lr / bias1) * (m / (sqrt(v) * isb2 + eps))
// Which products the compiler fuses with the addition behind them depends on the code AROUND the statements: written plainly,
// adam_kernel and the projection backward's tail came out one ulp apart in v.  So contraction is OFF here and every fused
// multiply-add is spelled out -- the very ones adam_kernel has always been compiled to (read off its ISA), so its results are
// what they were; division and square root are the correctly rounded ones in both units.
__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, float lr, float beta1, float beta2, float eps,
                                            float bias1, float inv_sqrt_bias2, float grad_scale)
{
#pragma clang fp contract(off)
    const float gk = g * grad_scale;
    m = fmaf(1.f - beta1, fmaf(grad_scale, g, -m), m);
    v = fmaf(beta2, v, gk * ((1.f - beta2) * gk));
    const float denom = fmaf(sqrtf(v), inv_sqrt_bias2, eps);
    p = fmaf(-(lr / bias1), m / denom, p);
}

// (host) the two bias corrections of step `step`, as every launcher hands them to its kernel
struct AdamBias {
    float bias1, inv_sqrt_bias2;
};
AdamBias adam_bias(float beta1, float beta2, int step);        // adam.hip

}  // namespace r3dg
