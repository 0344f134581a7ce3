// Per-sample forward of the shading integral with the intermediates its backward needs (SampleFwd, shade_sample), and the
// decisions on max |upstream gradient| that scale the fixed-point texture-gradient accumulation.  Shared by the general
// 16-lane backward (shading.hip) and the fixed-ray-set kernels (shading_frs.hip).
#pragma once
#include "shading_lookup.hpp"

namespace r3dg {

struct SampleFwd {
    float local[3], glob[3], lin[3], transport[3];
    float spec, ndi, area_ndi;
    // intermediates kept for the backward
    float Y[16], shsum[3];
    float L[3], Hh[3], ulen, NoL, NoH, VoH, rawNoH, rawVoH, nom0, nom1, nom2, nomr, frac0, p2;
    EnvTap taps;
    float vis;
};

// Layout of the per-wave uniform record u[64]: 0..47 SH coefficients (i*3+c), 48..50 albedo, 51 roughness,
// 52..54 normal, 55..57 view direction, 58..60 dL_dpbr, 61..63 dL_ddiffuse_light (the last six only in the backward).
template <bool ENV_LDS, bool HAVE_SHSUM = false, bool HAVE_TAP = false>
__device__ __forceinline__ void shade_sample(SampleFwd& s, const GaussFwd& G, const float* sh /*[48] in LDS, zero padded*/,
                                             int M, float dx, float dy, float dz, float vis, float area,
                                             const float* __restrict__ env, const float* s_env,
                                             const float* __restrict__ tr, int He, int We, const PackedTap* cached = nullptr)
{
    // environment light (global) * visibility
    if (HAVE_TAP) s.taps = taps_from_packed(*cached, He, We);
    else s.taps = env_taps(dx, dy, dz, tr, He, We);
    s.vis = vis;
    float e[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 4; t++) {
        if (s.taps.idx[t] >= 0) {
            float3 px;
            if (ENV_LDS) {
                const float* q = s_env + 3 * s.taps.idx[t];
                px = make_float3(q[0], q[1], q[2]);
            } else {
                // large maps live in L2: one 12-byte load per tap (global_load_dwordx3), not three 4-byte ones
                px = *reinterpret_cast<const float3*>(env + 3 * (size_t)s.taps.idx[t]);
            }
            e[0] += px.x * s.taps.w[t];
            e[1] += px.y * s.taps.w[t];
            e[2] += px.z * s.taps.w[t];
        }
    }
    // local incident light: max(SH(d), 0)
    {
        float acc[3];
        if (HAVE_SHSUM) {                        // the caller evaluated the SH sum in an earlier pass (passed via s.shsum)
            acc[0] = s.shsum[0]; acc[1] = s.shsum[1]; acc[2] = s.shsum[2];
        } else {
            sh_basis16(dx, dy, dz, M, s.Y);      // Y[i] = 0 for i >= M, and the LDS record is zero padded
            sh_local_sum(sh, s.Y, acc);
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {
            s.shsum[c] = acc[c];
            s.local[c] = fmaxf(acc[c], 0.f);
            s.glob[c] = e[c] * vis;
            s.lin[c] = s.local[c] + s.glob[c];
        }
    }
    s.ndi = fmaxf(G.n[0] * dx + G.n[1] * dy + G.n[2] * dz, 0.f);
    s.area_ndi = area * s.ndi;
    // GGX specular (neilf.py:374-407)
    const float dlen = fmaxf(sqrtf(dx * dx + dy * dy + dz * dz), 1e-12f);
    s.L[0] = dx / dlen; s.L[1] = dy / dlen; s.L[2] = dz / dlen;
    float u[3];
#pragma unroll
    for (int c = 0; c < 3; c++) u[c] = (s.L[c] + G.V[c]) / 2.0f;
    s.ulen = fmaxf(sqrtf(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]), 1e-12f);
#pragma unroll
    for (int c = 0; c < 3; c++) s.Hh[c] = u[c] / s.ulen;
    s.NoL = fminf(fmaxf(G.N[0] * s.L[0] + G.N[1] * s.L[1] + G.N[2] * s.L[2], 1e-6f), 1.f);
    s.rawNoH = G.N[0] * s.Hh[0] + G.N[1] * s.Hh[1] + G.N[2] * s.Hh[2];
    s.NoH = fminf(fmaxf(s.rawNoH, 1e-6f), 1.f);
    s.rawVoH = G.V[0] * s.Hh[0] + G.V[1] * s.Hh[1] + G.V[2] * s.Hh[2];
    s.VoH = fminf(fmaxf(s.rawVoH, 1e-6f), 1.f);
    const float FMi = (-5.55473f * s.VoH - 6.98316f) * s.VoH;
    s.p2 = exp2f(FMi);
    s.frac0 = 0.04f + 0.96f * s.p2;
    const float frac = s.frac0 * G.a2;
    s.nom0 = s.NoH * s.NoH * (G.a2 - 1.f) + 1.f;
    s.nom1 = G.NoV * (1.f - G.kk) + G.kk;
    s.nom2 = s.NoL * (1.f - G.kk) + G.kk;
    s.nomr = 4.f * kPi * s.nom0 * s.nom0 * s.nom1 * s.nom2;
    const float nom = fminf(fmaxf(s.nomr, 1e-6f), 4.f * kPi);
    s.spec = frac / nom;
#pragma unroll
    for (int c = 0; c < 3; c++) s.transport[c] = s.lin[c] * s.area_ndi;
}

// the largest of `n` non-negative floats (the block maxima of max|upstream gradient|; n == 1: grad_absmax_kernel's word),
// +inf = "some upstream gradient is not finite"; uniform over the wave.  This file is compiled with -ffast-math, which lets the
// compiler assume that no float is inf / nan and fold `x <= FLT_MAX` to true: everything that DECIDES on finiteness works on
// the bit patterns (non-negative floats order like unsigned integers; exponent all ones = inf / nan).
__device__ __forceinline__ bool not_finite_bits(unsigned int bits) { return (bits & 0x7f800000u) == 0x7f800000u; }
__device__ __forceinline__ unsigned int wave_gmax_bits(const unsigned int* __restrict__ gmax_bits, int n)
{
    unsigned int m = 0u;
    for (int i = threadIdx.x & 63; i < n; i += 64) {
        const unsigned int b = gmax_bits[i] & 0x7fffffffu;
        m = not_finite_bits(b) ? 0x7f800000u : (b > m ? b : m);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned int other = (unsigned int)__shfl_xor((int)m, o, 64);
        m = other > m ? other : m;
    }
    return m;
}
// fixed-point accumulation is possible for a positive, finite maximum
__device__ __forceinline__ bool gmax_usable(unsigned int bits) { return bits != 0u && bits < 0x7f800000u; }

}  // namespace r3dg
