// The transport cache of shading_transport.hpp built straight from the ray set: no [P,K,3] direction tensor and no radiance
// records in between.  In a header of its own because it needs the lat-long lookup (shading_lookup.hpp), which the CPU
// emulation in tests/emu cannot compile, and in a unit of its own (shading_relight_rayset.hip) because of the flags that unit
// is compiled with: see there.
#pragma once
#include "shading_lookup.hpp"
#include "shading_transport_layout.hpp"

namespace r3dg {

// =====================================================================================================================
// For callers whose directions are the fixed ray set of ray_set.hpp (relight.RelightRenderer(device_visibility=True): the
// visibility came from r3dg_bvh_trace_bundles, which generates the same rays and stores none): per sample the direction
// d_k = ray_set_direction(rotation_between_z(n), z_k), its lat-long lookup (make_tap, as shade_build_taps_kernel) in the
// optionally rotated light's frame, the bilinear sample of env [He,We,3] with zero padding, and the transport of
// shade_build_transport_kernel -- same sh_basis16 / sh_local_sum, same order of operations -- written to a FRESH buffer,
// plus the 13 per-Gaussian constants.  What the two-kernel path (shade_build_taps_kernel, shade_build_transport_kernel)
// moves per sample: 12 B direction in + 12 B radiance out, then 12 B direction + 12 B radiance + 4 B visibility in + 12 B
// transport out = 52 B; here 4 B visibility in + 12 B transport out, the map through the caches.
// The kernel's shape is the existing builder's: one wave per Gaussian, lane = sample, TR_WAVES waves per block, plain launch.
// BAKED (relight.RelightRenderer(baked_visibility=True)): `visibility` holds no [P,K] samples but the 16 baked SH coefficients
// of every Gaussian [P,16] (visibility_bake), and the sample's visibility is baked_visibility() of them at d_k -- the
// WORLD-frame direction, whatever the light's rotation: visibility is geometry.  Nothing is streamed in per sample.  The traced
// instance (BAKED = false) is the kernel as it was, operation for operation.
// =====================================================================================================================

// clamp(0.5 + sum_i v_i Y_i(d), 0, 1) (gaussian_renderer/neilf_composite.py:229-231; visibility_bake.sh_visibility): `v` the 16
// coefficients of one Gaussian in LDS (4 broadcast ds_read_b128), Y the FULL degree-3 basis at d
__device__ __forceinline__ float baked_visibility(const float* v /*[16] in LDS, 16-byte aligned*/, const float (&Y)[16])
{
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const float4 c4 = reinterpret_cast<const float4*>(v)[q];
        s += c4.x * Y[4 * q];
        s += c4.y * Y[4 * q + 1];
        s += c4.z * Y[4 * q + 2];
        s += c4.w * Y[4 * q + 3];
    }
    return fminf(fmaxf(s + 0.5f, 0.f), 1.f);
}

template <bool BAKED>
__global__ void __launch_bounds__(64 * TR_WAVES)
shade_build_transport_rayset_kernel(int P, int K, int M, const float* __restrict__ normals, const float* __restrict__ incidents,
                                    const float* __restrict__ visibility /*[P,K]; BAKED: [P,16]*/,
                                    const float* __restrict__ zsamples /*[K,3]*/,
                                    float uniform_area, const float* __restrict__ env, int He, int We,
                                    const float* __restrict__ tr, float* __restrict__ transport, float* __restrict__ consts)
{
    __shared__ __attribute__((aligned(16))) float s_sh[TR_WAVES][BAKED ? 64 : 48];     // BAKED: 48..63 the visibility coefficients
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = blockIdx.x * TR_WAVES + wave;
    if (g >= P) return;                                       // whole waves leave; no block-wide barrier below
    float* sh = s_sh[wave];
    if (lane < 48) sh[lane] = lane < 3 * M ? incidents[(size_t)g * 3 * M + lane] : 0.f;
    else if (BAKED) sh[lane] = visibility[(size_t)g * 16 + (lane - 48)];
    __builtin_amdgcn_wave_barrier();      // one wave: its LDS operations execute in order
    const float nx = normals[3 * (size_t)g], ny = normals[3 * (size_t)g + 1], nz = normals[3 * (size_t)g + 2];
    float R[9];
    rotation_between_z(nx, ny, nz, R);
    const size_t row = (size_t)g * (size_t)K;
    float acc[13];
#pragma unroll
    for (int i = 0; i < 13; i++) acc[i] = 0.f;
    const int kend = (K + 63) & ~63;
    for (int k = lane; k < kend; k += 64) {
        if (k < K) {
            float dx, dy, dz;
            ray_set_direction(R, zsamples[3 * k], zsamples[3 * k + 1], zsamples[3 * k + 2], dx, dy, dz);
            float vis;
            if (!BAKED) vis = visibility[row + k];
            // into the light's frame: one multiply and two fused multiply-adds per component, in this order -- the instructions
            // make_tap's own rotation compiles to in shade_build_taps_kernel (the lookup behind it is singular at the poles:
            // another rounding of these sums is another texel fraction there, see shading_relight_rayset.hip)
            float lx = dx, ly = dy, lz = dz;
            if (tr != nullptr) {
                lx = __fmaf_rn(dz, tr[2], __fmaf_rn(dy, tr[1], dx * tr[0]));
                ly = __fmaf_rn(dz, tr[5], __fmaf_rn(dy, tr[4], dx * tr[3]));
                lz = __fmaf_rn(dz, tr[8], __fmaf_rn(dy, tr[7], dx * tr[6]));
            }
            // the radiance of shade_build_taps_kernel (env != nullptr): packed lookup, then the four guarded texels
            const PackedTap t = make_tap(lx, ly, lz, nullptr, He, We);
            const int x0 = (int)(t.xy & 0xffffu) - 1, y0 = (int)(t.xy >> 16) - 1;
            const float wx[2] = {1.f - t.wx1, t.wx1}, wy[2] = {1.f - t.wy1, t.wy1};
            float e[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int b = 0; b < 2; b++) {
                    const int x = x0 + b, y = y0 + a;
                    if (x >= 0 && x <= We - 1 && y >= 0 && y <= He - 1) {
                        const float* px = env + 3 * ((size_t)y * We + x);
                        const float w = wy[a] * wx[b];
                        e[0] += px[0] * w; e[1] += px[1] * w; e[2] += px[2] * w;
                    }
                }
            float Y[16];
            sh_basis16(dx, dy, dz, BAKED ? 16 : M, Y);
            if (BAKED) {
                vis = baked_visibility(sh + 48, Y);
                // the visibility basis is always the full 16; the local light below sees the M of its own coefficients
#pragma unroll
                for (int i = 1; i < 16; i++) Y[i] = i < M ? Y[i] : 0.f;
            }
            float l[3];
            sh_local_sum(sh, Y, l);
            const float area_ndi = uniform_area * fmaxf(nx * dx + ny * dy + nz * dz, 0.f);
            float* o = transport + 3 * (row + k);
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float loc = fmaxf(l[c], 0.f), glob = e[c] * vis, lin = loc + glob, tc = lin * area_ndi;
                o[c] = tc;
                acc[c] += tc;
                acc[3 + c] += lin;
                acc[6 + c] += loc;
                acc[9 + c] += glob;
            }
            acc[12] += vis;
        }
    }
    const float invK = 1.0f / (float)K;
#pragma unroll
    for (int i = 0; i < 13; i++) acc[i] = wave_sum64(acc[i]) * invK;
    if (lane == 0) {
        float* o = consts + (size_t)g * TR_CONSTS;
#pragma unroll
        for (int i = 0; i < TR_CONSTS; i++) o[i] = i < 13 ? acc[i] : 0.f;
    }
}

// =====================================================================================================================
// The same visibility as a [P,K] tensor, for every consumer that takes one (r3dg_shade_build_split, the radiance cache,
// r3dg_shade_forward_cached, relight.frame_reference): one wave per Gaussian, lane = sample, the 16 coefficients read once per
// wave, whole-wave stores of consecutive floats.  No cross-lane operation follows the loop, so it needs no padded trip count.
// =====================================================================================================================
__global__ void __launch_bounds__(64 * TR_WAVES)
visibility_sh_expand_kernel(int P, int K, const float* __restrict__ normals, const float* __restrict__ zsamples /*[K,3]*/,
                            const float* __restrict__ visibility_sh /*[P,16]*/, float* __restrict__ out /*[P,K]*/)
{
    __shared__ __attribute__((aligned(16))) float s_v[TR_WAVES][16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = blockIdx.x * TR_WAVES + wave;
    if (g >= P) return;                                       // whole waves leave; no block-wide barrier below
    float* v = s_v[wave];
    if (lane < 16) v[lane] = visibility_sh[(size_t)g * 16 + lane];
    __builtin_amdgcn_wave_barrier();      // one wave: its LDS operations execute in order
    float R[9];
    rotation_between_z(normals[3 * (size_t)g], normals[3 * (size_t)g + 1], normals[3 * (size_t)g + 2], R);
    const size_t row = (size_t)g * (size_t)K;
    for (int k = lane; k < K; k += 64) {
        float dx, dy, dz;
        ray_set_direction(R, zsamples[3 * k], zsamples[3 * k + 1], zsamples[3 * k + 2], dx, dy, dz);
        float Y[16];
        sh_basis16(dx, dy, dz, 16, Y);
        out[row + k] = baked_visibility(v, Y);
    }
}

}  // namespace r3dg
