// Device helpers shared by the shading kernel families (general, fixed ray set, relight): the lat-long environment lookup
// (branch-free acos / atan2, bilinear taps and their 12-byte packed form, the float4-texel fetch), the global -> LDS DMA
// loads, and rotation_between_z.
#pragma once
#include "common.hpp"
#include "ray_set.hpp"
#include "shading_math.hpp"

namespace r3dg {

// acos / atan2 for the lat-long lookup, branch-free (Cephes single-precision minimax polynomials, ~1 ulp like the libm
// versions they replace at about a third of the instructions: the lookup runs once per cached sample, forward and
// backward).  acos: |x| <= 0.5 -> pi/2 - asin(x), else 2 asin(sqrt((1-|x|)/2)) reflected; atan: argument reduced to
// [0, tan(pi/8)] by the octant identities.
__device__ __forceinline__ float fast_acosf(float x)
{
    const float ax = fabsf(x);
    const bool big = ax > 0.5f;
    const float z = big ? 0.5f * (1.0f - ax) : x * x;
    const float s = big ? sqrtf(z) : ax;
    float p = 4.2163199048e-2f;
    p = p * z + 2.4181311049e-2f;
    p = p * z + 4.5470025998e-2f;
    p = p * z + 7.4953002686e-2f;
    p = p * z + 1.6666752422e-1f;
    const float a = s + s * z * p;                         // asin(s)
    const float pos = big ? 2.0f * a : 1.5707963267948966f - a;      // acos(|x|)
    return x >= 0.f ? pos : 3.14159265358979323846f - pos;
}

__device__ __forceinline__ float fast_atan2f(float y, float x)
{
    const float ax = fabsf(x), ay = fabsf(y);
    const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
    float a = mx > 0.f ? mn / mx : 0.f;                    // in [0,1]
    const bool hi = a > 0.4142135623730950f;               // tan(pi/8)
    a = hi ? (a - 1.0f) / (a + 1.0f) : a;
    const float z = a * a;
    float p = 8.05374449538e-2f;
    p = p * z - 1.38776856032e-1f;
    p = p * z + 1.99777106478e-1f;
    p = p * z - 3.33329491539e-1f;
    float r = p * z * a + a;
    r = hi ? r + 0.7853981633974483f : r;
    r = ay > ax ? 1.5707963267948966f - r : r;
    r = x < 0.f ? 3.14159265358979323846f - r : r;
    return __uint_as_float(__float_as_uint(r) | (__float_as_uint(y) & 0x80000000u));     // copysign: atan2(-0, x<0) = -pi
}

struct EnvTap {
    int idx[4];      // texel index (y*We + x), -1 when out of range (zero padding)
    float w[4];
};

// lat-long lookup coordinates + bilinear taps (direct_light_map.py:70-83; grid_sample align_corners=True, zeros)
__device__ __forceinline__ EnvTap env_taps(float dx, float dy, float dz, const float* __restrict__ tr, int He, int We)
{
    if (tr != nullptr) {
        const float tx = dx * tr[0] + dy * tr[1] + dz * tr[2];
        const float ty = dx * tr[3] + dy * tr[4] + dz * tr[5];
        const float tz = dx * tr[6] + dy * tr[7] + dz * tr[8];
        dx = tx; dy = ty; dz = tz;
    }
    const float phi = fast_acosf(dz) - 1e-6f;
    const float theta = fast_atan2f(dy, dx);
    const float qy = (phi / kPi) * 2.f - 1.f;
    const float qx = -theta / kPi;
    const float ix = (qx + 1.f) * 0.5f * (float)(We - 1);
    const float iy = (qy + 1.f) * 0.5f * (float)(He - 1);
    const float x0f = floorf(ix), y0f = floorf(iy);
    const float wx1 = ix - x0f, wy1 = iy - y0f, wx0 = 1.f - wx1, wy0 = 1.f - wy1;
    const int x0 = (int)x0f, y0 = (int)y0f;
    EnvTap t;
    const int xs[2] = {x0, x0 + 1}, ys[2] = {y0, y0 + 1};
    const float wxs[2] = {wx0, wx1}, wys[2] = {wy0, wy1};
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) {
            const bool ok = xs[b] >= 0 && xs[b] <= We - 1 && ys[a] >= 0 && ys[a] <= He - 1;
            t.idx[a * 2 + b] = ok ? ys[a] * We + xs[b] : -1;
            t.w[a * 2 + b] = wys[a] * wxs[b];
        }
    return t;
}

struct PackedTap {           // 12 bytes per cached sample
    uint32_t xy;             // (x0 + 1) | (y0 + 1) << 16, (x0, y0) = floor of the lat-long pixel coordinate (>= -1)
    float wx1, wy1;          // bilinear weights of column x0 + 1 / row y0 + 1
};

__device__ __forceinline__ PackedTap make_tap(float dx, float dy, float dz, const float* __restrict__ tr, int He, int We)
{
    if (tr != nullptr) {
        const float tx = dx * tr[0] + dy * tr[1] + dz * tr[2];
        const float ty = dx * tr[3] + dy * tr[4] + dz * tr[5];
        const float tz = dx * tr[6] + dy * tr[7] + dz * tr[8];
        dx = tx; dy = ty; dz = tz;
    }
    const float phi = fast_acosf(dz) - 1e-6f;
    const float theta = fast_atan2f(dy, dx);
    const float qy = (phi / kPi) * 2.f - 1.f;
    const float qx = -theta / kPi;
    const float ix = (qx + 1.f) * 0.5f * (float)(We - 1);
    const float iy = (qy + 1.f) * 0.5f * (float)(He - 1);
    const float x0f = floorf(ix), y0f = floorf(iy);
    PackedTap t;
    t.wx1 = ix - x0f;
    t.wy1 = iy - y0f;
    const int x0 = max((int)x0f, -1), y0 = max((int)y0f, -1);
    t.xy = (uint32_t)(x0 + 1) | ((uint32_t)(y0 + 1) << 16);
    return t;
}

// cached lookup record -> the four (texel, weight) taps of env_taps (texel -1 = zero padding)
__device__ __forceinline__ EnvTap taps_from_packed(const PackedTap& t, int He, int We)
{
    const int x0 = (int)(t.xy & 0xffffu) - 1, y0 = (int)(t.xy >> 16) - 1;
    const float wx[2] = {1.f - t.wx1, t.wx1}, wy[2] = {1.f - t.wy1, t.wy1};
    EnvTap o;
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) {
            const int x = x0 + b, y = y0 + a;
            const bool ok = x >= 0 && x <= We - 1 && y >= 0 && y <= He - 1;
            o.idx[a * 2 + b] = ok ? __mul24(y, We) + x : -1;
            o.w[a * 2 + b] = wy[a] * wx[b];
        }
    return o;
}

// bilinear sample with zero padding (grid_sample align_corners=True, padding_mode zeros) from a packed tap; the texture
// holds one float4 per texel (LDS or global)
__device__ __forceinline__ void env_fetch(const PackedTap& t, const float4* tex4, int He, int We, float (&e)[3],
                                          int (&tex)[4], float (&w)[4])
{
    const int x0 = (int)(t.xy & 0xffffu) - 1, y0 = (int)(t.xy >> 16) - 1;
    const float wx0 = 1.f - t.wx1, wy0 = 1.f - t.wy1;
    const bool xa = x0 >= 0, xb = x0 + 1 <= We - 1, ya = y0 >= 0, yb = y0 + 1 <= He - 1;    // x0 <= We-1, y0 <= He-1 always
    const int xc0 = xa ? x0 : 0, xc1 = xb ? x0 + 1 : We - 1, yc0 = ya ? y0 : 0, yc1 = yb ? y0 + 1 : He - 1;
    const float fx0 = xa ? wx0 : 0.f, fx1 = xb ? t.wx1 : 0.f, fy0 = ya ? wy0 : 0.f, fy1 = yb ? t.wy1 : 0.f;
    const int r0 = __mul24(yc0, We), r1 = __mul24(yc1, We);          // 24-bit operands (He, We <= 32767): full-rate multiply
    tex[0] = r0 + xc0; tex[1] = r0 + xc1; tex[2] = r1 + xc0; tex[3] = r1 + xc1;
    w[0] = fy0 * fx0; w[1] = fy0 * fx1; w[2] = fy1 * fx0; w[3] = fy1 * fx1;
    e[0] = e[1] = e[2] = 0.f;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const float4 v = tex4[tex[q]];
        e[0] += v.x * w[q]; e[1] += v.y * w[q]; e[2] += v.z * w[q];
    }
}

// rotation_between_z and the direction of a sample of the fixed ray set: ray_set.hpp (shared with the visibility trace)

// ---- register-free prefetch: global -> LDS DMA (global_load_lds), double buffered per wave -----------------------------
// Every wave owns two copies of {4 uniform records (4x64 floats), its 4 Gaussians' next 64 sample directions (4x64x3),
// visibilities (4x64), areas (4x64)}.  While the wave computes on one copy, the loads of its NEXT (Gaussian group,
// 64-sample block) are in flight into the other: the HBM/L2 latency of the three [P,K,*] caches and of the per-Gaussian
// record is hidden without spending VGPRs or extra waves (the kernels run at 2 waves/SIMD).  The LDS image of a DMA
// load is wave base + lane * size, so the copies keep the global layout: dirs [grp][k][3], vis/area [grp][k],
// record [grp][64].  With K % 4 == 0 every lane moves 16 bytes per instruction (9 DMA instructions per block),
// otherwise 4 bytes (24 instructions).
// The DMA is issued from inline assembly on purpose: the compiler's wait-count pass does not tell which LDS-DMA load
// feeds which LDS read and drains the whole vector-memory queue (s_waitcnt vmcnt(0)) in front of the first LDS access
// after a __builtin_amdgcn_global_load_lds -- including the prefetch that was just issued.  Loads it does not know
// about can only make its own waits stricter, never too weak (vmcnt completes in order), and the one true dependency
// -- "my previous prefetch has landed" -- is a single explicit s_waitcnt at the top of each block.  m0 (LDS base of
// the DMA) is saved and restored inside the statement.
template <int BYTES>
__device__ __forceinline__ void lds_dma(const float* gptr, float* lds_base /* wave-uniform */)
{
    const unsigned int off = __builtin_amdgcn_readfirstlane(
        (unsigned int)(size_t)(__attribute__((address_space(3))) float*)lds_base);
    unsigned int saved;
    if (BYTES == 16)
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\t"
                     "s_mov_b32 m0, %0" : "=&s"(saved) : "v"(gptr), "s"(off) : "memory");
    else
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\t"
                     "s_mov_b32 m0, %0" : "=&s"(saved) : "v"(gptr), "s"(off) : "memory");
}
// the same with the LDS byte address already in an SGPR (lds_address_of, computed once per wave): the generic-pointer form above
// costs a 64-bit VGPR pair + a null test per destination, which the compiler hoists out of loops and keeps live
__device__ __forceinline__ unsigned int lds_address_of(const float* lds_ptr /* wave-uniform */)
{
    return __builtin_amdgcn_readfirstlane((unsigned int)(size_t)(__attribute__((address_space(3))) const float*)lds_ptr);
}
template <int BYTES>
__device__ __forceinline__ void lds_dma_at(const float* gptr, unsigned int lds_byte_address /* SGPR */)
{
    unsigned int saved;
    if (BYTES == 16)
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\t"
                     "s_mov_b32 m0, %0" : "=&s"(saved) : "v"(gptr), "s"(lds_byte_address) : "memory");
    else
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\t"
                     "s_mov_b32 m0, %0" : "=&s"(saved) : "v"(gptr), "s"(lds_byte_address) : "memory");
}

// all DMA loads of this wave have landed (they are the only vector-memory loads in the steady-state loop)
__device__ __forceinline__ void wait_block_loads() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

}  // namespace r3dg
