// Device view store for gfx950 (r3dg_hip.h "r3dg_view_unpack"): the ground-truth views of a dataset stay on the device as the 8-bit
// pixels their files hold, and ONE launch per training iteration turns the chosen view into the [3,H,W] image over the background
// and the [1,H,W] mask the fused steps read -- bit for bit what the reference's reader makes of the file on the host
// (scene/utils.py:47-48, dataset_readers.py:246-249, camera_utils.py:35,56, cameras.py:34).
//
//   view_unpack_kernel<C>   flat over the N = H*W pixels, a lane = 4 consecutive pixels:
//       load     RGBA: one 16-byte load; RGB: three 4-byte loads (12 bytes).  A pixel pointer that is not 16-byte (RGB: 4-byte)
//                aligned, and the last lane when N % 4 != 0, read single bytes -- only the bytes of their own pixels.
//       compute  u = byte / 255, a = alpha / 255 (C = 3: a = 1), x = u * a + bg * (1 - a): float64, every operation rounded on its
//                own (the file is compiled with -ffp-contract=off and the operations are spelled with the _rn intrinsics), then
//                (float)x clamped to [0,1] as torch.clamp does (a NaN stays one); mask = (float)a.
//       store    one 16-byte store per plane: a wave writes 1 KB contiguous per plane.  A plane whose lane address is not 16-byte
//                aligned (the output pointer itself, or N % 4 != 0 for planes 1 and 2) and the last lane store single floats.
//   256-thread workgroups, no LDS, no atomics; the 4 pixels live in named registers (no indexed local array): no scratch.
//
//   view_unpack_masked_kernel   (r3dg_hip.h "r3dg_view_unpack_masked") a view whose mask is a file of its own -- the NeILF layout,
//       scene/utils.py:52-57, dataset_readers.py:358-364: RGB pixels [H,W,3] and a one-byte mask plane [H,W].  Same lane shape:
//       three 4-byte loads of the pixels and one 4-byte load of the mask bytes, one 16-byte store per plane.  m = byte > 0,
//       image = (float)((byte / 255 in float64) * m) clamped, mask = m; no background (the reader composites none here).
#include "launchers.hpp"

namespace r3dg {

namespace {

__device__ __forceinline__ bool aligned16(const void* p) { return ((size_t)p & 15) == 0; }

__device__ __forceinline__ float clamp01(float x) { return x < 0.f ? 0.f : (x > 1.f ? 1.f : x); }

// one pixel packed as r | g << 8 | b << 16 | a << 24 -> its three composited colours and its mask value
__device__ __forceinline__ void unpack_pixel(uint32_t px, double bg0, double bg1, double bg2, float& r, float& g, float& b,
                                             float& m)
{
    const double a = __ddiv_rn((double)(px >> 24), 255.0);
    const double na = __dsub_rn(1.0, a);
    const double ur = __ddiv_rn((double)(px & 255u), 255.0);
    const double ug = __ddiv_rn((double)((px >> 8) & 255u), 255.0);
    const double ub = __ddiv_rn((double)((px >> 16) & 255u), 255.0);
    r = clamp01((float)__dadd_rn(__dmul_rn(ur, a), __dmul_rn(bg0, na)));
    g = clamp01((float)__dadd_rn(__dmul_rn(ug, a), __dmul_rn(bg1, na)));
    b = clamp01((float)__dadd_rn(__dmul_rn(ub, a), __dmul_rn(bg2, na)));
    m = (float)a;
}

// the lane's n <= 4 floats of one plane at dst (= plane + first pixel of the lane)
__device__ __forceinline__ void store_lane(float* dst, int n, float v0, float v1, float v2, float v3)
{
    if (n == 4 && aligned16(dst)) {
        // (a native clang vector: HIP's float4 is a struct, its store is split into four floats, and the compiler then folds this
        // branch into the scalar stores below -- 12 + 4 byte stores for every lane)
        typedef float vec4 __attribute__((ext_vector_type(4)));
        *reinterpret_cast<vec4*>(dst) = vec4{v0, v1, v2, v3};
        return;
    }
    if (n > 0) dst[0] = v0;
    if (n > 1) dst[1] = v1;
    if (n > 2) dst[2] = v2;
    if (n > 3) dst[3] = v3;
}

template <int C>
__device__ __forceinline__ uint32_t load_pixel_bytes(const uint8_t* p)
{
    uint32_t px = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
    return px | (C == 4 ? ((uint32_t)p[3] << 24) : 0xff000000u);
}

template <int C>
__global__ void __launch_bounds__(256)
view_unpack_kernel(uint32_t N, const uint8_t* __restrict__ pixels, const float* __restrict__ background,
                   float* __restrict__ image, float* __restrict__ mask)
{
    const size_t first = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;          // the lane's first pixel
    if (first >= N) return;
    const int n = (N - first < 4) ? (int)(N - first) : 4;
    const uint8_t* src = pixels + first * C;
    uint32_t p0 = 0, p1 = 0, p2 = 0, p3 = 0;
    if (n == 4 && C == 4 && aligned16(src)) {
        const uint4 v = *reinterpret_cast<const uint4*>(src);
        p0 = v.x, p1 = v.y, p2 = v.z, p3 = v.w;
    } else if (n == 4 && C == 3 && ((size_t)src & 3) == 0) {
        const uint32_t* w = reinterpret_cast<const uint32_t*>(src);
        const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];                          // bytes r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
        p0 = (w0 & 0x00ffffffu) | 0xff000000u;
        p1 = (w0 >> 24) | ((w1 & 0x0000ffffu) << 8) | 0xff000000u;
        p2 = (w1 >> 16) | ((w2 & 0x000000ffu) << 16) | 0xff000000u;
        p3 = (w2 >> 8) | 0xff000000u;
    } else {
        p0 = load_pixel_bytes<C>(src);
        if (n > 1) p1 = load_pixel_bytes<C>(src + C);
        if (n > 2) p2 = load_pixel_bytes<C>(src + 2 * C);
        if (n > 3) p3 = load_pixel_bytes<C>(src + 3 * C);
    }
    const double bg0 = (double)background[0], bg1 = (double)background[1], bg2 = (double)background[2];
    float r0, g0, b0, m0, r1, g1, b1, m1, r2, g2, b2, m2, r3, g3, b3, m3;
    unpack_pixel(p0, bg0, bg1, bg2, r0, g0, b0, m0);
    unpack_pixel(p1, bg0, bg1, bg2, r1, g1, b1, m1);
    unpack_pixel(p2, bg0, bg1, bg2, r2, g2, b2, m2);
    unpack_pixel(p3, bg0, bg1, bg2, r3, g3, b3, m3);
    store_lane(image + first, n, r0, r1, r2, r3);
    store_lane(image + (size_t)N + first, n, g0, g1, g2, g3);
    store_lane(image + 2 * (size_t)N + first, n, b0, b1, b2, b3);
    if (mask) store_lane(mask + first, n, m0, m1, m2, m3);
}

// a pixel of the NeILF layout: px as unpack_pixel takes it (alpha bits unused), mb its mask byte
__device__ __forceinline__ void unpack_masked_pixel(uint32_t px, uint32_t mb, float& r, float& g, float& b, float& m)
{
    const double md = mb ? 1.0 : 0.0;                                           // mask[mask > 0.5] = 1 on the float of the byte
    r = clamp01((float)__dmul_rn(__ddiv_rn((double)(px & 255u), 255.0), md));
    g = clamp01((float)__dmul_rn(__ddiv_rn((double)((px >> 8) & 255u), 255.0), md));
    b = clamp01((float)__dmul_rn(__ddiv_rn((double)((px >> 16) & 255u), 255.0), md));
    m = (float)md;
}

__global__ void __launch_bounds__(256)
view_unpack_masked_kernel(uint32_t N, const uint8_t* __restrict__ pixels, const uint8_t* __restrict__ mask_bytes,
                          float* __restrict__ image, float* __restrict__ mask)
{
    const size_t first = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;          // the lane's first pixel
    if (first >= N) return;
    const int n = (N - first < 4) ? (int)(N - first) : 4;
    const uint8_t* src = pixels + first * 3;
    const uint8_t* msrc = mask_bytes + first;
    uint32_t p0 = 0, p1 = 0, p2 = 0, p3 = 0, mw = 0;
    if (n == 4 && ((size_t)src & 3) == 0) {
        const uint32_t* w = reinterpret_cast<const uint32_t*>(src);
        const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];                          // bytes r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
        p0 = w0 & 0x00ffffffu;
        p1 = (w0 >> 24) | ((w1 & 0x0000ffffu) << 8);
        p2 = (w1 >> 16) | ((w2 & 0x000000ffu) << 16);
        p3 = w2 >> 8;
    } else {
        p0 = load_pixel_bytes<3>(src);
        if (n > 1) p1 = load_pixel_bytes<3>(src + 3);
        if (n > 2) p2 = load_pixel_bytes<3>(src + 6);
        if (n > 3) p3 = load_pixel_bytes<3>(src + 9);
    }
    if (n == 4 && ((size_t)msrc & 3) == 0) {
        mw = *reinterpret_cast<const uint32_t*>(msrc);
    } else {
        mw = msrc[0];
        if (n > 1) mw |= (uint32_t)msrc[1] << 8;
        if (n > 2) mw |= (uint32_t)msrc[2] << 16;
        if (n > 3) mw |= (uint32_t)msrc[3] << 24;
    }
    float r0, g0, b0, m0, r1, g1, b1, m1, r2, g2, b2, m2, r3, g3, b3, m3;
    unpack_masked_pixel(p0, mw & 255u, r0, g0, b0, m0);
    unpack_masked_pixel(p1, (mw >> 8) & 255u, r1, g1, b1, m1);
    unpack_masked_pixel(p2, (mw >> 16) & 255u, r2, g2, b2, m2);
    unpack_masked_pixel(p3, mw >> 24, r3, g3, b3, m3);
    store_lane(image + first, n, r0, r1, r2, r3);
    store_lane(image + (size_t)N + first, n, g0, g1, g2, g3);
    store_lane(image + 2 * (size_t)N + first, n, b0, b1, b2, b3);
    if (mask) store_lane(mask + first, n, m0, m1, m2, m3);
}

}  // namespace

void launch_view_unpack_masked(hipStream_t s, int W, int H, const uint8_t* pixels, const uint8_t* mask_bytes, float* image,
                               float* mask)
{
    const size_t N = (size_t)W * H, lanes = (N + 3) / 4;                         // (N < 2^31: the caller has checked)
    view_unpack_masked_kernel<<<(unsigned)((lanes + 255) / 256), 256, 0, s>>>((uint32_t)N, pixels, mask_bytes, image, mask);
    check_launch(s, false, "view_unpack_masked_kernel");
}

void launch_view_unpack(hipStream_t s, int W, int H, int C, const uint8_t* pixels, const float* background, float* image,
                        float* mask)
{
    const size_t N = (size_t)W * H, lanes = (N + 3) / 4;                         // (N < 2^31: the caller has checked)
    const unsigned blocks = (unsigned)((lanes + 255) / 256);
    if (C == 4)
        view_unpack_kernel<4><<<blocks, 256, 0, s>>>((uint32_t)N, pixels, background, image, mask);
    else
        view_unpack_kernel<3><<<blocks, 256, 0, s>>>((uint32_t)N, pixels, background, image, mask);
    check_launch(s, false, "view_unpack_kernel");
}

}  // namespace r3dg
