// Antialiased downscale of a ground-truth view for gfx950 (r3dg_hip.h "r3dg_view_resize"): what the reference's loadCam makes of a
// view whose `--resolution` scale is not 1 (utils/camera_utils.py:13-58, scene/cameras.py:34), run ONCE per view when the view
// store loads it.  In the reference's order: composite at full size (the arithmetic of r3dg_view_unpack / r3dg_view_unpack_masked,
// rounded to float32, not yet clamped), separable antialiased bilinear filter (torch's `_upsample_bilinear2d_aa`: per axis
// scale = in / out, centre = scale * (i + 0.5), support = scale, taps [int(centre - support + 0.5), int(centre + support + 0.5))
// cut to the image, weight 1 - |(j - centre + 0.5) / scale| normalised to sum 1), clamp to [0,1]; the mask by nearest neighbour
// from the full-size float mask (src = min(floor(dst * float32(in / out)), in - 1)).
//
//   view_resize_kernel<KIND>   KIND 0: RGB, 1: RGBA over the background, 2: RGB + a one-byte mask plane.
//     A 256-thread workgroup owns a tile of 64 x 8 output pixels.
//       weights   lanes 0..63 compute the tap range and the normalised weights of their output column, lanes 64..71 those of the
//                 tile's 8 output rows: in float64, once per workgroup, kept in LDS as float32.  Two 256-entry tables (byte / 255
//                 as float64 and as float32) replace every division of the composite.
//       chunks    the source rows the tile needs, R at a time (R chosen by the launcher so that everything fits 60 KB of LDS):
//         stage       the rows' bytes of the tile's source columns into LDS by 16-byte loads from 16-byte-aligned addresses (the
//                     last 16 bytes of the array, where they would reach past it, by single bytes);
//         horizontal  a wave filters one staged row into 64 output columns x 3 channels (float32 fma over the column's taps, the
//                     composite of a tap from the staged bytes and the tables) -> LDS [R][3][64];
//         vertical    a lane owns output column t % 64 of tile rows t / 64 and t / 64 + 4 and adds the chunk's rows to its six
//                     float32 sums (the row test is uniform over the wave).
//       store     a wave writes 64 consecutive floats of one output row per channel (256 B); the mask is read straight from the
//                 source bytes.
//   No atomics, no indexed local arrays: no scratch.  Compiled with -ffp-contract=off: the composite is the reader's bit for bit.
#include "launchers.hpp"

#include <math.h>
#include <stdexcept>

namespace r3dg {

namespace {

constexpr int TILE_W = 64, TILE_H = 8, THREADS = 256;
constexpr int LDS_BUDGET = 60 * 1024, MAX_CHUNK_ROWS = 16;

__host__ __device__ inline int round16(int x) { return (x + 15) & ~15; }

// LDS layout in bytes (the launcher sizes it, the kernel walks it): every region starts on a 16-byte boundary
struct ResizeLayout {
    int lutd, lut, xmin, xsize, ymin, ysize, wx, wy, hbuf, raw, rawm, total;
};

__host__ __device__ inline ResizeLayout resize_layout(int Kx, int Ky, int R, int rowcap, int mrowcap)
{
    ResizeLayout l;
    l.lutd = 0;
    l.lut = l.lutd + 256 * 8;
    l.xmin = l.lut + 256 * 4;
    l.xsize = l.xmin + TILE_W * 4;
    l.ymin = l.xsize + TILE_W * 4;
    l.ysize = l.ymin + round16(TILE_H * 4);
    l.wx = l.ysize + round16(TILE_H * 4);
    l.wy = l.wx + round16(Kx * TILE_W * 4);
    l.hbuf = l.wy + round16(TILE_H * Ky * 4);
    l.raw = l.hbuf + R * 3 * TILE_W * 4;
    l.rawm = l.raw + R * rowcap;
    l.total = l.rawm + R * mrowcap;
    return l;
}

__device__ __forceinline__ float clamp01(float x) { return x < 0.f ? 0.f : (x > 1.f ? 1.f : x); }

// tap range and normalised weights of output index i of an axis with `in` source samples: weights[k * stride], k < size
__device__ __forceinline__ void axis_weights(int i, int in, double scale, int K, int& first, int& size, float* weights, int stride)
{
    const double support = scale >= 1.0 ? scale : 1.0, invscale = scale >= 1.0 ? __ddiv_rn(1.0, scale) : 1.0;
    const double centre = __dmul_rn(scale, (double)i + 0.5);
    long long lo = (long long)(centre - support + 0.5), hi = (long long)(centre + support + 0.5);
    lo = lo < 0 ? 0 : lo;
    hi = hi > in ? in : hi;
    long long n = hi - lo;
    n = n < 0 ? 0 : (n > K ? K : n);
    first = (int)lo, size = (int)n;
    double total = 0.0;
    for (int k = 0; k < size; k++) {
        const double x = fabs(((double)(k + first) - centre + 0.5) * invscale);
        total += x < 1.0 ? 1.0 - x : 0.0;
    }
    for (int k = 0; k < size; k++) {
        const double x = fabs(((double)(k + first) - centre + 0.5) * invscale);
        const double w = x < 1.0 ? 1.0 - x : 0.0;
        weights[k * stride] = (float)(total != 0.0 ? w / total : w);
    }
}

// rows [y0, y0 + rows) x bytes [x0 * C, x1 * C) of an [H, W * C] byte array -> LDS rows of `rowcap` bytes, row r starting at the
// 16-byte-aligned global address at or below its first byte
__device__ __forceinline__ void stage_rows(const uint8_t* __restrict__ src, size_t total_bytes, int W, int C, int y0, int rows,
                                           int x0, int x1, uint8_t* lds, int rowcap)
{
    const int cap16 = rowcap >> 4;
    for (int item = threadIdx.x; item < rows * cap16; item += THREADS) {
        const int r = item / cap16, i = item - r * cap16;
        const size_t b0 = ((size_t)(y0 + r) * W + x0) * C, b1 = ((size_t)(y0 + r) * W + x1) * C;
        const size_t a = (b0 & ~(size_t)15) + (size_t)i * 16;
        if (a >= b1) continue;
        uint8_t* dst = lds + r * rowcap + i * 16;
        if (a + 16 <= total_bytes) {
            typedef uint32_t uvec4 __attribute__((ext_vector_type(4)));       // (a native vector: one 16-byte load, one LDS store)
            *reinterpret_cast<uvec4*>(dst) = *reinterpret_cast<const uvec4*>(src + a);
        } else {
            for (int k = 0; k < 16; k++)
                if (a + k < total_bytes) dst[k] = src[a + k];
        }
    }
}

template <int KIND>
__global__ void __launch_bounds__(THREADS)
view_resize_kernel(int W, int H, int OW, int OH, const uint8_t* __restrict__ pixels, const uint8_t* __restrict__ mask_bytes,
                   const float* __restrict__ background, double scale_x, double scale_y, float nearest_x, float nearest_y,
                   int Kx, int Ky, int R, int rowcap, int mrowcap, float* __restrict__ image, float* __restrict__ mask)
{
    constexpr int C = KIND == 1 ? 4 : 3;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const ResizeLayout L = resize_layout(Kx, Ky, R, rowcap, mrowcap);
    double* lutd = reinterpret_cast<double*>(lds + L.lutd);
    float* lut = reinterpret_cast<float*>(lds + L.lut);
    int* xmin = reinterpret_cast<int*>(lds + L.xmin);
    int* xsize = reinterpret_cast<int*>(lds + L.xsize);
    int* ymin = reinterpret_cast<int*>(lds + L.ymin);
    int* ysize = reinterpret_cast<int*>(lds + L.ysize);
    float* wx = reinterpret_cast<float*>(lds + L.wx);             // [Kx][64]
    float* wy = reinterpret_cast<float*>(lds + L.wy);             // [8][Ky]
    float* hbuf = reinterpret_cast<float*>(lds + L.hbuf);         // [R][3][64]
    uint8_t* raw = lds + L.raw;                                   // [R][rowcap]
    uint8_t* rawm = lds + L.rawm;                                 // [R][mrowcap]

    const int t = threadIdx.x, ox0 = blockIdx.x * TILE_W, oy0 = blockIdx.y * TILE_H;
    const int lastx = min(TILE_W, OW - ox0) - 1, lasty = min(TILE_H, OH - oy0) - 1;
    {
        const double u = __ddiv_rn((double)t, 255.0);
        lutd[t] = u;
        lut[t] = (float)u;
    }
    if (t < TILE_W) {
        int first = 0, size = 0;
        if (t <= lastx) axis_weights(ox0 + t, W, scale_x, Kx, first, size, wx + t, TILE_W);
        xmin[t] = first, xsize[t] = size;
    } else if (t < TILE_W + TILE_H) {
        const int j = t - TILE_W;
        int first = 0, size = 0;
        if (j <= lasty) axis_weights(oy0 + j, H, scale_y, Ky, first, size, wy + j * Ky, 1);
        ymin[j] = first, ysize[j] = size;
    }
    __syncthreads();

    const int sx0 = xmin[0], sx1 = xmin[lastx] + xsize[lastx], sy0 = ymin[0], sy1 = ymin[lasty] + ysize[lasty];
    const size_t total_bytes = (size_t)W * H * C, total_mask = (size_t)W * H;
    double bg0 = 0.0, bg1 = 0.0, bg2 = 0.0;
    if (KIND == 1) bg0 = (double)background[0], bg1 = (double)background[1], bg2 = (double)background[2];
    const int x = t & (TILE_W - 1), ja = t >> 6, jb = ja + 4;
    const int ya = ymin[ja], na = ysize[ja], yb = ymin[jb], nb = ysize[jb];
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, b0 = 0.f, b1 = 0.f, b2 = 0.f;
    const bool fits = (sx1 - sx0) * C + 15 <= rowcap && (KIND != 2 || (sx1 - sx0) + 15 <= mrowcap);     // (the launcher's bound)

    for (int r0 = sy0; r0 < sy1 && fits; r0 += R) {
        const int rows = min(R, sy1 - r0);
        stage_rows(pixels, total_bytes, W, C, r0, rows, sx0, sx1, raw, rowcap);
        if (KIND == 2) stage_rows(mask_bytes, total_mask, W, 1, r0, rows, sx0, sx1, rawm, mrowcap);
        __syncthreads();
        // horizontal: item = (row of the chunk, output column); a wave takes one row
        for (int item = t; item < rows * TILE_W; item += THREADS) {
            const int r = item >> 6;
            const size_t rowstart = ((size_t)(r0 + r) * W + sx0);
            const uint8_t* p = raw + r * rowcap + (int)((rowstart * C) & 15) + (xmin[x] - sx0) * C;
            const uint8_t* pm = rawm + r * mrowcap + (int)(rowstart & 15) + (xmin[x] - sx0);
            float h0 = 0.f, h1 = 0.f, h2 = 0.f;
            const int n = xsize[x];
            for (int k = 0; k < n; k++, p += C, pm++) {
                const float w = wx[k * TILE_W + x];
                float v0, v1, v2;
                if (KIND == 1) {
                    const double a = lutd[p[3]], inv = __dsub_rn(1.0, a);
                    v0 = (float)__dadd_rn(__dmul_rn(lutd[p[0]], a), __dmul_rn(bg0, inv));
                    v1 = (float)__dadd_rn(__dmul_rn(lutd[p[1]], a), __dmul_rn(bg1, inv));
                    v2 = (float)__dadd_rn(__dmul_rn(lutd[p[2]], a), __dmul_rn(bg2, inv));
                } else {
                    const bool on = KIND == 0 || pm[0] != 0;
                    v0 = on ? lut[p[0]] : 0.f;
                    v1 = on ? lut[p[1]] : 0.f;
                    v2 = on ? lut[p[2]] : 0.f;
                }
                h0 = fmaf(w, v0, h0);
                h1 = fmaf(w, v1, h1);
                h2 = fmaf(w, v2, h2);
            }
            float* h = hbuf + r * 3 * TILE_W + x;
            h[0] = h0, h[TILE_W] = h1, h[2 * TILE_W] = h2;
        }
        __syncthreads();
        // vertical: this lane's two output rows take what the chunk holds of their taps
        for (int r = 0; r < rows; r++) {
            const int ka = r0 + r - ya, kb = r0 + r - yb;
            const float* h = hbuf + r * 3 * TILE_W + x;
            if (ka >= 0 && ka < na) {
                const float w = wy[ja * Ky + ka];
                a0 = fmaf(w, h[0], a0), a1 = fmaf(w, h[TILE_W], a1), a2 = fmaf(w, h[2 * TILE_W], a2);
            }
            if (kb >= 0 && kb < nb) {
                const float w = wy[jb * Ky + kb];
                b0 = fmaf(w, h[0], b0), b1 = fmaf(w, h[TILE_W], b1), b2 = fmaf(w, h[2 * TILE_W], b2);
            }
        }
        __syncthreads();
    }

    const int ox = ox0 + x;
    if (ox >= OW) return;
    const size_t plane = (size_t)OW * OH;
    const int sxn = min((int)floorf(__fmul_rn((float)ox, nearest_x)), W - 1);
    for (int half = 0; half < 2; half++) {
        const int oy = oy0 + (half ? jb : ja);
        if (oy >= OH) continue;
        const size_t o = (size_t)oy * OW + ox;
        image[o] = clamp01(half ? b0 : a0);
        image[plane + o] = clamp01(half ? b1 : a1);
        image[2 * plane + o] = clamp01(half ? b2 : a2);
        if (mask) {
            const int syn = min((int)floorf(__fmul_rn((float)oy, nearest_y)), H - 1);
            const size_t s = (size_t)syn * W + sxn;
            float m = 1.f;
            if (KIND == 1) m = (float)__ddiv_rn((double)pixels[s * 4 + 3], 255.0);
            if (KIND == 2) m = mask_bytes[s] ? 1.f : 0.f;
            mask[o] = m;
        }
    }
}

}  // namespace

void launch_view_resize(hipStream_t s, int W, int H, int C, const uint8_t* pixels, const uint8_t* mask_bytes, const float* background,
                        int OW, int OH, float* image, float* mask)
{
    // (1 <= in / out <= 16 on both axes and W * H < 2^31: the caller has checked)
    const double scale_x = (double)W / OW, scale_y = (double)H / OH;
    const int Kx = 2 * (int)ceil(scale_x) + 1, Ky = 2 * (int)ceil(scale_y) + 1;
    // source columns of a tile: taps of 64 consecutive outputs span at most 63 * scale + 2 * support + 1 samples
    const int span = (int)ceil(63.0 * scale_x + 2.0 * scale_x) + 2;
    const int rowcap = round16(span * C + 15) + 16, mrowcap = mask_bytes ? round16(span + 15) + 16 : 0;
    const int fixed = resize_layout(Kx, Ky, 0, rowcap, mrowcap).total, per_row = 3 * TILE_W * 4 + rowcap + mrowcap;
    int R = (LDS_BUDGET - fixed) / per_row;
    R = R > MAX_CHUNK_ROWS ? MAX_CHUNK_ROWS : R;
    if (R < 1) throw std::runtime_error("view_resize: a chunk of one source row does not fit the LDS budget");
    const size_t lds = (size_t)resize_layout(Kx, Ky, R, rowcap, mrowcap).total;
    const dim3 grid((unsigned)((OW + TILE_W - 1) / TILE_W), (unsigned)((OH + TILE_H - 1) / TILE_H));
    const float nx = (float)W / (float)OW, ny = (float)H / (float)OH;
    if (C == 4)
        view_resize_kernel<1><<<grid, THREADS, lds, s>>>(W, H, OW, OH, pixels, nullptr, background, scale_x, scale_y, nx, ny, Kx, Ky,
                                                         R, rowcap, mrowcap, image, mask);
    else if (mask_bytes)
        view_resize_kernel<2><<<grid, THREADS, lds, s>>>(W, H, OW, OH, pixels, mask_bytes, background, scale_x, scale_y, nx, ny, Kx,
                                                         Ky, R, rowcap, mrowcap, image, mask);
    else
        view_resize_kernel<0><<<grid, THREADS, lds, s>>>(W, H, OW, OH, pixels, nullptr, background, scale_x, scale_y, nx, ny, Kx, Ky,
                                                         R, rowcap, mrowcap, image, mask);
    check_launch(s, false, "view_resize_kernel");
}

}  // namespace r3dg
