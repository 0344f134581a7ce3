// OpenEXR views on the device for gfx950 (r3dg_hip.h "r3dg_exr_unpack_chunks", "r3dg_view_unpack_hdr"; the two decode kernels
// themselves are in exr_decode.hpp, which tests/emu/exr_emu.cpp also compiles for the host).  The host inflates a
// file's ZIP / ZIPS chunks (zlib: serial) and uploads the bytes; everything after the inflate happens here: the byte predictor (a
// running sum mod 256 over the WHOLE chunk), the even / odd byte un-split and the de-planarisation of the chunk's rows into the
// resident planar view [kept,H,W], in the file's own sample type and bit for bit (nothing is converted: NaN payloads and
// denormals pass through).  One launch per training iteration then turns a resident view into the float image the steps read.
//
// Decomposition of the chunk decode: a TWO-PASS TILE-SUM SCAN.  After the inflate a chunk is d[0..n), n even; with half = n / 2
//     t[i] = (d[0] + ... + d[i] + 128 * (i & 1)) mod 256          (t[i] = t[i-1] + d[i] - 128, unrolled: -128 i = 128 (i & 1) mod 256)
//     raw[2j] = t[j], raw[2j+1] = t[half + j]
// so raw bytes [2kT, 2(k+1)T) need exactly t over the LOW tile [kT, (k+1)T) and the HIGH tile [half + kT, half + (k+1)T), and
// each of those needs one number from outside: the byte sum of everything in front of it.
//   exr_tile_sums_kernel   grid (tiles, chunks): the byte sums mod 256 of low tile k and high tile k -> tile_sums[chunk][2][tiles].
//   exr_unpack_kernel<B>   grid (tiles, chunks): carry-in = sum of the tile sums in front (at most a few hundred numbers, summed by
//                          the workgroup: a 512 KB chunk has 64 tiles per half); a lane scans its 16 low and 16 high bytes in
//                          registers, one packed wave scan (v_mov DPP / shuffles) + 4 wave totals through LDS give its offsets;
//                          the interleaved 8 KB of raw bytes go to LDS; then lane i takes samples i, i + 256, ...: consecutive lanes
//                          store consecutive samples of a plane row (a wave writes 128 B / 256 B contiguous per instruction).
// A chunk is never assumed to fit LDS (a ZIP chunk of a 4-channel float file 2048 wide is 512 KB): the tile is the unit, T = 4096
// scan positions per half.  Every tile of every chunk runs in parallel; the inflated bytes are read twice (the second time from
// L2: a view is a few MB), the output is written once.  The alternatives: one workgroup per chunk walking tiles with an LDS carry
// serialises a chunk (an 800 x 800 half RGBA view has 50 chunks: 50 workgroups on 256 CUs); a scan in place in the inflated buffer
// followed by a gather launch writes and re-reads every byte once more.  A chunk stored raw (and every chunk of an uncompressed
// file) skips the scan: its lanes load the 32 raw bytes directly.
//
// Bounds: a table row that does not fit (rows outside [1, max_chunk_rows], a row range outside [0, H), a byte range outside the
// inflated buffer, an offset off the 16-byte grid) makes its workgroups return; nothing outside the planes is written, nothing
// outside the inflated buffer and the tables is read.  256-thread workgroups, 8.1 KB of LDS, no atomics, plain C++ (no inline
// assembly), named registers only (no indexed local arrays): no scratch.
//
//   view_unpack_hdr_kernel<HALF>   flat over the H*W pixels, a lane = one pixel: three 2- or 4-byte loads and a mask byte in,
//       three floats and the mask out (a wave stores 256 B contiguous per plane).  x -> sRGB in float32 with the float32-rounded
//       constants NumPy uses beside a float32 array (scene/utils.py:40-46 -> rgb_to_srgb(clip=False): x > 0.0031308 ?
//       pow(x, 1/2.4) * 1.055 - 0.055 : 12.92 * x), m = byte > 0, image = m ? clamp(srgb, 0, 1) : background, mask = m
//       (dataset_readers.py:551-555 with a 0 / 1 mask is a select; cameras.py:34 clamps; a NaN stays one).  Compiled with
//       -ffp-contract=off: the multiply and the subtraction round separately, as NumPy's do.
#include "launchers.hpp"
#include "exr_decode.hpp"

namespace r3dg {

namespace {

__device__ __forceinline__ float srgb_of(float x)
{
    // the constants as float32, as NumPy takes Python floats beside a float32 array
    return x > 0.0031308f ? powf(x, (float)(1.0 / 2.4)) * 1.055f - 0.055f : 12.92f * x;
}

__device__ __forceinline__ float clamp01(float x) { return x < 0.f ? 0.f : (x > 1.f ? 1.f : x); }

template <bool HALF>
__global__ void __launch_bounds__(256)
view_unpack_hdr_kernel(uint32_t N, const void* __restrict__ view, const uint8_t* __restrict__ mask_bytes,
                       const float* __restrict__ background, float* __restrict__ image, float* __restrict__ mask)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    float r, g, b;
    if (HALF) {
        const uint16_t* v = reinterpret_cast<const uint16_t*>(view);
        r = (float)__builtin_bit_cast(_Float16, v[i]);
        g = (float)__builtin_bit_cast(_Float16, v[(size_t)N + i]);
        b = (float)__builtin_bit_cast(_Float16, v[2 * (size_t)N + i]);
    } else {
        const float* v = reinterpret_cast<const float*>(view);
        r = v[i], g = v[(size_t)N + i], b = v[2 * (size_t)N + i];
    }
    const bool m = mask_bytes ? mask_bytes[i] > 0 : true;
    image[i] = m ? clamp01(srgb_of(r)) : background[0];
    image[(size_t)N + i] = m ? clamp01(srgb_of(g)) : background[1];
    image[2 * (size_t)N + i] = m ? clamp01(srgb_of(b)) : background[2];
    if (mask) mask[i] = m ? 1.f : 0.f;
}

}  // namespace

size_t exr_tiles_per_chunk(int W, int C, int B, int max_rows)
{
    const size_t half = (size_t)max_rows * W * C * B / 2;
    return (half + TILE - 1) / TILE;
}

void launch_exr_unpack_chunks(hipStream_t s, int W, int H, int C, int B, int chunks, int max_rows, const uint8_t* inflated,
                              long long inflated_bytes, const int32_t* table, int kept, const int32_t* kept_channels,
                              uint32_t* tile_sums, void* planes)
{
    const dim3 grid((unsigned)exr_tiles_per_chunk(W, C, B, max_rows), (unsigned)chunks);
    exr_tile_sums_kernel<<<grid, THREADS, 0, s>>>(W, H, C, B, max_rows, inflated, inflated_bytes, table, tile_sums);
    check_launch(s, false, "exr_tile_sums_kernel");
    if (B == 2)
        exr_unpack_kernel<2><<<grid, THREADS, 0, s>>>(W, H, C, max_rows, inflated, inflated_bytes, table, kept, kept_channels,
                                                     tile_sums, planes);
    else
        exr_unpack_kernel<4><<<grid, THREADS, 0, s>>>(W, H, C, max_rows, inflated, inflated_bytes, table, kept, kept_channels,
                                                     tile_sums, planes);
    check_launch(s, false, "exr_unpack_kernel");
}

void launch_view_unpack_hdr(hipStream_t s, int W, int H, int is_half, const void* view, const uint8_t* mask_bytes,
                            const float* background, float* image, float* mask)
{
    const size_t N = (size_t)W * H;                                                  // (N < 2^31: the caller has checked)
    const unsigned blocks = (unsigned)((N + 255) / 256);
    if (is_half)
        view_unpack_hdr_kernel<true><<<blocks, 256, 0, s>>>((uint32_t)N, view, mask_bytes, background, image, mask);
    else
        view_unpack_hdr_kernel<false><<<blocks, 256, 0, s>>>((uint32_t)N, view, mask_bytes, background, image, mask);
    check_launch(s, false, "view_unpack_hdr_kernel");
}

}  // namespace r3dg
