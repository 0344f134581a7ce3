// The two launches of the OpenEXR chunk decode (exr_unpack.hip, which explains them): kernels only, no launch syntax, so that the
// same source also runs under the lock-step CPU emulation of tests/emu/exr_emu.cpp.
#pragma once

namespace r3dg {

constexpr int TILE = R3DG_EXR_TILE;                 // scan positions of each half per workgroup = 16 per lane
constexpr int THREADS = 256;
static_assert(TILE == 16 * THREADS, "a lane scans 16 low and 16 high bytes");

// up to 4 bytes at p (n <= 0: none) as a little-endian word
__device__ __forceinline__ uint32_t load_bytes4(const uint8_t* p, int n)
{
    uint32_t w = 0;
    if (n > 0) w = p[0];
    if (n > 1) w |= (uint32_t)p[1] << 8;
    if (n > 2) w |= (uint32_t)p[2] << 16;
    if (n > 3) w |= (uint32_t)p[3] << 24;
    return w;
}

// the n <= 16 bytes at p as four words (bytes past n: zero); only bytes [p, p + n) are read
__device__ __forceinline__ void load16(const uint8_t* p, int n, uint32_t& w0, uint32_t& w1, uint32_t& w2, uint32_t& w3)
{
    if (n == 16 && ((size_t)p & 15) == 0) {
        const uint4 v = *reinterpret_cast<const uint4*>(p);
        w0 = v.x, w1 = v.y, w2 = v.z, w3 = v.w;
    } else if (n == 16 && ((size_t)p & 3) == 0) {
        const uint32_t* w = reinterpret_cast<const uint32_t*>(p);
        w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
    } else {
        w0 = load_bytes4(p, n);
        w1 = load_bytes4(p + 4, n - 4);
        w2 = load_bytes4(p + 8, n - 8);
        w3 = load_bytes4(p + 12, n - 12);
    }
}

__device__ __forceinline__ uint32_t byte_sum(uint32_t w)
{
    const uint32_t pair = (w & 0x00ff00ffu) + ((w >> 8) & 0x00ff00ffu);
    return (pair & 0xffffu) + (pair >> 16);
}

// the four bytes of w replaced by the running sums t: run += byte; t = (run + 128 * parity of the byte's index) mod 256.
// `odd_first`: the index of the word's first byte is odd.
__device__ __forceinline__ uint32_t scan_word(uint32_t w, uint32_t& run, bool odd_first)
{
    const uint32_t pa = odd_first ? 128u : 0u, pb = odd_first ? 0u : 128u;
    run += w & 255u;
    uint32_t t = (run + pa) & 255u;
    run += (w >> 8) & 255u;
    t |= ((run + pb) & 255u) << 8;
    run += (w >> 16) & 255u;
    t |= ((run + pa) & 255u) << 16;
    run += w >> 24;
    t |= ((run + pb) & 255u) << 24;
    return t;
}

// raw bytes 2j = low byte j, 2j + 1 = high byte j, for the lower (a) and the upper (b) two bytes of the words lo and hi
__device__ __forceinline__ void interleave(uint32_t lo, uint32_t hi, uint32_t& a, uint32_t& b)
{
    a = (lo & 0xffu) | ((hi & 0xffu) << 8) | ((lo & 0xff00u) << 8) | ((hi & 0xff00u) << 16);
    b = ((lo >> 16) & 0xffu) | ((hi >> 8) & 0xff00u) | ((lo >> 8) & 0xff0000u) | (hi & 0xff000000u);
}

struct Chunk {
    const uint8_t* bytes;
    uint32_t n;              // raw = inflated bytes of the chunk
    int first_row, rows;
    bool raw, ok;
};

// row `chunk` of the table (offset, first row, rows, stored-raw flag), checked against everything it indexes
__device__ __forceinline__ Chunk read_chunk(const int32_t* __restrict__ table, int chunk, int W, int H, int C, int B, int max_rows,
                                            const uint8_t* inflated, long long inflated_bytes)
{
    Chunk c;
    const uint32_t offset = (uint32_t)table[4 * chunk];
    c.first_row = table[4 * chunk + 1];
    c.rows = table[4 * chunk + 2];
    c.raw = table[4 * chunk + 3] != 0;
    c.ok = c.rows >= 1 && c.rows <= max_rows && c.first_row >= 0 && c.first_row <= H - c.rows && (offset & 15u) == 0;
    c.n = c.ok ? (uint32_t)c.rows * (uint32_t)W * (uint32_t)C * (uint32_t)B : 0;      // (< 2^31: the caller has checked max_rows)
    c.ok = c.ok && (long long)offset + (long long)c.n <= inflated_bytes;
    c.bytes = inflated + offset;
    return c;
}

__global__ void __launch_bounds__(THREADS)
exr_tile_sums_kernel(int W, int H, int C, int B, int max_rows, const uint8_t* __restrict__ inflated, long long inflated_bytes,
                     const int32_t* __restrict__ table, uint32_t* __restrict__ tile_sums)
{
    __shared__ uint32_t wave_sums[THREADS / 64];
    const int tiles = gridDim.x, k = blockIdx.x, chunk = blockIdx.y, tid = threadIdx.x;
    const Chunk c = read_chunk(table, chunk, W, H, C, B, max_rows, inflated, inflated_bytes);
    if (!c.ok || c.raw) return;                                                       // (uniform over the workgroup)
    const uint32_t half = c.n / 2, pos = (uint32_t)k * TILE + 16u * tid;
    const int n = pos >= half ? 0 : (half - pos < 16u ? (int)(half - pos) : 16);
    uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0, b0 = 0, b1 = 0, b2 = 0, b3 = 0;
    if (n > 0) {
        load16(c.bytes + pos, n, a0, a1, a2, a3);
        load16(c.bytes + half + pos, n, b0, b1, b2, b3);
    }
    // low sum in bits 0..15, high sum in bits 16..31, each reduced mod 256 first: 256 lanes * 255 fits its field
    uint32_t v = ((byte_sum(a0) + byte_sum(a1) + byte_sum(a2) + byte_sum(a3)) & 255u) |
                 (((byte_sum(b0) + byte_sum(b1) + byte_sum(b2) + byte_sum(b3)) & 255u) << 16);
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    if ((tid & 63) == 0) wave_sums[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) {
        const uint32_t s = wave_sums[0] + wave_sums[1] + wave_sums[2] + wave_sums[3];
        tile_sums[((size_t)chunk * 2 + 0) * tiles + k] = s & 255u;
        tile_sums[((size_t)chunk * 2 + 1) * tiles + k] = (s >> 16) & 255u;
    }
}

template <int B>                                     // bytes per sample: 2 (half) or 4 (float)
__global__ void __launch_bounds__(THREADS)
exr_unpack_kernel(int W, int H, int C, int max_rows, const uint8_t* __restrict__ inflated, long long inflated_bytes,
                  const int32_t* __restrict__ table, int kept, const int32_t* __restrict__ kept_channels,
                  const uint32_t* __restrict__ tile_sums, void* __restrict__ planes)
{
    __shared__ __attribute__((aligned(16))) uint32_t tile[2 * TILE / 4];              // the 8 KB of raw bytes of this tile pair
    __shared__ uint32_t wave_totals[THREADS / 64], wave_carries[THREADS / 64];
    __shared__ int kept_s[R3DG_EXR_MAX_KEPT];
    const int tiles = gridDim.x, k = blockIdx.x, chunk = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Chunk c = read_chunk(table, chunk, W, H, C, B, max_rows, inflated, inflated_bytes);
    if (!c.ok) return;                                                                // (uniform over the workgroup)
    const uint32_t first_byte = 2u * (uint32_t)k * TILE;                              // of the raw bytes this workgroup produces
    if (first_byte >= c.n) return;
    if (tid < kept) kept_s[tid] = kept_channels[tid];
    uint32_t o0, o1, o2, o3, o4, o5, o6, o7;                                          // the lane's 32 raw bytes
    if (c.raw) {
        const uint32_t pos = first_byte + 32u * tid;
        const int n = pos >= c.n ? 0 : (c.n - pos < 32u ? (int)(c.n - pos) : 32);
        o0 = o1 = o2 = o3 = o4 = o5 = o6 = o7 = 0;
        if (n > 0) load16(c.bytes + pos, n < 16 ? n : 16, o0, o1, o2, o3);
        if (n > 16) load16(c.bytes + pos + 16, n - 16, o4, o5, o6, o7);
    } else {
        const uint32_t half = c.n / 2, pos = (uint32_t)k * TILE + 16u * tid;
        const int n = pos >= half ? 0 : (half - pos < 16u ? (int)(half - pos) : 16);
        uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0, b0 = 0, b1 = 0, b2 = 0, b3 = 0;
        if (n > 0) {
            load16(c.bytes + pos, n, a0, a1, a2, a3);
            load16(c.bytes + half + pos, n, b0, b1, b2, b3);
        }
        // carry-in: the low tile has the low tiles before it in front; the high tile the whole low half and the high tiles before
        // it (tiles past a short chunk's last one hold 0).  Packed as the sums below.
        const uint32_t* sums = tile_sums + (size_t)chunk * 2 * tiles;
        uint32_t carry = 0;
        for (int j = tid; j < tiles; j += THREADS) {
            const uint32_t lo = sums[j], hi = sums[tiles + j];
            carry += (j < k ? lo : 0u) + ((lo + (j < k ? hi : 0u)) << 16);
        }
        carry = (carry & 0x000000ffu) | (carry & 0x00ff0000u);
        for (int d = 32; d >= 1; d >>= 1) carry += __shfl_xor(carry, d);
        // the lane's own totals (mod 256, packed) and their inclusive scan over the wave
        const uint32_t mine = ((byte_sum(a0) + byte_sum(a1) + byte_sum(a2) + byte_sum(a3)) & 255u) |
                              (((byte_sum(b0) + byte_sum(b1) + byte_sum(b2) + byte_sum(b3)) & 255u) << 16);
        uint32_t incl = mine;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        if (lane == 63) wave_totals[wave] = incl;
        if (lane == 0) wave_carries[wave] = carry;
        __syncthreads();
        uint32_t before = wave_carries[0] + wave_carries[1] + wave_carries[2] + wave_carries[3];
        before = ((before & 0x000000ffu) | (before & 0x00ff0000u)) + incl - mine;    // (each field stays below 2^16: 255 + 255 * 255)
        if (wave > 0) before += wave_totals[0];
        if (wave > 1) before += wave_totals[1];
        if (wave > 2) before += wave_totals[2];
        uint32_t run_lo = before & 0xffffu, run_hi = before >> 16;                   // (only their low 8 bits matter)
        const bool hi_odd = (half & 1u) != 0;                                         // index of the lane's first high byte: half + pos
        a0 = scan_word(a0, run_lo, false), a1 = scan_word(a1, run_lo, false);
        a2 = scan_word(a2, run_lo, false), a3 = scan_word(a3, run_lo, false);
        b0 = scan_word(b0, run_hi, hi_odd), b1 = scan_word(b1, run_hi, hi_odd);
        b2 = scan_word(b2, run_hi, hi_odd), b3 = scan_word(b3, run_hi, hi_odd);
        interleave(a0, b0, o0, o1);
        interleave(a1, b1, o2, o3);
        interleave(a2, b2, o4, o5);
        interleave(a3, b3, o6, o7);
    }
    uint4* mine4 = reinterpret_cast<uint4*>(tile + 8 * tid);
    mine4[0] = make_uint4(o0, o1, o2, o3);
    mine4[1] = make_uint4(o4, o5, o6, o7);
    __syncthreads();
    // samples of this tile, lane i: i, i + 256, ...; sample s of the chunk is row s / (W C), channel (s % (W C)) / W, x = s % W
    const uint32_t bytes_here = c.n - first_byte < 2u * TILE ? c.n - first_byte : 2u * TILE;
    const uint32_t count = bytes_here / B, s0 = first_byte / B, WC = (uint32_t)W * (uint32_t)C;
    for (uint32_t sl = tid; sl < count; sl += THREADS) {
        const uint32_t s = s0 + sl, row = s / WC, rem = s - row * WC, ch = rem / (uint32_t)W, x = rem - ch * (uint32_t)W;
        for (int q = 0; q < kept; q++) {
            if (kept_s[q] != (int)ch) continue;
            const size_t at = ((size_t)q * H + (size_t)(c.first_row + (int)row)) * W + x;
            if (B == 2)
                reinterpret_cast<uint16_t*>(planes)[at] = reinterpret_cast<const uint16_t*>(tile)[sl];
            else
                reinterpret_cast<uint32_t*>(planes)[at] = tile[sl];
        }
    }
}

}  // namespace r3dg
