// PNG frames encoded on the device (r3dg_hip.h "r3dg_png_encode") for gfx950: the scanline filter, a deflate stream and the
// Adler-32 in three launches.  Deflate is serial only through its match history and its bit offset; both are cut at row-segment
// boundaries (a segment: the rows that fit 16384 bytes, one row at least), so a segment is an independent unit of work.
//
//   png_segment_kernel   one workgroup of 1024 lanes per segment; the filtered bytes and the packed bits live in LDS.
//                          1. FILTER: teams of waves take a row each (16 one-wave teams down to one team of 16 waves for a one-row
//                             segment): five scores per row (sum |int8|) by wave reductions, the lowest wins (ties: lowest type),
//                             the chosen filter's bytes go to LDS.  The pixel row above is read from the picture, also across a
//                             segment boundary.
//                          2. RUNS: a lane owns a contiguous chunk of 4 * odd bytes (odd dword stride: byte reads of neighbouring
//                             lanes fall into different LDS banks).  The start of the run that enters a chunk is a forward max-scan
//                             of the lanes' last run starts, the end of the run that leaves it a backward min-scan of their first
//                             ones.  With (offset in run, run length) every position knows its token in closed form: no hash
//                             chains, no search.
//                          3. BITS: the lanes' bit counts are scanned once; the total decides coded or stored BEFORE anything is
//                             written.  A lane's tokens are contiguous bits: it shifts them through a 64-bit register and stores
//                             whole words it owns alone; only its first and last partial word are merged with an LDS atomicOr.
//                          4. The segment goes to its fixed slot of the scratch with its byte count and its Adler pair
//                             (sum b, sum (n - i) b) mod 65521.
//   png_offsets_kernel   one workgroup: scans the byte counts into stream offsets, combines the Adler pairs (a closed form in the
//                        segments' raw sizes: a reduction, no serial chain), writes the 2-byte head, `03 00`, the checksum and
//                        the total.
//   png_gather_kernel    one workgroup per segment: slot -> stream, word stores on the destination's alignment.
// No global atomics, nothing synchronises, no byte outside the arrays is touched; the picture is read with byte loads (any alignment).
#include "launchers.hpp"

#include <atomic>

namespace r3dg {

namespace {

constexpr int PNG_THREADS = 1024, PNG_WAVES = PNG_THREADS / 64;
constexpr int PNG_SEGMENT_BYTES = 16384;
constexpr uint32_t ADLER_MOD = 65521;

struct PngShape {
    int row_bytes, rows_per_seg, nseg, seg_raw;    // seg_raw: bytes of a full segment
    long long slot_bytes, meta_offset, offsets_offset, scratch_bytes;
};

PngShape png_shape(int W, int H, int C)
{
    PngShape p;
    p.row_bytes = W * C + 1;
    p.rows_per_seg = std::max(1, std::min(H, PNG_SEGMENT_BYTES / p.row_bytes));
    p.nseg = (H + p.rows_per_seg - 1) / p.rows_per_seg;
    p.seg_raw = p.rows_per_seg * p.row_bytes;
    p.slot_bytes = ((long long)p.seg_raw + 5 + 3 + 15) & ~15ll;         // a segment, coded or stored, and the gather's look-ahead word
    p.meta_offset = p.slot_bytes * p.nseg;
    p.offsets_offset = p.meta_offset + ((12ll * p.nseg + 7) & ~7ll);    // counts, Adler sums A, B: 4 bytes each; then the offsets
    p.scratch_bytes = p.offsets_offset + 8ll * p.nseg;
    return p;
}

struct PngArgs {
    int W, H, C, row_bytes, rows_per_seg, nseg, header_bits;
    long long slot_bytes;
    const uint8_t* bytes;
    const uint32_t* code_table;
    const uint8_t* block_header;
    uint8_t* slots;
    int32_t* counts;
    uint32_t *adler_a, *adler_b;
    long long* offsets;
    uint8_t* zlib;
    int32_t* zlib_bytes;
};

struct OpSum { __device__ static int apply(int a, int b) { return a + b; } };
struct OpMax { __device__ static int apply(int a, int b) { return max(a, b); } };
struct OpMin { __device__ static int apply(int a, int b) { return min(a, b); } };

// Exclusive scan of one int per lane over the workgroup (REVERSE: from the last lane down); `total`: the whole workgroup's.
// s_wave: one int per wave.  Two barriers; s_wave is free again on return.
template <class Op, bool REVERSE>
__device__ int block_scan_exclusive(int v, int identity, int* s_wave, int& total)
{
    const int lane = lane_id(), wave = (int)threadIdx.x >> 6, waves = (int)blockDim.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = REVERSE ? __shfl_down(inc, d, 64) : __shfl_up(inc, d, 64);
        if (REVERSE ? lane + d < 64 : lane >= d) inc = Op::apply(inc, o);
    }
    if (lane == (REVERSE ? 0 : 63)) s_wave[wave] = inc;
    int before = REVERSE ? __shfl_down(inc, 1, 64) : __shfl_up(inc, 1, 64);
    if (lane == (REVERSE ? 63 : 0)) before = identity;
    __syncthreads();
    int pre = identity;
    total = identity;
    for (int w = 0; w < waves; w++) {
        const int t = s_wave[w];
        total = Op::apply(total, t);
        if (REVERSE ? w > wave : w < wave) pre = Op::apply(pre, t);
    }
    __syncthreads();
    return Op::apply(pre, before);
}

__device__ __forceinline__ int wave_sum_int(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// |int8(d)|: the cost of a filtered byte
__device__ __forceinline__ int residual_cost(int d)
{
    d &= 255;
    return d < 128 ? d : 256 - d;
}

__device__ __forceinline__ int paeth_predictor(int a, int b, int c)
{
    const int p = a + b - c;
    const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ uint32_t literal_token(int byte, const uint32_t* code, int& nb)
{
    const uint32_t c = code[byte];
    nb = (int)((c >> 16) & 31);
    return c & 0xFFFFu;
}

// length code, its extra bits, the one distance bit (0: distance 1) of a match of L in 3..258
__device__ __forceinline__ uint32_t match_token(int L, const uint32_t* code, int& nb)
{
    int sym = 285, eb = 0, ev = 0;
    if (L != 258) {
        const int l = L - 3;
        if (l < 8) {
            sym = 257 + l;
        } else {
            eb = 29 - __clz(l);                        // floor(log2 l) - 2
            sym = 261 + 4 * eb + ((l >> eb) & 3);
            ev = l & ((1 << eb) - 1);
        }
    }
    const uint32_t c = code[sym];
    const int len = (int)((c >> 16) & 31);
    nb = len + eb + 1;
    return (c & 0xFFFFu) | ((uint32_t)ev << len);
}

// the token that position k of a run of n bytes `byte` emits (nb = 0: none).  rest = n - 1 bytes follow the literal: m matches of
// 258 while rest >= 261 or rest == 258, then a tail t: 259 / 260 -> (t - 3, 3); 3..257 -> one match; 1, 2 -> literals.
__device__ __forceinline__ uint32_t token_at(int k, int n, int byte, const uint32_t* code, int& nb)
{
    nb = 0;
    if (k == 0) return literal_token(byte, code, nb);
    const int rest = n - 1, r = k - 1;
    int m = 0, t = rest;
    if (rest >= 3) {
        m = (rest - 3) / 258;
        t = rest - 258 * m;
        if (t == 258) m++, t = 0;
    }
    if (r < 258 * m) return r % 258 ? 0u : match_token(258, code, nb);
    const int q = r - 258 * m;
    if (t < 3) return literal_token(byte, code, nb);
    if (t <= 257) return q ? 0u : match_token(t, code, nb);
    if (q == 0) return match_token(t - 3, code, nb);
    if (q == t - 3) return match_token(3, code, nb);
    return 0u;
}

// every token of the chunk [c0, c1) in order: emit(bits, count).  run_start: the start of the run that holds c0 - 1 (the forward
// scan); next_start: the first run start at or after c1 (the backward scan; n when there is none)
template <class F>
__device__ __forceinline__ void walk_chunk(const uint8_t* filt, int c0, int c1, int run_start, int next_start, const uint32_t* code,
                                           F&& emit)
{
    int s = run_start, e = -1;
    int prev = c0 > 0 ? (int)filt[c0 - 1] : -1;
    for (int i = c0; i < c1; i++) {
        const int b = filt[i];
        if (b != prev) s = i;
        prev = b;
        if (e <= i) {                                  // a run this lane has not measured yet: its end is the next run's start
            int j = i + 1;
            while (j < c1 && filt[j] == b) j++;
            e = j < c1 ? j : next_start;
        }
        int nb;
        const uint32_t v = token_at(i - s, e - s, b, code, nb);
        if (nb) emit(v, nb);
    }
}

__global__ void __launch_bounds__(PNG_THREADS)
png_segment_kernel(PngArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    __shared__ uint32_t s_code[286];
    __shared__ int s_wave[PNG_WAVES];
    __shared__ int s_score[2][PNG_WAVES][5];
    const int seg = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row0 = seg * a.rows_per_seg;
    const int rows = min(a.rows_per_seg, a.H - row0);
    const int n = rows * a.row_bytes;                              // 1..65535
    const int region_words = (a.rows_per_seg * a.row_bytes + 5 + 3) >> 2;
    // region: [0,5) the stored block's header, then the filtered bytes -- a stored segment is the region as it stands
    uint8_t* region = lds;
    uint8_t* filt = region + 5;
    uint32_t* out = reinterpret_cast<uint32_t*>(lds) + region_words;        // region_words words: a coded segment of n + 5 bytes at most

    for (int i = tid; i < 286; i += PNG_THREADS) s_code[i] = a.code_table[i];
    for (int i = tid; i < region_words; i += PNG_THREADS) out[i] = 0u;

    // ---- 1. filter ----
    const int WC = a.row_bytes - 1, C = a.C;
    int teams = 1;
    while (teams < rows && teams < PNG_WAVES) teams <<= 1;
    const int team_threads = PNG_THREADS / teams, team_waves = PNG_WAVES / teams;
    const int team = tid / team_threads, tt = tid - team * team_threads;
    const int iters = (rows + teams - 1) / teams;
    for (int it = 0; it < iters; it++) {
        const int r = it * teams + team;
        const bool active = r < rows;
        const int y = row0 + r;
        const bool has_up = y > 0;
        const uint8_t* cur = a.bytes + (size_t)(active ? y : 0) * WC;
        const uint8_t* up = a.bytes + (size_t)(active && has_up ? y - 1 : 0) * WC;
        int sc[5] = {0, 0, 0, 0, 0};
        if (active) {
            for (int x = tt; x < WC; x += team_threads) {
                const int v = cur[x];
                const int pa = x >= C ? (int)cur[x - C] : 0;
                const int pb = has_up ? (int)up[x] : 0;
                const int pc = (has_up && x >= C) ? (int)up[x - C] : 0;
                sc[0] += residual_cost(v);
                sc[1] += residual_cost(v - pa);
                sc[2] += residual_cost(v - pb);
                sc[3] += residual_cost(v - ((pa + pb) >> 1));
                sc[4] += residual_cost(v - paeth_predictor(pa, pb, pc));
            }
        }
#pragma unroll
        for (int k = 0; k < 5; k++) {
            const int t = wave_sum_int(sc[k]);
            if (lane == 0) s_score[it & 1][wave][k] = t;
        }
        __syncthreads();
        if (active) {
            int best = 0, best_score = 0x7fffffff;
#pragma unroll
            for (int k = 0; k < 5; k++) {
                int t = 0;
                for (int w = 0; w < team_waves; w++) t += s_score[it & 1][team * team_waves + w][k];
                if (t < best_score) best_score = t, best = k;
            }
            uint8_t* dst = filt + r * a.row_bytes;
            if (tt == 0) dst[0] = (uint8_t)best;
            for (int x = tt; x < WC; x += team_threads) {
                const int v = cur[x];
                const int pa = x >= C ? (int)cur[x - C] : 0;
                const int pb = has_up ? (int)up[x] : 0;
                int pred = 0;
                if (best == 1) pred = pa;
                else if (best == 2) pred = pb;
                else if (best == 3) pred = (pa + pb) >> 1;
                else if (best == 4) pred = paeth_predictor(pa, pb, (has_up && x >= C) ? (int)up[x - C] : 0);
                dst[1 + x] = (uint8_t)(v - pred);
            }
        }
    }
    __syncthreads();

    // ---- 2. runs ----
    const int chunk = 4 * (((n + 4 * PNG_THREADS - 1) / (4 * PNG_THREADS)) | 1);
    const int c0 = min(tid * chunk, n), c1 = min(c0 + chunk, n);
    int first = n, last = -1;
    uint32_t sum_a = 0, sum_b = 0;
    {
        int prev = c0 > 0 ? (int)filt[c0 - 1] : -1;
        for (int i = c0; i < c1; i++) {
            const int b = filt[i];
            if (b != prev) {
                if (first == n) first = i;
                last = i;
            }
            prev = b;
            sum_a += (uint32_t)b;
            sum_b += (uint32_t)(n - i) * (uint32_t)b;          // at most 68 x 65535 x 255 per lane
        }
    }
    int total;
    const int run_start = block_scan_exclusive<OpMax, false>(last, -1, s_wave, total);
    const int next_start = block_scan_exclusive<OpMin, true>(first, n, s_wave, total);
    int adler_a, adler_b;
    block_scan_exclusive<OpSum, false>((int)sum_a, 0, s_wave, adler_a);
    block_scan_exclusive<OpSum, false>((int)(sum_b % ADLER_MOD), 0, s_wave, adler_b);

    // ---- 3. bits ----
    int my_bits = 0;
    walk_chunk(filt, c0, c1, run_start, next_start, s_code, [&](uint32_t, int nb) { my_bits += nb; });
    int token_bits;
    const int bit0 = a.header_bits + block_scan_exclusive<OpSum, false>(my_bits, 0, s_wave, token_bits);
    const uint32_t eob = s_code[256];
    const int eob_at = a.header_bits + token_bits;
    const int trailer_at = (eob_at + (int)((eob >> 16) & 31) + 3 + 7) >> 3;       // end of block, `000`, zero bits to the byte boundary
    const int coded_bytes = trailer_at + 4;
    const bool stored = coded_bytes > n + 5;
    const int count = stored ? n + 5 : coded_bytes;

    if (stored) {
        if (tid == 0) {
            region[0] = 0;
            region[1] = (uint8_t)n, region[2] = (uint8_t)(n >> 8);
            region[3] = (uint8_t)~n, region[4] = (uint8_t)(~n >> 8);
        }
    } else {
        const int header_bytes = (a.header_bits + 7) >> 3;
        if (tid < header_bytes) {
            uint32_t b = a.block_header[tid];
            if (tid == header_bytes - 1 && (a.header_bits & 7)) b &= (1u << (a.header_bits & 7)) - 1u;
            atomicOr(&out[tid >> 2], b << (8 * (tid & 3)));
        }
        int word = bit0 >> 5, fill = bit0 & 31;
        bool shared_word = fill != 0;                  // the first word is shared with the lanes before unless it starts on a boundary
        unsigned long long acc = 0;
        walk_chunk(filt, c0, c1, run_start, next_start, s_code, [&](uint32_t v, int nb) {
            acc |= (unsigned long long)v << fill;
            fill += nb;
            if (fill >= 32) {
                if (shared_word) atomicOr(&out[word], (uint32_t)acc);
                else out[word] = (uint32_t)acc;
                shared_word = false;
                word++, acc >>= 32, fill -= 32;
            }
        });
        if (fill > 0 && acc) atomicOr(&out[word], (uint32_t)acc);
        if (tid == 0) {
            const unsigned long long e = (unsigned long long)(eob & 0xFFFFu) << (eob_at & 31);
            if ((uint32_t)e) atomicOr(&out[eob_at >> 5], (uint32_t)e);
            if ((uint32_t)(e >> 32)) atomicOr(&out[(eob_at >> 5) + 1], (uint32_t)(e >> 32));
            const int f0 = trailer_at + 2, f1 = trailer_at + 3;                    // 00 00 FF FF
            atomicOr(&out[f0 >> 2], 0xFFu << (8 * (f0 & 3)));
            atomicOr(&out[f1 >> 2], 0xFFu << (8 * (f1 & 3)));
        }
    }
    __syncthreads();

    // ---- 4. the slot ----
    const uint32_t* src = stored ? reinterpret_cast<const uint32_t*>(region) : out;
    uint32_t* slot = reinterpret_cast<uint32_t*>(a.slots + (size_t)seg * a.slot_bytes);
    const int words = (count + 3) >> 2;
    for (int i = tid; i < words; i += PNG_THREADS) slot[i] = src[i];
    if (tid == 0) {
        a.counts[seg] = count;
        a.adler_a[seg] = (uint32_t)adler_a % ADLER_MOD;
        a.adler_b[seg] = (uint32_t)adler_b % ADLER_MOD;
    }
}

__global__ void __launch_bounds__(PNG_THREADS)
png_offsets_kernel(PngArgs a)
{
    __shared__ int s_wave[PNG_WAVES];
    const int tid = (int)threadIdx.x;
    const long long N = (long long)a.H * a.row_bytes;
    long long running = 2;                                     // 78 01
    unsigned long long acc_a = 0, acc_b = 0;
    for (int base = 0; base < a.nseg; base += PNG_THREADS) {
        const int k = base + tid;
        const bool live = k < a.nseg;
        int total;
        const int before = block_scan_exclusive<OpSum, false>(live ? a.counts[k] : 0, 0, s_wave, total);
        if (live) {
            a.offsets[k] = running + before;
            // byte i of segment k weighs (n_k - i) + (the bytes behind the segment) in the stream's second sum
            const long long end = min((long long)(k + 1) * a.rows_per_seg, (long long)a.H) * a.row_bytes;
            const unsigned long long behind = (unsigned long long)((N - end) % ADLER_MOD);
            acc_a = (acc_a + a.adler_a[k]) % ADLER_MOD;
            acc_b = (acc_b + a.adler_b[k] + (unsigned long long)a.adler_a[k] * behind) % ADLER_MOD;
        }
        running += total;
    }
    int sum_a, sum_b;
    block_scan_exclusive<OpSum, false>((int)acc_a, 0, s_wave, sum_a);
    block_scan_exclusive<OpSum, false>((int)acc_b, 0, s_wave, sum_b);
    if (tid == 0) {
        const uint32_t s1 = (1u + (uint32_t)sum_a) % ADLER_MOD;
        const uint32_t s2 = (uint32_t)(((unsigned long long)(N % ADLER_MOD) + (unsigned long long)sum_b) % ADLER_MOD);
        uint8_t* z = a.zlib;
        z[0] = 0x78, z[1] = 0x01;
        z[running] = 0x03, z[running + 1] = 0x00;              // a final, empty fixed-code block
        z[running + 2] = (uint8_t)(s2 >> 8), z[running + 3] = (uint8_t)s2;
        z[running + 4] = (uint8_t)(s1 >> 8), z[running + 5] = (uint8_t)s1;
        *a.zlib_bytes = (int32_t)(running + 6);
    }
}

__global__ void __launch_bounds__(256)
png_gather_kernel(PngArgs a)
{
    const int seg = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int count = a.counts[seg];
    const uint8_t* src = a.slots + (size_t)seg * a.slot_bytes;
    uint8_t* dst = a.zlib + a.offsets[seg];
    const int head = min(count, (int)((4 - ((size_t)dst & 3)) & 3));          // bytes up to the destination's word boundary
    if (tid < head) dst[tid] = src[tid];
    const int words = (count - head) >> 2;
    const uint32_t* sw = reinterpret_cast<const uint32_t*>(src);             // (the slot is 16-byte aligned and ends a word behind the count)
    uint32_t* dw = reinterpret_cast<uint32_t*>(dst + head);
    const int shift = 8 * head;
    for (int j = tid; j < words; j += 256) {
        const unsigned long long pair = (unsigned long long)sw[j] | ((unsigned long long)sw[j + 1] << 32);
        dw[j] = (uint32_t)(pair >> shift);
    }
    const int done = head + 4 * words;
    if (tid < count - done) dst[done + tid] = src[done + tid];
}

}  // namespace

long long png_zlib_bound(int W, int H, int C)
{
    const PngShape p = png_shape(W, H, C);
    return 2 + (long long)H * p.row_bytes + 5ll * p.nseg + 6;
}

long long png_scratch_bytes(int W, int H, int C) { return png_shape(W, H, C).scratch_bytes; }

void launch_png_encode(hipStream_t s, int W, int H, int C, const uint8_t* bytes, const uint32_t* code_table,
                       const uint8_t* block_header, int header_bits, uint8_t* scratch, uint8_t* zlib, int32_t* zlib_bytes)
{
    const PngShape p = png_shape(W, H, C);
    PngArgs a = {};
    a.W = W, a.H = H, a.C = C, a.row_bytes = p.row_bytes, a.rows_per_seg = p.rows_per_seg, a.nseg = p.nseg;
    a.header_bits = header_bits, a.slot_bytes = p.slot_bytes;
    a.bytes = bytes, a.code_table = code_table, a.block_header = block_header;
    a.slots = scratch;
    a.counts = reinterpret_cast<int32_t*>(scratch + p.meta_offset);
    a.adler_a = reinterpret_cast<uint32_t*>(a.counts + p.nseg);
    a.adler_b = a.adler_a + p.nseg;
    a.offsets = reinterpret_cast<long long*>(scratch + p.offsets_offset);
    a.zlib = zlib, a.zlib_bytes = zlib_bytes;
    const size_t smem = 2 * (size_t)((p.seg_raw + 5 + 3) >> 2) * 4;            // the region and the packed bits
    // above 64 KB (a row of more than ~32 000 bytes) the kernel needs the per-device function attribute, asked for once
    if (smem + 4096 > 65536) {
        static std::atomic<unsigned long long> done{0};
        int dev = 0;
        R3DG_HIP(hipGetDevice(&dev));
        const unsigned long long bit = 1ull << (dev & 63);
        if (!(done.load(std::memory_order_acquire) & bit)) {
            R3DG_HIP(hipFuncSetAttribute((const void*)png_segment_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         2 * ((65535 + 5 + 3) >> 2) * 4));
            done.fetch_or(bit, std::memory_order_release);
        }
    }
    png_segment_kernel<<<p.nseg, PNG_THREADS, smem, s>>>(a);
    check_launch(s, false, "png_segment_kernel");
    png_offsets_kernel<<<1, PNG_THREADS, 0, s>>>(a);
    check_launch(s, false, "png_offsets_kernel");
    png_gather_kernel<<<p.nseg, 256, 0, s>>>(a);
    check_launch(s, false, "png_gather_kernel");
}

}  // namespace r3dg
