// Scene assembly for gfx950 (r3dg_hip.h "scene assembly"): the rows of a reference PLY (scene/gaussian_model.py:507-665) and the
// 13 coefficient-major parameter groups of a model, converted into each other and placed into a composite
// (relighting.py:28-52, GaussianModel.set_transform :84-95) in ONE launch per object.
//
//   scene_tile_kernel<FROM_RECORDS, TO_RECORDS>   one workgroup = one tile of 64 rows:
//       1. stage in    records: the tile's 64 x A floats are ONE contiguous span, read flat (lane = consecutive float) into LDS
//                      rows of stride A | 1; groups: every group's 64 x w floats likewise, scattered to the canonical slot.
//       2. place       (optional) thread = row: the 13 transformed scalars, in LDS.  thread = (row, SH vector): bands 1..3 of the
//                      7 SH vectors times the object's 3x3 / 5x5 / 7x7 rotation matrices, in LDS.
//       3. stage out   groups: per group a flat span of 64 x w floats at the row offset (lane = consecutive destination float),
//                      gathered from LDS through the column map with the channel-major -> coefficient-major transpose;
//                      records: the tile's 64 x columns floats flat.
//   A 520-byte row is no multiple of a cache line; a thread per row would touch 64 lines per wave access.  With the odd LDS
//   stride, lanes that read one column of consecutive rows fall on 64 different banks.
//   No atomics; the only per-thread arrays (15 coefficients in, 15 out) are indexed by unrolled constants: no scratch memory.
//
//   relight_quantize_kernel   [C,H,W] float -> [H,W,C] uint8 as torchvision's save_image rounds (thread = output byte).
#include "glue_math.hpp"
#include "launchers.hpp"

namespace r3dg {

namespace {

constexpr int kRows = 64, kThreads = 256, kCols = R3DG_SCENE_COLUMNS, kGroups = R3DG_SCENE_GROUPS;
constexpr int kStageBatch = 4;      // loads in flight per thread while staging in

// first canonical slot and floats per row of every group; the two [P,15,3] groups are channel-major in a record
__device__ __forceinline__ constexpr int group_slot(int g)
{
    constexpr int s[kGroups] = {0, 3, 6, 9, 54, 55, 58, 62, 65, 66, 69, 114, 115};
    return s[g];
}
__device__ __forceinline__ constexpr int group_width(int g)
{
    constexpr int w[kGroups] = {3, 3, 3, 45, 1, 3, 4, 3, 1, 3, 45, 1, 15};
    return w[g];
}
template <int G>
__device__ __forceinline__ int slot_of(int e)
{
    if (G == 3 || G == 10) return group_slot(G) + (e % 3) * 15 + e / 3;
    return group_slot(G) + e;
}

struct SceneArgs {
    int P, A, flags, out_cols;
    long long row_offset;
    const float* records_in;
    const int* column_map;
    const float* placement;
    float* records_out;
    SceneGroups src, dst;
};

struct Tile {
    float* rows;
    const int* map;     // canonical slot -> column of the staged row (-1: absent)
    int stride;
    __device__ __forceinline__ float ld(int r, int slot) const
    {
        const int c = map[slot];
        return c >= 0 ? rows[r * stride + c] : 0.f;
    }
    __device__ __forceinline__ void st(int r, int slot, float v) const
    {
        const int c = map[slot];
        if (c >= 0) rows[r * stride + c] = v;
    }
};

// n floats of src (flat, row length A) -> LDS rows of `stride`; A_ > 0: the row length as a compile-time constant
template <int A_>
__device__ __forceinline__ void stage_records_in(const float* __restrict__ src, int n, int A, int stride, float* rows)
{
    const int a = A_ > 0 ? A_ : A;
    for (int f0 = threadIdx.x; f0 < n; f0 += kThreads * kStageBatch) {
        float v[kStageBatch];
#pragma unroll
        for (int j = 0; j < kStageBatch; j++) v[j] = src[min(f0 + j * kThreads, n - 1)];
#pragma unroll
        for (int j = 0; j < kStageBatch; j++) {
            const int f = f0 + j * kThreads;
            if (f < n) {
                const int r = f / a;
                rows[r * stride + (f - r * a)] = v[j];
            }
        }
    }
}
template <int COLS>
__device__ __forceinline__ void stage_records_out(float* __restrict__ dst, int n, int stride, const float* rows)
{
    for (int f = threadIdx.x; f < n; f += kThreads) {
        const int r = f / COLS;
        dst[f] = rows[r * stride + (f - r * COLS)];
    }
}

template <int G>
__device__ __forceinline__ void stage_group_in(const SceneGroups& src, size_t row0, int nrows, const Tile& t)
{
    constexpr int w = group_width(G);
    const float* __restrict__ g = src.p[G];
    const int n = nrows * w;
    for (int j = threadIdx.x; j < n; j += kThreads) {
        const int r = j / w;
        t.rows[r * t.stride + slot_of<G>(j - r * w)] = g != nullptr ? g[row0 * w + j] : 0.f;
    }
}
template <int G>
__device__ __forceinline__ void stage_group_out(const SceneGroups& dst, size_t row0, int nrows, const Tile& t, bool zero)
{
    constexpr int w = group_width(G);
    float* __restrict__ g = dst.p[G];
    const int n = nrows * w;
    for (int j = threadIdx.x; j < n; j += kThreads) {
        const int r = j / w;
        g[row0 * w + j] = zero ? 0.f : t.ld(r, slot_of<G>(j - r * w));
    }
}

// c'_l = M_l c_l for the 15 coefficients of bands 1..3 that start at canonical slot `base`; pl = the placement block in LDS
__device__ __forceinline__ void rotate_sh_vector(const Tile& t, int r, int base, const float* pl)
{
    float c[15], o[15];
#pragma unroll
    for (int i = 0; i < 15; i++) c[i] = t.ld(r, base + i);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 3; j++) s = fmaf(pl[28 + i * 3 + j], c[j], s);
        o[i] = s;
    }
#pragma unroll
    for (int i = 0; i < 5; i++) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 5; j++) s = fmaf(pl[37 + i * 5 + j], c[3 + j], s);
        o[3 + i] = s;
    }
#pragma unroll
    for (int i = 0; i < 7; i++) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 7; j++) s = fmaf(pl[62 + i * 7 + j], c[8 + j], s);
        o[8 + i] = s;
    }
#pragma unroll
    for (int i = 0; i < 15; i++) t.st(r, base + i, o[i]);
}

// relight.transform_object on one staged row: xyz = T (x,1), scaling = log(exp(s) * scale), normal = R n, rotation = q * rot
__device__ __forceinline__ void place_row(const Tile& t, int r, const float* pl)
{
    const float x = t.ld(r, 0), y = t.ld(r, 1), z = t.ld(r, 2);
    const float nx = t.ld(r, 3), ny = t.ld(r, 4), nz = t.ld(r, 5);
    const float w2 = t.ld(r, 58), x2 = t.ld(r, 59), y2 = t.ld(r, 60), z2 = t.ld(r, 61);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        t.st(r, k, fmaf(x, pl[4 * k], fmaf(y, pl[4 * k + 1], fmaf(z, pl[4 * k + 2], pl[4 * k + 3]))));
        t.st(r, 3 + k, fmaf(nx, pl[15 + 3 * k], fmaf(ny, pl[16 + 3 * k], nz * pl[17 + 3 * k])));
        t.st(r, 55 + k, logf(expf(t.ld(r, 55 + k)) * pl[12 + k]));
    }
    const float w1 = pl[24], x1 = pl[25], y1 = pl[26], z1 = pl[27];          // Hamilton product (utils/general_utils.py:141-151)
    t.st(r, 58, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2);
    t.st(r, 59, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2);
    t.st(r, 60, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2);
    t.st(r, 61, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2);
}

template <bool FROM_RECORDS, bool TO_RECORDS>
__global__ void __launch_bounds__(kThreads) scene_tile_kernel(SceneArgs a)
{
    extern __shared__ float s_rows[];
    __shared__ int s_map[kCols];
    __shared__ float s_place[R3DG_SCENE_PLACEMENT_FLOATS];
    const int tid = threadIdx.x;
    const size_t row0 = (size_t)blockIdx.x * kRows;
    const int nrows = (int)min((size_t)kRows, (size_t)a.P - row0);
    const Tile t = {s_rows, s_map, FROM_RECORDS ? (a.A | 1) : (kCols | 1)};
    const bool placed = a.placement != nullptr;
    if (tid < kCols) {
        const int m = FROM_RECORDS ? a.column_map[tid] : tid;
        s_map[tid] = m < (FROM_RECORDS ? a.A : kCols) ? m : -1;      // (a column past the row is absent, never read)
    }
    if (placed && tid < R3DG_SCENE_PLACEMENT_FLOATS) s_place[tid] = a.placement[tid];

    if (FROM_RECORDS) {
        const float* __restrict__ src = a.records_in + row0 * (size_t)a.A;
        const int n = nrows * a.A;
        if (a.A == kCols) stage_records_in<kCols>(src, n, a.A, t.stride, s_rows);
        else if (a.A == R3DG_SCENE_STAGE1_COLUMNS) stage_records_in<R3DG_SCENE_STAGE1_COLUMNS>(src, n, a.A, t.stride, s_rows);
        else stage_records_in<0>(src, n, a.A, t.stride, s_rows);
    } else {
        stage_group_in<0>(a.src, row0, nrows, t);
        stage_group_in<1>(a.src, row0, nrows, t);
        stage_group_in<2>(a.src, row0, nrows, t);
        stage_group_in<3>(a.src, row0, nrows, t);
        stage_group_in<4>(a.src, row0, nrows, t);
        stage_group_in<5>(a.src, row0, nrows, t);
        stage_group_in<6>(a.src, row0, nrows, t);
        if (!TO_RECORDS || a.out_cols == kCols) {
            stage_group_in<7>(a.src, row0, nrows, t);
            stage_group_in<8>(a.src, row0, nrows, t);
            stage_group_in<9>(a.src, row0, nrows, t);
            stage_group_in<10>(a.src, row0, nrows, t);
            stage_group_in<11>(a.src, row0, nrows, t);
            stage_group_in<12>(a.src, row0, nrows, t);
        }
    }
    __syncthreads();

    const bool zero_incidents = (a.flags & R3DG_SCENE_ZERO_INCIDENTS) != 0;
    if (!TO_RECORDS && placed) {
        if (tid < nrows) place_row(t, tid, s_place);                 // (slots 0..5, 55..61: none of them an SH slot)
        if (a.flags & R3DG_SCENE_ROTATE_SH) {
            for (int task = tid; task < 7 * kRows; task += kThreads) {
                const int vec = task / kRows, r = task - vec * kRows;      // (one vector per wave, lane = row)
                if (r >= nrows || (zero_incidents && vec >= 3 && vec < 6)) continue;
                rotate_sh_vector(t, r, vec < 3 ? 9 + 15 * vec : vec < 6 ? 69 + 15 * (vec - 3) : 115, s_place);
            }
        }
        __syncthreads();
    }

    if (TO_RECORDS) {
        float* __restrict__ dst = a.records_out + row0 * (size_t)a.out_cols;
        if (a.out_cols == kCols) stage_records_out<kCols>(dst, nrows * kCols, t.stride, s_rows);
        else stage_records_out<R3DG_SCENE_STAGE1_COLUMNS>(dst, nrows * R3DG_SCENE_STAGE1_COLUMNS, t.stride, s_rows);
    } else {
        const size_t out0 = (size_t)a.row_offset + row0;
        stage_group_out<0>(a.dst, out0, nrows, t, false);
        stage_group_out<1>(a.dst, out0, nrows, t, false);
        stage_group_out<2>(a.dst, out0, nrows, t, false);
        stage_group_out<3>(a.dst, out0, nrows, t, false);
        stage_group_out<4>(a.dst, out0, nrows, t, false);
        stage_group_out<5>(a.dst, out0, nrows, t, false);
        stage_group_out<6>(a.dst, out0, nrows, t, false);
        stage_group_out<7>(a.dst, out0, nrows, t, false);
        stage_group_out<8>(a.dst, out0, nrows, t, false);
        stage_group_out<9>(a.dst, out0, nrows, t, zero_incidents);
        stage_group_out<10>(a.dst, out0, nrows, t, zero_incidents);
        stage_group_out<11>(a.dst, out0, nrows, t, false);
        stage_group_out<12>(a.dst, out0, nrows, t, false);
    }
}

__global__ void __launch_bounds__(256)
relight_quantize_kernel(size_t HW, int C, const float* __restrict__ image, uint8_t* __restrict__ bytes)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= HW * (size_t)C) return;
    const size_t pix = i / (size_t)C;
    const int c = (int)(i - pix * (size_t)C);
    bytes[i] = quantize_byte(image[(size_t)c * HW + pix]);
}

template <bool FROM_RECORDS, bool TO_RECORDS>
void launch_tiles(hipStream_t s, const SceneArgs& a, const char* what)
{
    const int stride = FROM_RECORDS ? (a.A | 1) : (kCols | 1);
    const unsigned blocks = (unsigned)(((size_t)a.P + kRows - 1) / kRows);
    scene_tile_kernel<FROM_RECORDS, TO_RECORDS><<<blocks, kThreads, (size_t)kRows * stride * sizeof(float), s>>>(a);
    check_launch(s, false, what);
}

}  // namespace

void launch_scene_place_records(hipStream_t s, int P, int A, const float* records, const int* column_map, const float* placement,
                                int flags, long long row_offset, const SceneGroups& dst)
{
    SceneArgs a = {};
    a.P = P, a.A = A, a.flags = flags, a.row_offset = row_offset;
    a.records_in = records, a.column_map = column_map, a.placement = placement, a.dst = dst;
    launch_tiles<true, false>(s, a, "scene_place_records");
}

void launch_scene_place_groups(hipStream_t s, int P, const SceneGroups& src, const float* placement, int flags,
                               long long row_offset, const SceneGroups& dst)
{
    SceneArgs a = {};
    a.P = P, a.A = kCols, a.flags = flags, a.row_offset = row_offset;
    a.placement = placement, a.src = src, a.dst = dst;
    launch_tiles<false, false>(s, a, "scene_place_groups");
}

void launch_scene_pack_records(hipStream_t s, int P, int columns, const SceneGroups& src, float* records)
{
    SceneArgs a = {};
    a.P = P, a.A = kCols, a.out_cols = columns;
    a.src = src, a.records_out = records;
    launch_tiles<false, true>(s, a, "scene_pack_records");
}

void launch_relight_quantize(hipStream_t s, int W, int H, int C, const float* image, uint8_t* bytes)
{
    const size_t HW = (size_t)W * H, n = HW * C;
    relight_quantize_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(HW, C, image, bytes);
    check_launch(s, false, "relight_quantize_kernel");
}

}  // namespace r3dg
