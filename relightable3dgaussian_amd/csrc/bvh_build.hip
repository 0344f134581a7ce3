// LBVH build (K17) for gfx950.
// Reference semantics: construct_bvh bvh/src/construct.cu:147-265 (Morton codes of leaf-box centroids, stable sort,
// Karras ranges/splits, bottom-up box merge + leaf counts).  The tree is traversed by bvh_trace.hip.
//
// Compiled with -ffp-contract=off: Morton codes decide the (integer) tree topology and must equal the oracle's.
// Differences from the reference's thrust pipeline:
//   * the 30-bit Morton keys are sorted by this library's own stable LSD radix sort (3 passes of 10 bits);
//   * the bottom-up merge publishes each child box with an agent-scope release before the arrival flag and the
//     second arriver acquires before reading its sibling's box -- gfx950's per-XCD L2s are not coherent, so the
//     reference's fence-free atomicCAS hand-off (construct.cu:243-258) would read stale boxes here.
#include "launchers.hpp"

namespace r3dg {

struct Box {
    float lo[3], hi[3];
};

__device__ __forceinline__ uint32_t expand_bits(uint32_t v)
{
    v = (v * 0x00010001u) & 0xFF0000FFu;
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}
__device__ __forceinline__ int common_upper_bits(uint64_t a, uint64_t b) { return __clzll((long long)(a ^ b)); }

// ---- whole-scene box: per-block partials then one small block ----
__global__ void __launch_bounds__(256) whole_box_partial_kernel(int P, const float* __restrict__ leaf, float* __restrict__ partial)
{
    __shared__ float s[4][6];
    float b[6] = {100000.f, 100000.f, 100000.f, -100000.f, -100000.f, -100000.f};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < P; i += gridDim.x * 256) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            b[a] = fminf(b[a], leaf[6 * (size_t)i + a]);
            b[3 + a] = fmaxf(b[3 + a], leaf[6 * (size_t)i + 3 + a]);
        }
    }
#pragma unroll
    for (int a = 0; a < 6; a++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float n = __shfl_xor(b[a], o, 64);
            b[a] = a < 3 ? fminf(b[a], n) : fmaxf(b[a], n);
        }
    }
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int a = 0; a < 6; a++) s[threadIdx.x >> 6][a] = b[a];
    __syncthreads();
    if (threadIdx.x < 6) {
        const int a = threadIdx.x;
        float v = s[0][a];
        for (int w = 1; w < 4; w++) v = a < 3 ? fminf(v, s[w][a]) : fmaxf(v, s[w][a]);
        partial[blockIdx.x * 6 + a] = v;
    }
}
__global__ void whole_box_final_kernel(int nb, const float* __restrict__ partial, float* __restrict__ whole)
{
    const int a = threadIdx.x;
    if (a >= 6) return;
    float v = a < 3 ? 100000.f : -100000.f;
    for (int i = 0; i < nb; i++) v = a < 3 ? fminf(v, partial[i * 6 + a]) : fmaxf(v, partial[i * 6 + a]);
    whole[a] = v;
}

// Morton code of the leaf-box centroid (construct.cu:23-51); also copies the unsorted boxes aside
__global__ void __launch_bounds__(256)
morton_kernel(int P, const float* __restrict__ leaf, const float* __restrict__ whole, uint64_t* __restrict__ keys,
              uint32_t* __restrict__ vals, float* __restrict__ leaf_copy)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    float c[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float lo = leaf[6 * (size_t)i + a], hi = leaf[6 * (size_t)i + 3 + a];
        leaf_copy[6 * (size_t)i + a] = lo;
        leaf_copy[6 * (size_t)i + 3 + a] = hi;
        float p = (float)((hi + lo) * 0.5);
        p -= whole[a];
        p /= (whole[3 + a] - whole[a]);
        c[a] = fminf(fmaxf(p * 1024.0f, 0.0f), 1024.0f - 1.0f);
    }
    const uint32_t m = expand_bits((uint32_t)c[0]) * 4 + expand_bits((uint32_t)c[1]) * 2 + expand_bits((uint32_t)c[2]);
    keys[i] = (uint64_t)m;
    vals[i] = (uint32_t)i;
}

// sorted order -> leaf rows of aabbs, 64-bit codes (m << 31 | original index, sic), leaf object ids
__global__ void __launch_bounds__(256)
scatter_leaves_kernel(int P, const uint64_t* __restrict__ keys_sorted, const uint32_t* __restrict__ idx_sorted,
                      const float* __restrict__ leaf_copy, float* __restrict__ aabbs, int32_t* __restrict__ nodes,
                      uint64_t* __restrict__ morton)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= P) return;
    const uint32_t src = idx_sorted[j];
    const size_t row = (size_t)(P - 1 + j);
#pragma unroll
    for (int a = 0; a < 6; a++) aabbs[6 * row + a] = leaf_copy[6 * (size_t)src + a];
    morton[j] = (keys_sorted[j] << 31) | (uint64_t)src;
    nodes[5 * row + 3] = (int32_t)src;
}

// Karras internal nodes (construct.cu:54-145, 203-229)
__global__ void __launch_bounds__(256)
internal_nodes_kernel(int P, const uint64_t* __restrict__ code, int32_t* __restrict__ nodes, int2* __restrict__ ranges,
                      int* __restrict__ nonzero_count_seen)
{
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= P - 1) return;
    const int num_leaves = P;
    int first, last;
    if (idx == 0) {
        first = 0;
        last = num_leaves - 1;
    } else {
        const uint64_t self = code[idx];
        const int L_delta = common_upper_bits(self, code[idx - 1]);
        const int R_delta = common_upper_bits(self, code[idx + 1]);
        const int d = (R_delta > L_delta) ? 1 : -1;
        const int delta_min = min(L_delta, R_delta);
        int l_max = 2;
        int delta = -1;
        int i_tmp = idx + d * l_max;
        if (0 <= i_tmp && i_tmp < num_leaves) delta = common_upper_bits(self, code[i_tmp]);
        while (delta > delta_min) {
            l_max <<= 1;
            i_tmp = idx + d * l_max;
            delta = -1;
            if (0 <= i_tmp && i_tmp < num_leaves) delta = common_upper_bits(self, code[i_tmp]);
        }
        int l = 0;
        int t = l_max >> 1;
        while (t > 0) {
            i_tmp = idx + (l + t) * d;
            delta = -1;
            if (0 <= i_tmp && i_tmp < num_leaves) delta = common_upper_bits(self, code[i_tmp]);
            if (delta > delta_min) l += t;
            t >>= 1;
        }
        const int jdx = idx + l * d;
        first = min(idx, jdx);
        last = max(idx, jdx);
    }
    // find_split
    int split;
    {
        const uint64_t first_code = code[first], last_code = code[last];
        if (first_code == last_code) {
            split = (first + last) >> 1;
        } else {
            const int delta_node = common_upper_bits(first_code, last_code);
            split = first;
            int stride = last - first;
            do {
                stride = (stride + 1) >> 1;
                const int middle = split + stride;
                if (middle < last) {
                    const int delta = common_upper_bits(first_code, code[middle]);
                    if (delta > delta_node) split = middle;
                }
            } while (stride > 1);
        }
    }
    int left = split, right = split + 1;
    if (first == split) left += P - 1;
    if (last == split + 1) right += P - 1;
    int32_t* node = nodes + 5 * (size_t)idx;
    node[1] = left;
    node[2] = right;
    node[3] = -1;
    nodes[5 * (size_t)left] = idx;
    nodes[5 * (size_t)right] = idx;
    ranges[idx] = make_int2(first, last);                  // the leaves below this node (range_boxes_kernel)
    if (node[4] != 0) atomicOr(nonzero_count_seen, 1);     // caller-initialised leaf counter (bvh/__init__.py:29-57 puts 0)
}

// bottom-up merge (construct.cu:231-264) with explicit release/acquire around the arrival flag
__global__ void __launch_bounds__(256)
merge_boxes_kernel(int P, int32_t* __restrict__ nodes, float* __restrict__ aabbs, int* __restrict__ flags,
                   const int* __restrict__ nonzero_count_seen)
{
    // (only for a node table whose internal leaf counters were not zero on entry: the counters then depend on the walk)
    if (nonzero_count_seen != nullptr && *nonzero_count_seen == 0) return;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= P) return;
    int idx = P - 1 + j;
    int num = 1;
    int parent = nodes[5 * (size_t)idx];
    while (parent != -1) {
        __threadfence();                                        // release my (or the leaf's) box before arriving
        atomicAdd(&nodes[5 * (size_t)parent + 4], num);
        const int old = atomicCAS(&flags[parent], 0, 1);
        if (old == 0) return;                                   // first arrival: the sibling finishes this node
        __threadfence();                                        // acquire the sibling's box
        const int lidx = nodes[5 * (size_t)parent + 1], ridx = nodes[5 * (size_t)parent + 2];
        volatile const float* lb = aabbs + 6 * (size_t)lidx;
        volatile const float* rb = aabbs + 6 * (size_t)ridx;
        float m[6];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            m[a] = fminf(lb[a], rb[a]);
            m[3 + a] = fmaxf(lb[3 + a], rb[3 + a]);
        }
#pragma unroll
        for (int a = 0; a < 6; a++) aabbs[6 * (size_t)parent + a] = m[a];
        num = atomicAdd(&nodes[5 * (size_t)parent + 4], 0);
        idx = parent;
        parent = nodes[5 * (size_t)parent];
    }
}

// ---- boxes of the internal nodes without inter-thread synchronisation ----------------------------------------------------------
// The reference walks up from every leaf; the second thread to arrive at a node merges its children's boxes
// (construct.cu:231-264).  That needs a release/acquire pair per level and thread, and on this part a device-scope fence is
// an L2 write-back + invalidate across the 8 XCDs: merge_boxes_kernel above spends 2.06 ms on 300k leaves, 93 % of it
// waiting.  But the box of a node is just min / max over the leaves of its RANGE [first, last] (Karras ranges are
// contiguous in Morton order), and min / max give the same bits in any order.  So: boxes of aligned runs of 256 leaves and
// of 256 such runs (two tiny tables), then every internal node reduces its range from at most 2 x 255 leaves + 2 x 255 runs
// + the super-runs between them -- independent threads, no atomics, no fences.  The leaf counter of the node table
// (column 4: the reference adds the children's counters into whatever the caller put there) is last - first + 1 when the
// caller's internal rows hold 0 as the reference's own RayTracer prepares them; any other initial content is detected on
// the device and routed through the reference-shaped walk.
constexpr int BOX_RUN = 256;

__device__ __forceinline__ void box_include(float (&b)[6], const float* __restrict__ o)
{
#pragma unroll
    for (int a = 0; a < 3; a++) {
        b[a] = fminf(b[a], o[a]);
        b[3 + a] = fmaxf(b[3 + a], o[3 + a]);
    }
}

// level 0 -> 1: one thread per run of 256 consecutive boxes (n boxes in, ceil(n/256) out)
__global__ void __launch_bounds__(256)
run_boxes_kernel(int n, const float* __restrict__ in, float* __restrict__ out)
{
    __shared__ float s_b[4][6];
    const int run = blockIdx.x, i = run * BOX_RUN + threadIdx.x;
    float b[6] = {3.0e38f, 3.0e38f, 3.0e38f, -3.0e38f, -3.0e38f, -3.0e38f};
    if (i < n) box_include(b, in + 6 * (size_t)i);
#pragma unroll
    for (int a = 0; a < 6; a++) {
        float v = b[a];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float w = __shfl_xor(v, o, 64);
            v = a < 3 ? fminf(v, w) : fmaxf(v, w);
        }
        if ((threadIdx.x & 63) == 0) s_b[threadIdx.x >> 6][a] = v;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int a = threadIdx.x;
        const float v0 = s_b[0][a], v1 = s_b[1][a], v2 = s_b[2][a], v3 = s_b[3][a];
        out[6 * (size_t)run + a] = a < 3 ? fminf(fminf(v0, v1), fminf(v2, v3)) : fmaxf(fmaxf(v0, v1), fmaxf(v2, v3));
    }
}

__global__ void __launch_bounds__(256)
range_boxes_kernel(int P, const int2* __restrict__ ranges, const float* __restrict__ leaf /* Morton order */,
                   const float* __restrict__ run1, const float* __restrict__ run2, const int* __restrict__ nonzero_count_seen,
                   int32_t* __restrict__ nodes, float* __restrict__ aabbs)
{
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= P - 1) return;
    const int2 r = ranges[idx];
    int i = r.x;
    const int last = r.y;
    float b[6] = {3.0e38f, 3.0e38f, 3.0e38f, -3.0e38f, -3.0e38f, -3.0e38f};
    // leaves up to the next run boundary, whole runs up to the next super-run boundary, whole super-runs, and down again
    while (i <= last && (i % BOX_RUN) != 0) { box_include(b, leaf + 6 * (size_t)i); i++; }
    while (i + BOX_RUN - 1 <= last && ((i / BOX_RUN) % BOX_RUN) != 0) { box_include(b, run1 + 6 * (size_t)(i / BOX_RUN)); i += BOX_RUN; }
    while (i + BOX_RUN * BOX_RUN - 1 <= last) { box_include(b, run2 + 6 * (size_t)(i / (BOX_RUN * BOX_RUN))); i += BOX_RUN * BOX_RUN; }
    while (i + BOX_RUN - 1 <= last) { box_include(b, run1 + 6 * (size_t)(i / BOX_RUN)); i += BOX_RUN; }
    while (i <= last) { box_include(b, leaf + 6 * (size_t)i); i++; }
#pragma unroll
    for (int a = 0; a < 6; a++) aabbs[6 * (size_t)idx + a] = b[a];
    if (*nonzero_count_seen == 0) nodes[5 * (size_t)idx + 4] = last - r.x + 1;
}

// ---- leaf preparation: what the host side of RayTracer does in ~40 PyTorch launches before the build, in one ----------------------
// One thread per Gaussian: the node-table initialisation and the leaf boxes of bvh.leaf_boxes (bvh/__init__.py:29-57) and the
// inverse covariance of train_step.inverse_covariance (gaussian_model.py:257-260).
// BIT-EXACT (with -ffp-contract=off): nodes and aabbs.  Every product, sum, division and square root below is the one PyTorch
// operation bvh.build_rotation / bvh.leaf_boxes run at that place, in their order: the quaternion is divided by
// sqrt(((r0 r0 + r1 r1) + r2 r2) + r3 r3), the matrix entries are 1 - 2 (a + b) and 2 (a -+ b), a corner is
// ((mean + (+-R[:,0]) (3 s0)) + (+-R[:,1]) (3 s1)) + (+-R[:,2]) (3 s2) -- a sign commutes with a product exactly -- and min / max
// give the same bits in any order.  The Morton codes and the tree built from these boxes are then those of RayTracer(...).
// NOT bit-exact: the inverse covariance R diag(1/s^2) R^T.  PyTorch normalises with F.normalize and multiplies with a batched
// GEMM whose summation order is the BLAS library's: a handful of fp32 roundings.  Here the formula is evaluated in double from
// the fp32 inputs and rounded once (54 double operations per Gaussian, once per visibility update), so every entry is the
// nearest float to the exact value (tests/test_visibility_refresh_gpu.py compares both with a float64 evaluation).
__global__ void __launch_bounds__(256)
bvh_prepare_leaves_kernel(int P, const float* __restrict__ means, const float* __restrict__ scales,
                          const float* __restrict__ rotations, int32_t* __restrict__ nodes, float* __restrict__ aabbs,
                          float* __restrict__ covs_inv)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    if (i < P - 1) {                                                // internal row i
        int32_t* n = nodes + 5 * (size_t)i;
        n[0] = n[1] = n[2] = n[3] = -1;
        n[4] = 0;
        float* b = aabbs + 6 * (size_t)i;
        b[0] = b[1] = b[2] = 100000.f;
        b[3] = b[4] = b[5] = -100000.f;
    }
    const size_t row = (size_t)(P - 1 + i);                         // leaf row of Gaussian i (the build sorts them)
    int32_t* n = nodes + 5 * row;
    n[0] = n[1] = n[2] = n[3] = -1;
    n[4] = 1;
    const float r0 = rotations[4 * (size_t)i], r1 = rotations[4 * (size_t)i + 1], r2 = rotations[4 * (size_t)i + 2],
                r3 = rotations[4 * (size_t)i + 3];
    const float norm = sqrtf(r0 * r0 + r1 * r1 + r2 * r2 + r3 * r3);
    const float w = r0 / norm, x = r1 / norm, y = r2 / norm, z = r3 / norm;
    const float R[9] = {1.f - 2.f * (y * y + z * z), 2.f * (x * y - w * z), 2.f * (x * z + w * y),
                        2.f * (x * y + w * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z - w * x),
                        2.f * (x * z - w * y), 2.f * (y * z + w * x), 1.f - 2.f * (x * x + y * y)};
    const float s0 = scales[3 * (size_t)i], s1 = scales[3 * (size_t)i + 1], s2 = scales[3 * (size_t)i + 2];
    const float sa = 3.f * s0, sb = 3.f * s1, sc = 3.f * s2;
    float* b = aabbs + 6 * row;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float m = means[3 * (size_t)i + a];
        const float ca = R[3 * a] * sa, cb = R[3 * a + 1] * sb, cc = R[3 * a + 2] * sc;
        float lo = 0.f, hi = 0.f;
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const float v = ((m + ((c & 4) ? -ca : ca)) + ((c & 2) ? -cb : cb)) + ((c & 1) ? -cc : cc);
            lo = c == 0 ? v : fminf(lo, v);
            hi = c == 0 ? v : fmaxf(hi, v);
        }
        b[a] = lo;
        b[3 + a] = hi;
    }
    // L = R diag(1/s); S = L L^T, the upper triangle row by row, from the fp32 inputs in double and rounded once
    const double q0 = r0, q1 = r1, q2 = r2, q3 = r3;
    const double qn = fmax(sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3), 1e-12);          // F.normalize's eps
    const double dw = q0 / qn, dx = q1 / qn, dy = q2 / qn, dz = q3 / qn;
    const double D[9] = {1.0 - 2.0 * (dy * dy + dz * dz), 2.0 * (dx * dy - dw * dz), 2.0 * (dx * dz + dw * dy),
                         2.0 * (dx * dy + dw * dz), 1.0 - 2.0 * (dx * dx + dz * dz), 2.0 * (dy * dz - dw * dx),
                         2.0 * (dx * dz - dw * dy), 2.0 * (dy * dz + dw * dx), 1.0 - 2.0 * (dx * dx + dy * dy)};
    const double i0 = 1.0 / (double)s0, i1 = 1.0 / (double)s1, i2 = 1.0 / (double)s2;
    double L[9];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        L[3 * a] = D[3 * a] * i0;
        L[3 * a + 1] = D[3 * a + 1] * i1;
        L[3 * a + 2] = D[3 * a + 2] * i2;
    }
    float* c = covs_inv + 6 * (size_t)i;
    int o = 0;
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int d = a; d < 3; d++)
            c[o++] = (float)(L[3 * a] * L[3 * d] + L[3 * a + 1] * L[3 * d + 1] + L[3 * a + 2] * L[3 * d + 2]);
}

// ---- host ----
size_t bvh_build_temp_bytes(size_t P)
{
    size_t o = 0;
    auto take = [&](size_t b) { o = align_up(o + b, 256); };
    take(P * 24);        // leaf box copy
    take(P * 8);         // keys in
    take(P * 8);         // keys out
    take(P * 4);         // vals in
    take(P * 4);         // vals out
    take(P * 4 + 4);     // flags
    take(1024 * 6 * 4);  // partial boxes
    take(256);           // whole box
    take(sort_temp_bytes(P));
    return o + 256;
}

void bvh_prepare_leaves(hipStream_t s, int P, const float* means, const float* scales, const float* rotations, int32_t* nodes,
                        float* aabbs, float* covs_inv)
{
    if (P <= 0) return;
    bvh_prepare_leaves_kernel<<<(P + 255) / 256, 256, 0, s>>>(P, means, scales, rotations, nodes, aabbs, covs_inv);
}

void bvh_build(hipStream_t s, int P, int32_t* nodes, float* aabbs, uint64_t* morton, void* temp)
{
    char* base = (char*)temp;
    size_t o = 0;
    auto take = [&](size_t b) { char* p = base + o; o = align_up(o + b, 256); return p; };
    float* leaf_copy = (float*)take((size_t)P * 24);
    uint64_t* k_in = (uint64_t*)take((size_t)P * 8);
    uint64_t* k_out = (uint64_t*)take((size_t)P * 8);
    uint32_t* v_in = (uint32_t*)take((size_t)P * 4);
    uint32_t* v_out = (uint32_t*)take((size_t)P * 4);
    int* flags = (int*)take((size_t)P * 4 + 4);
    float* partial = (float*)take(1024 * 6 * 4);
    float* whole = (float*)take(256);
    void* sort_temp = (void*)take(sort_temp_bytes((size_t)P));

    float* leaf = aabbs + 6 * (size_t)(P - 1);
    const int nb = min(1024, (P + 255) / 256);
    whole_box_partial_kernel<<<nb, 256, 0, s>>>(P, leaf, partial);
    whole_box_final_kernel<<<1, 64, 0, s>>>(nb, partial, whole);
    const int g = (P + 255) / 256;
    morton_kernel<<<g, 256, 0, s>>>(P, leaf, whole, k_in, v_in, leaf_copy);
    check_launch(s, false, "bvh morton");
    sort_pairs(s, (size_t)P, k_in, v_in, k_out, v_out, 30, sort_temp, false);
    scatter_leaves_kernel<<<g, 256, 0, s>>>(P, k_out, v_out, leaf_copy, aabbs, nodes, morton);
    check_launch(s, false, "bvh scatter_leaves");
    if (P > 1) {
        R3DG_HIP(hipMemsetAsync(flags, 0, (size_t)P * 4 + 4, s));
        int* nonzero_count_seen = flags + P;
        int2* ranges = reinterpret_cast<int2*>(k_in);                    // (the unsorted keys are dead after the sort)
        internal_nodes_kernel<<<(P - 1 + 255) / 256, 256, 0, s>>>(P, morton, nodes, ranges, nonzero_count_seen);
        check_launch(s, false, "bvh internal_nodes");
        // run tables in the (equally dead) unsorted-value buffer: ceil(P/256) + ceil(P/65536) boxes of 24 bytes <= 4 P bytes
        float* run1 = reinterpret_cast<float*>(v_in);
        const int n1 = (P + BOX_RUN - 1) / BOX_RUN, n2 = (n1 + BOX_RUN - 1) / BOX_RUN;
        float* run2 = run1 + 6 * (size_t)n1;
        const float* leaf_sorted = aabbs + 6 * (size_t)(P - 1);
        run_boxes_kernel<<<n1, 256, 0, s>>>(P, leaf_sorted, run1);
        run_boxes_kernel<<<n2, 256, 0, s>>>(n1, run1, run2);
        range_boxes_kernel<<<(P - 1 + 255) / 256, 256, 0, s>>>(P, ranges, leaf_sorted, run1, run2, nonzero_count_seen, nodes,
                                                              aabbs);
        check_launch(s, false, "bvh range_boxes");
        merge_boxes_kernel<<<g, 256, 0, s>>>(P, nodes, aabbs, flags, nonzero_count_seen);
        check_launch(s, false, "bvh merge_boxes");
    }
}

}  // namespace r3dg
