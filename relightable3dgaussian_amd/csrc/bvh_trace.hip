// Visibility trace (K18) and per-ray hit lists (K19) over the LBVH of bvh_build.hip, for gfx950.
// Reference semantics: trace_bvh_opacity_cuda bvh/src/trace.cu:196-286 (stack traversal, per-leaf Gaussian attenuation,
// T < 0.9 -> 0) and trace_bvh_cuda trace.cu:8-192.
//
// Compiled with -ffp-contract=off: integer hit counts and the {0, >= 0.9} class of a ray must equal the oracle's.
// The traversal stack holds 64 entries (reference: 32 with only a printf on overflow, trace.cuh:21-28); pushes beyond that
// are dropped and counted in *overflow so callers can detect it.
#include "launchers.hpp"
#include "ray_set.hpp"

namespace r3dg {

constexpr int TRACE_STACK = 64;

// ---- exact quotients without the division expansion ---------------------------------------------------------------------------
// A slab test divides six differences by the ray direction; hipcc expands each IEEE fp32 division into 11 instructions
// (2 v_div_scale, v_rcp, 5 FMA/mul, v_div_fmas, v_div_fixup): 12 divisions = two thirds of a node step's VALU work, all by
// the SAME three divisors for the whole life of the ray.  The expansion is r = rcp(d); r += (1 - d r) r; q = a r;
// q += (a - d q) r; q += (a - d q) r, wrapped in a power-of-two pre/post scaling that only engages for extreme exponents
// and a fix-up for zeros / infinities / NaNs.  Outside those cases the scaling is the identity, so keeping the refined
// reciprocal per ray and running the five remaining operations gives the SAME bits (same operations on the same values).
// Sufficient for "no scaling, no fix-up" (ISA, V_DIV_SCALE_F32): 2^-63 <= |d| <= 2 and the numerator 0 or
// 2^-103 <= |a| < 2^32; the latter holds for every difference of two TAME coordinates (0, or 2^-60 <= |x| < 2^31).
// Rays or nodes that are not tame (never in practice) take the compiler's division.  The sign of a zero quotient may
// differ; quotients are only compared.
__device__ __forceinline__ bool tame_coordinate(float x)
{
    const uint32_t e = (__float_as_uint(x) >> 23) & 0xffu;
    return x == 0.0f || (e >= 127u - 60u && e < 127u + 31u);
}
__device__ __forceinline__ bool tame_direction(float d)
{
    const uint32_t e = (__float_as_uint(d) >> 23) & 0xffu;
    return e >= 127u - 63u && e <= 127u;            // 2^-63 <= |d| < 2
}
__device__ __forceinline__ float refined_reciprocal(float d)
{
    const float r = __builtin_amdgcn_rcpf(d);
    const float e = __builtin_fmaf(-d, r, 1.0f);
    return __builtin_fmaf(e, r, r);
}
__device__ __forceinline__ float exact_quotient(float a, float neg_d, float r)
{
    const float q0 = a * r;
    const float e0 = __builtin_fmaf(neg_d, q0, a);
    const float q1 = __builtin_fmaf(e0, r, q0);
    const float e1 = __builtin_fmaf(neg_d, q1, a);
    return __builtin_fmaf(e1, r, q1);
}

// How a slab test forms (coordinate difference) / (ray direction), per axis: the compiler's division, or exact_quotient on
// the reciprocals a tame ray keeps
struct PlainDivision {
    float dx, dy, dz;
    __device__ __forceinline__ float x(float a) const { return a / dx; }
    __device__ __forceinline__ float y(float a) const { return a / dy; }
    __device__ __forceinline__ float z(float a) const { return a / dz; }
};
struct KeptReciprocal {
    float ndx, ndy, ndz, rx, ry, rz;            // negated direction, refined_reciprocal of the direction
    __device__ __forceinline__ float x(float a) const { return exact_quotient(a, ndx, rx); }
    __device__ __forceinline__ float y(float a) const { return exact_quotient(a, ndy, ry); }
    __device__ __forceinline__ float z(float a) const { return exact_quotient(a, ndz, rz); }
};

// ray / box (ray_intersects, utility.cuh:35-82): tmax of the parameter interval inside the box, -1 for a miss; the traversals
// only ask tmax > 0.  (The hit lists keep the whole interval: slab_interval below.  Each of the two is written the way its
// kernels were compiled from: hipcc schedules them differently when one is derived from the other.)
template <class Quotient>
__device__ __forceinline__ float slab_tmax(const float* __restrict__ box, float ox, float oy, float oz, const Quotient q)
{
    float tmin = q.x(box[0] - ox);
    float tmax = q.x(box[3] - ox);
    if (tmin > tmax) { const float t = tmin; tmin = tmax; tmax = t; }
    float tymin = q.y(box[1] - oy);
    float tymax = q.y(box[4] - oy);
    if (tymin > tymax) { const float t = tymin; tymin = tymax; tymax = t; }
    if (tmin > tymax || tymin > tmax) return -1.0f;
    if (tymin > tmin) tmin = tymin;
    if (tymax < tmax) tmax = tymax;
    float tzmin = q.z(box[2] - oz);
    float tzmax = q.z(box[5] - oz);
    if (tzmin > tzmax) { const float t = tzmin; tzmin = tzmax; tzmax = t; }
    if (tmin > tzmax || tzmin > tmax) return -1.0f;
    if (tzmax < tmax) tmax = tzmax;
    return tmax;
}

// ---- thread per ray over the reference's node and box tables (R3DG_OPT_TRACE_FORMULATION = 0) ---------------------------------
// The reference's own shape: the baseline the default is compared against bit for bit, and the kernel for a caller that
// cannot give the Gaussian count.
__global__ void __launch_bounds__(256)
trace_opacity_kernel(int num_rays, const int32_t* __restrict__ nodes, const float* __restrict__ aabbs,
                     const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                     const float* __restrict__ means, const float* __restrict__ covs, const float* __restrict__ opac,
                     const float* __restrict__ normals, int32_t* __restrict__ contributes, float* __restrict__ out,
                     int* __restrict__ overflow)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= num_rays) return;
    const float ox = rays_o[3 * (size_t)r], oy = rays_o[3 * (size_t)r + 1], oz = rays_o[3 * (size_t)r + 2];
    const float dx = rays_d[3 * (size_t)r], dy = rays_d[3 * (size_t)r + 1], dz = rays_d[3 * (size_t)r + 2];
    const PlainDivision by_d = {dx, dy, dz};
    int stack[TRACE_STACK];
    int sp = 0;
    stack[sp++] = 0;
    int count = 0;
    float T = 1.0f;
    bool lost = false;
    while (sp > 0) {
        const int node_id = stack[--sp];
        const int32_t* node = nodes + 5 * (size_t)node_id;
        if (node[4] <= 1) {
            const int g = node[3];
            const float op = opac[g];
            if (op < 1.f / 255.f) continue;
            const float nx = normals[3 * (size_t)g], ny = normals[3 * (size_t)g + 1], nz = normals[3 * (size_t)g + 2];
            if (nx * dx + ny * dy + nz * dz > 0) continue;
            const float* ci = covs + 6 * (size_t)g;
            const float c0 = ci[0], c1 = ci[1], c2 = ci[2], c3 = ci[3], c4 = ci[4], c5 = ci[5];
            const float mx = means[3 * (size_t)g], my = means[3 * (size_t)g + 1], mz = means[3 * (size_t)g + 2];
            const float m0 = mx - ox, m1 = my - oy, m2 = mz - oz;
            const float t1 = c0 * m0 * dx + c1 * m0 * dy + c2 * m0 * dz + c1 * m1 * dx + c3 * m1 * dy + c4 * m1 * dz +
                             c2 * m2 * dx + c4 * m2 * dy + c5 * m2 * dz;
            const float t2 = c0 * dx * dx + c1 * dx * dy + c2 * dx * dz + c1 * dy * dx + c3 * dy * dy + c4 * dy * dz +
                             c2 * dz * dx + c4 * dz * dy + c5 * dz * dz;
            const float t = t1 / t2;
            if (t < 0.01) continue;
            const float px = ox + t * dx, py = oy + t * dy, pz = oz + t * dz;
            const float f0 = mx - px, f1 = my - py, f2 = mz - pz;
            const float s = f0 * f0 * c0 + f1 * f1 * c3 + f2 * f2 * c5 + 2 * f0 * f1 * c1 + 2 * f0 * f2 * c2 +
                            2 * f1 * f2 * c4;
            const float power = -0.5f * s;
            if (power > 0) continue;
            count += 1;
            const float alpha = op * __expf(power);
            T *= 1 - alpha;
            if (T < 0.9) {
                out[r] = 0.0f;        // contributes[r] keeps its initial 0 (trace.cu:251-254)
                return;
            }
        } else {
            const int lid = node[1], rid = node[2];
            const float tl = slab_tmax(aabbs + 6 * (size_t)lid, ox, oy, oz, by_d);
            const float tr = slab_tmax(aabbs + 6 * (size_t)rid, ox, oy, oz, by_d);
            // the nearer child is pushed last, i.e. popped next
            const int first = tl > tr ? lid : rid, second = tl > tr ? rid : lid;
            const float tf = tl > tr ? tl : tr, ts = tl > tr ? tr : tl;
            if (tf > 0) { if (sp < TRACE_STACK) stack[sp++] = first; else lost = true; }
            if (ts > 0) { if (sp < TRACE_STACK) stack[sp++] = second; else lost = true; }
        }
    }
    contributes[r] = count;
    out[r] = T;
    if (lost) atomicAdd(overflow, 1);
}

// ---- packed traversal records ---------------------------------------------------------------------------------------------------
// rocprofv3 on the thread-per-ray kernel above (P=300k, K=64; profiles/r02_pmc_trace.json): 12.7e9 L2 requests per 6.4 M rays,
// 45 % of them L2 misses (3.3 TB/s of 64-byte lines from the Infinity Cache), VALU busy 37 %, lanes 26 % utilised -- the walk
// is bound by memory transactions, not by issue.  Every step touches 3 lines (node record 20 B, two child boxes 24 B each at
// unrelated rows) or 5 (leaf: node + opacity + normal + covariance + mean from five arrays), and the 42 MB working set is ten
// times one XCD's 4 MB L2.  pack_traversal_kernel rewrites the tree once per set of Gaussian arrays into one 64-byte record
// per internal node (both child ids and both child boxes) and one per leaf IN MORTON ORDER (mean, inverse covariance,
// opacity, normal): one line per step.
struct __attribute__((aligned(16))) TNode {
    int left, right;
    float lb[6], rb[6];
    int pad[2];
};
struct __attribute__((aligned(16))) TLeaf {
    float mean[3], cov[6], op, n[3];
    float pad[3];
};
static_assert(sizeof(TNode) == 64 && sizeof(TLeaf) == 64, "one cache line per traversal record");

__global__ void __launch_bounds__(256)
pack_traversal_kernel(int P, const int32_t* __restrict__ nodes, const float* __restrict__ aabbs,
                      const float* __restrict__ means, const float* __restrict__ covs, const float* __restrict__ opac,
                      const float* __restrict__ normals, TNode* __restrict__ tn, TLeaf* __restrict__ tl)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < P - 1) {
        TNode o;
        o.left = nodes[5 * (size_t)i + 1];
        o.right = nodes[5 * (size_t)i + 2];
#pragma unroll
        for (int a = 0; a < 6; a++) {
            o.lb[a] = aabbs[6 * (size_t)o.left + a];
            o.rb[a] = aabbs[6 * (size_t)o.right + a];
        }
        // pad[0] = 1: every box coordinate is 0 or has 2^-60 <= |x| < 2^31 (see exact_quotient)
        bool tame = true;
#pragma unroll
        for (int a = 0; a < 6; a++) tame = tame && tame_coordinate(o.lb[a]) && tame_coordinate(o.rb[a]);
        o.pad[0] = tame ? 1 : 0;
        o.pad[1] = 0;
        tn[i] = o;
    }
    if (i < P) {
        const int g = nodes[5 * (size_t)(P - 1 + i) + 3];
        TLeaf o;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            o.mean[a] = means[3 * (size_t)g + a];
            o.n[a] = normals[3 * (size_t)g + a];
            o.pad[a] = 0.f;
        }
#pragma unroll
        for (int a = 0; a < 6; a++) o.cov[a] = covs[6 * (size_t)g + a];
        o.op = opac[g];
        tl[i] = o;
    }
}

// ---- where the phased kernel's rays come from ------------------------------------------------------------------------------------
// A lane that refills asks its source for ray `idx` of the launch: origin, direction, and the row of the outputs the result
// goes to.  Everything else of the kernel (queues, refill, voting, termination) does not know which source it has.
// ArrayRays: one (rays_o, rays_d) row per ray, results in the same row -- the reference's interface.
struct ArrayRays {
    const float* __restrict__ rays_o;
    const float* __restrict__ rays_d;
    static constexpr bool optional_counts = false;
    __device__ __forceinline__ int load(int idx, const TLeaf* __restrict__, float& ox, float& oy, float& oz, float& dx, float& dy,
                                        float& dz) const
    {
        ox = rays_o[3 * (size_t)idx]; oy = rays_o[3 * (size_t)idx + 1]; oz = rays_o[3 * (size_t)idx + 2];
        dx = rays_d[3 * (size_t)idx]; dy = rays_d[3 * (size_t)idx + 1]; dz = rays_d[3 * (size_t)idx + 2];
        return idx;
    }
};
// BundleRays: the K visibility rays of every Gaussian of the Morton leaf slots [leaf_lo, leaf_hi), generated here.  Ray idx of
// the launch is sample k = idx % K of slot i = leaf_lo + idx / K: consecutive rays start at the same or at a neighbouring
// Gaussian by construction (what update_visibility arranges with a gather of the origins by the leaf order).  The origin
// Gaussian's mean and normal are in the packed leaf record tl[i]; the direction is sample k of the fixed ray set of that normal
// (ray_set.hpp: the function the fixed-ray-set shading kernels regenerate their directions with), the origin
// mean + direction * offset as a separate multiply and add (RayTracer.trace_visibility: rays_o + rays_d * 0.05 in PyTorch).
// The result belongs to row g * K + k of the outputs, g the slot's object id: the caller's order, no scatter pass behind the
// trace.  `dirs_out` (optional, [P,K,3]): the generated direction, for callers that need the tensor.
struct BundleRays {
    const int32_t* __restrict__ leaf_nodes;        // rows P-1.. of the node table: column 3 = object id of the slot
    const float* __restrict__ zsamples;            // [K,3]
    float* __restrict__ dirs_out;
    int K, leaf_lo;
    float offset;
    static constexpr bool optional_counts = true;
    __device__ __forceinline__ int load(int idx, const TLeaf* __restrict__ tl, float& ox, float& oy, float& oz, float& dx,
                                        float& dy, float& dz) const
    {
        const int q = idx / K, k = idx - q * K, i = leaf_lo + q;
        const TLeaf* __restrict__ leaf = tl + i;
        float R[9];
        rotation_between_z(leaf->n[0], leaf->n[1], leaf->n[2], R);
        ray_set_direction(R, zsamples[3 * k], zsamples[3 * k + 1], zsamples[3 * k + 2], dx, dy, dz);
        const float sx = dx * offset, sy = dy * offset, sz = dz * offset;
        ox = leaf->mean[0] + sx; oy = leaf->mean[1] + sy; oz = leaf->mean[2] + sz;
        const int row = leaf_nodes[5 * (size_t)i + 3] * K + k;
        if (dirs_out != nullptr) {
            dirs_out[3 * (size_t)row] = dx; dirs_out[3 * (size_t)row + 1] = dy; dirs_out[3 * (size_t)row + 2] = dz;
        }
        return row;
    }
};

// HemisphereRays: T random rays of every Gaussian of the Morton leaf slots [leaf_lo, leaf_hi) in the hemisphere of its normal, the
// rays GaussianModel.finetune_visibility draws one iteration at a time (scene/gaussian_model.py:293-296).  Ray idx of the launch
// is iteration t = idx % T of slot i = leaf_lo + idx / T: the origin coherence of BundleRays.  With g the slot's object id the
// direction is d = z / max(|z|, 1e-12) of the caller's draw z = raw_dirs[t, g, :] (F.normalize), negated when d . n_g < 0 (strict,
// n_g from the packed leaf record), the origin mean_g + d * offset as a separate multiply and add.  The result belongs to row
// t * P + g of the outputs and d to dirs_out[t, g, :]: iteration-major, what the fit kernel (visibility_bake.hip) reads coalesced.
struct HemisphereRays {
    const int32_t* __restrict__ leaf_nodes;        // rows P-1.. of the node table: column 3 = object id of the slot
    const float* __restrict__ raw_dirs;            // [T,P,3]
    float* __restrict__ dirs_out;                  // [T,P,3]
    int T, P, leaf_lo;
    float offset;
    static constexpr bool optional_counts = true;
    __device__ __forceinline__ int load(int idx, const TLeaf* __restrict__ tl, float& ox, float& oy, float& oz, float& dx,
                                        float& dy, float& dz) const
    {
        const int q = idx / T, t = idx - q * T, i = leaf_lo + q;
        const TLeaf* __restrict__ leaf = tl + i;
        const int g = leaf_nodes[5 * (size_t)i + 3];
        const int row = t * P + g;                 // (< P * T, which the caller checked to fit an int)
        const float zx = raw_dirs[3 * (size_t)row], zy = raw_dirs[3 * (size_t)row + 1], zz = raw_dirs[3 * (size_t)row + 2];
        const float len = fmaxf(sqrtf(zx * zx + zy * zy + zz * zz), 1e-12f);
        dx = zx / len; dy = zy / len; dz = zz / len;
        if (dx * leaf->n[0] + dy * leaf->n[1] + dz * leaf->n[2] < 0.f) { dx = -dx; dy = -dy; dz = -dz; }
        const float sx = dx * offset, sy = dy * offset, sz = dz * offset;
        ox = leaf->mean[0] + sx; oy = leaf->mean[1] + sy; oz = leaf->mean[2] + sz;
        dirs_out[3 * (size_t)row] = dx; dirs_out[3 * (size_t)row + 1] = dy; dirs_out[3 * (size_t)row + 2] = dz;
        return row;
    }
};

// ---- packed records, phase-separated persistent waves (R3DG_OPT_TRACE_FORMULATION = 1, default) -------------------------------
// Persistent waves: 83 % of the visibility rays are occluded after a handful of leaves while the rest walk thousands of
// nodes, so a fixed ray per thread leaves ~3/4 of the lanes idle.  Here a lane whose ray has finished pulls the next ray
// from a per-XCD queue with one wave-aggregated atomic per refill (once refill_min_idle lanes are idle, or all of them).
// XCD-contiguous queues: the host traces the ray bundles in Morton order of their origin Gaussian
// (train_step.update_visibility), the hardware places block b on XCD b % 8, and each XCD's queue is a contiguous eighth of
// the ray set -- so an XCD's 4 MB L2 serves one region of the scene (its subtree + the shared top levels) instead of 1/8 of
// everything.
// Phase separation: a loop that runs the leaf body (Gaussian response, ~60 VALU) and then the node body (two slab tests,
// ~70 VALU) executes BOTH whenever a wave holds lanes of either kind, which is nearly always: each lane advances one step
// for the price of two.  Here each lane keeps its current node in a register and the wave VOTES per iteration: the body
// with more ready lanes runs, the other lanes wait one turn.  The register also halves the stack traffic (a node whose
// children are both hit pushes one and continues with the other instead of push, push, pop).  Per-ray visit order,
// arithmetic and the overflow accounting are those of trace_opacity_kernel, so results are identical.
// COUNT (R3DG_OPT_TRACE_COUNT_VISITS, measurement builds of the same kernel): every lane counts the node steps (one slab test of
// both children) and leaf steps (one Gaussian evaluated) of its rays; one 64-bit atomic pair per wave at the end, into words
// 8..11 of the wave's own queue line (zeroed with the queue heads before the launch; read by r3dg_bvh_trace_visits).
// Rays: ArrayRays, BundleRays or HemisphereRays (above).  `ray` holds the OUTPUT row of the lane's current ray (< 0: idle).
template <bool COUNT, class Rays>
__global__ void __launch_bounds__(256)
trace_opacity_phased_kernel(int num_rays, int P, const TNode* __restrict__ tn, const TLeaf* __restrict__ tl, const Rays rays,
                            int32_t* __restrict__ contributes, float* __restrict__ out, int* __restrict__ overflow,
                            int* __restrict__ queues /* 8 x 16 ints, zeroed */, int refill_min_idle, int node_weight,
                            int leaf_weight)
{
    const int lane = threadIdx.x & 63;
    const int xcd = (int)(blockIdx.x & 7u);
    const int per = (num_rays + 7) / 8;
    // own queue first (locality); once it is empty the wave helps the next XCD's queue, and so on round the ring, so
    // an XCD whose eighth of the scene is cheap does not idle while a dense eighth finishes
    int q_turn = 0;
    int q_lo = min(num_rays, xcd * per), q_hi = min(num_rays, q_lo + per);
    int* next_ray = queues + 16 * xcd;
    unsigned long long* visit_words = reinterpret_cast<unsigned long long*>(queues + 16 * xcd + 8);
    unsigned int n_node_steps = 0u, n_leaf_steps = 0u;
    int stack[TRACE_STACK];
    int sp = 0, ray = -1, count = 0, cur = -1;
    float ox = 0.f, oy = 0.f, oz = 0.f, dx = 0.f, dy = 0.f, dz = 1.f, T = 1.0f;
    float rx = 0.f, ry = 0.f, rz = 1.f;          // refined reciprocals of the direction (exact_quotient)
    bool lost = false, exhausted = false, tame_ray = false;
    const int first_leaf = P - 1;
    while (true) {
        const unsigned long long idle = __ballot(ray < 0);
        if (idle != 0ull && !exhausted) {
            const int n_idle = __popcll(idle);
            if (n_idle >= refill_min_idle || idle == __ballot(true)) {
                int base = 0;
                const int leader = __builtin_ctzll(idle);
                if (lane == leader) base = atomicAdd(next_ray, n_idle);
                base = q_lo + __builtin_amdgcn_readlane(base, leader);
                const bool drained = base + n_idle >= q_hi;
                if (ray < 0) {
                    const int idx = base + __popcll(idle & ((1ull << lane) - 1ull));
                    if (idx < q_hi) {
                        ray = rays.load(idx, tl, ox, oy, oz, dx, dy, dz);
                        rx = refined_reciprocal(dx); ry = refined_reciprocal(dy); rz = refined_reciprocal(dz);
                        tame_ray = tame_direction(dx) && tame_direction(dy) && tame_direction(dz) && tame_coordinate(ox) &&
                                   tame_coordinate(oy) && tame_coordinate(oz);
                        cur = 0;
                        sp = 0;
                        count = 0;
                        T = 1.0f;
                    }
                }
                if (drained) {
                    if (++q_turn == 8) exhausted = true;
                    else {
                        const int q = (xcd + q_turn) & 7;
                        q_lo = min(num_rays, q * per);
                        q_hi = min(num_rays, q_lo + per);
                        next_ray = queues + 16 * q;
                    }
                }
            }
        }
        const bool at_leaf = ray >= 0 && cur >= first_leaf;
        const bool at_node = ray >= 0 && cur < first_leaf;
        const unsigned long long leaf_m = __ballot(at_leaf), node_m = __ballot(at_node);
        if ((leaf_m | node_m) == 0ull) {
            if (exhausted) break;
            continue;
        }
        bool finished = false, stepped = false;
        if (__popcll(node_m) * node_weight >= __popcll(leaf_m) * leaf_weight) {
            float4 q0 = {}, q1 = {}, q2 = {}, q3 = {};
            if (at_node) {
                const float4* q = reinterpret_cast<const float4*>(tn + cur);
                q0 = q[0]; q1 = q[1]; q2 = q[2]; q3 = q[3];
            }
            const float lb[6] = {q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
            const float rb[6] = {q2.x, q2.y, q2.z, q2.w, q3.x, q3.y};
            float tl_ = -1.0f, tr_ = -1.0f;
            if (__ballot(at_node && !(tame_ray && __float_as_int(q3.z) != 0)) == 0ull) {
                if (at_node) {
                    const KeptReciprocal by_r = {-dx, -dy, -dz, rx, ry, rz};
                    tl_ = slab_tmax(lb, ox, oy, oz, by_r);
                    tr_ = slab_tmax(rb, ox, oy, oz, by_r);
                }
            } else if (at_node) {
                const PlainDivision by_d = {dx, dy, dz};
                tl_ = slab_tmax(lb, ox, oy, oz, by_d);
                tr_ = slab_tmax(rb, ox, oy, oz, by_d);
            }
            if (at_node) {
                stepped = true;
                if (COUNT) ++n_node_steps;
                const int lid = __float_as_int(q0.x), rid = __float_as_int(q0.y);
                const int first = tl_ > tr_ ? lid : rid, second = tl_ > tr_ ? rid : lid;
                const float tf = tl_ > tr_ ? tl_ : tr_, ts = tl_ > tr_ ? tr_ : tl_;
                // trace_opacity_kernel pushes `first`, then `second`, and pops `second` next: it stays in the register instead
                cur = -1;
                if (tf > 0) {
                    if (ts > 0) {
                        if (sp < TRACE_STACK) stack[sp++] = first; else lost = true;
                        if (sp < TRACE_STACK) cur = second; else lost = true;
                    } else {
                        if (sp < TRACE_STACK) cur = first; else lost = true;
                    }
                }
            }
        } else if (at_leaf) {
            stepped = true;
            if (COUNT) ++n_leaf_steps;
            // the Gaussian response of trace_opacity_kernel, written out here too: hipcc allocates the registers of both
            // kernels differently once the body is a function they share
            const float4* q = reinterpret_cast<const float4*>(tl + (cur - first_leaf));
            const float4 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
            const float op = q2.y;
            const float nx = q2.z, ny = q2.w, nz = q3.x;
            if (!(op < 1.f / 255.f) && !(nx * dx + ny * dy + nz * dz > 0)) {
                const float c0 = q0.w, c1 = q1.x, c2 = q1.y, c3 = q1.z, c4 = q1.w, c5 = q2.x;
                const float mx = q0.x, my = q0.y, mz = q0.z;
                const float m0 = mx - ox, m1 = my - oy, m2 = mz - oz;
                const float t1 = c0 * m0 * dx + c1 * m0 * dy + c2 * m0 * dz + c1 * m1 * dx + c3 * m1 * dy + c4 * m1 * dz +
                                 c2 * m2 * dx + c4 * m2 * dy + c5 * m2 * dz;
                const float t2 = c0 * dx * dx + c1 * dx * dy + c2 * dx * dz + c1 * dy * dx + c3 * dy * dy + c4 * dy * dz +
                                 c2 * dz * dx + c4 * dz * dy + c5 * dz * dz;
                const float t = t1 / t2;
                if (!(t < 0.01)) {
                    const float px = ox + t * dx, py = oy + t * dy, pz = oz + t * dz;
                    const float f0 = mx - px, f1 = my - py, f2 = mz - pz;
                    const float s = f0 * f0 * c0 + f1 * f1 * c3 + f2 * f2 * c5 + 2 * f0 * f1 * c1 + 2 * f0 * f2 * c2 +
                                    2 * f1 * f2 * c4;
                    const float power = -0.5f * s;
                    if (!(power > 0)) {
                        count += 1;
                        const float alpha = op * __expf(power);
                        T *= 1 - alpha;
                        if (T < 0.9) {          // retired with 0; contributes keeps 0 (trace.cu:251-254)
                            T = 0.0f;
                            count = 0;
                            finished = true;
                        }
                    }
                }
            }
            cur = -1;
        }
        if (stepped) {
            if (!finished && cur < 0 && sp > 0) cur = stack[--sp];
            if (finished || cur < 0) {
                if (!Rays::optional_counts || contributes != nullptr) contributes[ray] = count;
                out[ray] = T;
                ray = -1;
                sp = 0;
                cur = -1;
            }
        }
    }
    if (lost) atomicAdd(overflow, 1);
    if (COUNT) {
        unsigned long long a = n_node_steps, b = n_leaf_steps;
        for (int d = 32; d > 0; d >>= 1) {
            a += __shfl_xor(a, d);
            b += __shfl_xor(b, d);
        }
        if (lane == 0) {
            atomicAdd(visit_words, a);
            atomicAdd(visit_words + 1, b);
        }
    }
}

// ---- trace_bvh: per-ray hit lists (K19; bvh/src/trace.cu:8-192, bound at bvh/src/bindings.cpp:11) ----------------------------
// Pass 1 counts, per ray, the leaves of every subtree of <= 4 leaves whose box the ray reaches (tmax > 0 on the way down);
// the caller scans the counts; pass 2 repeats the walk carrying each node's (tmin, tmax) and writes one entry per such leaf:
// t = (mean - o) . d (the POINT form of ray_intersects, utility.cuh:84-88), rejected (t = 1e6, id = -1) unless
// 0.01 <= t and tmin <= t <= tmax of the collapsed subtree's box; key = ray << 32 | bits(t), position = o + t d.
// The caller then sorts the entries of each ray by t (stable sort on the key).  No Python caller exists in the reference.
__device__ __forceinline__ float2 slab_interval(const float* __restrict__ box, float ox, float oy, float oz, float dx,
                                                float dy, float dz)
{
    float tmin = (box[0] - ox) / dx;
    float tmax = (box[3] - ox) / dx;
    if (tmin > tmax) { const float t = tmin; tmin = tmax; tmax = t; }
    float tymin = (box[1] - oy) / dy;
    float tymax = (box[4] - oy) / dy;
    if (tymin > tymax) { const float t = tymin; tymin = tymax; tymax = t; }
    if (tmin > tymax || tymin > tmax) return make_float2(-1.0f, -1.0f);
    if (tymin > tmin) tmin = tymin;
    if (tymax < tmax) tmax = tymax;
    float tzmin = (box[2] - oz) / dz;
    float tzmax = (box[5] - oz) / dz;
    if (tzmin > tzmax) { const float t = tzmin; tzmin = tzmax; tzmax = t; }
    if (tmin > tzmax || tzmin > tmax) return make_float2(-1.0f, -1.0f);
    if (tzmin > tmin) tmin = tzmin;
    if (tzmax < tmax) tmax = tzmax;
    return make_float2(tmin, tmax);
}

__global__ void __launch_bounds__(256)
trace_count_kernel(int num_rays, const int32_t* __restrict__ nodes, const float* __restrict__ aabbs,
                   const float* __restrict__ rays_o, const float* __restrict__ rays_d, int32_t* __restrict__ counts,
                   int* __restrict__ overflow)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= num_rays) return;
    const float ox = rays_o[3 * (size_t)r], oy = rays_o[3 * (size_t)r + 1], oz = rays_o[3 * (size_t)r + 2];
    const float dx = rays_d[3 * (size_t)r], dy = rays_d[3 * (size_t)r + 1], dz = rays_d[3 * (size_t)r + 2];
    int stack[TRACE_STACK];
    int sp = 0, count = 0;
    bool lost = false;
    stack[sp++] = 0;
    while (sp > 0) {
        const int32_t* node = nodes + 5 * (size_t)stack[--sp];
        if (node[4] <= 4) {
            count += node[4];
        } else {
            const int lid = node[1], rid = node[2];
            const float tl = slab_interval(aabbs + 6 * (size_t)lid, ox, oy, oz, dx, dy, dz).y;
            const float tr = slab_interval(aabbs + 6 * (size_t)rid, ox, oy, oz, dx, dy, dz).y;
            const int first = tl > tr ? lid : rid, second = tl > tr ? rid : lid;
            const float tf = tl > tr ? tl : tr, ts = tl > tr ? tr : tl;
            if (tf > 0) { if (sp < TRACE_STACK) stack[sp++] = first; else lost = true; }
            if (ts > 0) { if (sp < TRACE_STACK) stack[sp++] = second; else lost = true; }
        }
    }
    counts[r] = count;
    if (lost) atomicAdd(overflow, 1);
}

__global__ void __launch_bounds__(256)
trace_fill_kernel(int num_rays, const int32_t* __restrict__ nodes, const float* __restrict__ aabbs,
                  const float* __restrict__ rays_o, const float* __restrict__ rays_d, const float* __restrict__ means,
                  const int32_t* __restrict__ counts, const int64_t* __restrict__ offsets_inclusive,
                  uint64_t* __restrict__ keys, int32_t* __restrict__ points, float* __restrict__ positions,
                  int32_t* __restrict__ ray_ids)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= num_rays) return;
    if (counts[r] == 0) return;
    const size_t offset = r == 0 ? 0 : (size_t)offsets_inclusive[r - 1];
    const float ox = rays_o[3 * (size_t)r], oy = rays_o[3 * (size_t)r + 1], oz = rays_o[3 * (size_t)r + 2];
    const float dx = rays_d[3 * (size_t)r], dy = rays_d[3 * (size_t)r + 1], dz = rays_d[3 * (size_t)r + 2];
    int stack[TRACE_STACK];
    float2 stack_t[TRACE_STACK];
    int sp = 0, count = 0;
    stack[0] = 0;
    stack_t[0] = make_float2(-1000.f, 1000.f);
    sp = 1;
    while (sp > 0) {
        --sp;
        const int node_id = stack[sp];
        const float2 iv = stack_t[sp];
        const int32_t* node = nodes + 5 * (size_t)node_id;
        if (node[4] <= 4) {
            int stack2[8];
            int sp2 = 0;
            stack2[sp2++] = node_id;
            while (sp2 > 0) {
                const int32_t* n2 = nodes + 5 * (size_t)stack2[--sp2];
                if (n2[3] >= 0) {
                    int object_id = n2[3];
                    float t = (means[3 * (size_t)object_id] - ox) * dx + (means[3 * (size_t)object_id + 1] - oy) * dy +
                              (means[3 * (size_t)object_id + 2] - oz) * dz;
                    if (t < 0.01 || t < iv.x || t > iv.y) {
                        t = 1000000.f;
                        object_id = -1;
                    }
                    const size_t w = offset + (size_t)count;
                    keys[w] = ((uint64_t)(uint32_t)r << 32) | (uint64_t)__float_as_uint(t);
                    points[w] = object_id;
                    ray_ids[w] = r;
                    positions[3 * w] = ox + t * dx;
                    positions[3 * w + 1] = oy + t * dy;
                    positions[3 * w + 2] = oz + t * dz;
                    ++count;
                } else if (sp2 + 2 <= 8) {
                    stack2[sp2++] = n2[1];
                    stack2[sp2++] = n2[2];
                }
            }
        } else {
            const int lid = node[1], rid = node[2];
            const float2 il = slab_interval(aabbs + 6 * (size_t)lid, ox, oy, oz, dx, dy, dz);
            const float2 ir = slab_interval(aabbs + 6 * (size_t)rid, ox, oy, oz, dx, dy, dz);
            const bool lf = il.y > ir.y;
            const int first = lf ? lid : rid, second = lf ? rid : lid;
            const float2 i1 = lf ? il : ir, i2 = lf ? ir : il;
            if (i1.y > 0 && sp < TRACE_STACK) { stack[sp] = first; stack_t[sp] = i1; sp++; }
            if (i2.y > 0 && sp < TRACE_STACK) { stack[sp] = second; stack_t[sp] = i2; sp++; }
        }
    }
}

// ---- host ----
void bvh_trace_count(hipStream_t s, int num_rays, const int32_t* nodes, const float* aabbs, const float* rays_o,
                     const float* rays_d, int32_t* counts, int* overflow)
{
    if (num_rays <= 0) return;
    trace_count_kernel<<<(num_rays + 255) / 256, 256, 0, s>>>(num_rays, nodes, aabbs, rays_o, rays_d, counts, overflow);
}

void bvh_trace_fill(hipStream_t s, int num_rays, const int32_t* nodes, const float* aabbs, const float* rays_o,
                    const float* rays_d, const float* means, const int32_t* counts, const int64_t* offsets_inclusive,
                    uint64_t* keys, int32_t* points, float* positions, int32_t* ray_ids)
{
    if (num_rays <= 0) return;
    trace_fill_kernel<<<(num_rays + 255) / 256, 256, 0, s>>>(num_rays, nodes, aabbs, rays_o, rays_d, means, counts,
                                                            offsets_inclusive, keys, points, positions, ray_ids);
}

// Packed traversal records: 64 bytes per internal node + 64 bytes per leaf + the 8 per-XCD ray-queue heads (8 x 64 bytes).
// The buffer belongs to the CALLER (r3dg_bvh_pack_traversal / r3dg_bvh_trace_opacity_packed: one per tracer, packed once per
// set of Gaussian arrays); the reference-shaped entry point r3dg_bvh_trace_opacity packs per call into a scratch buffer that
// is private to its (device, stream) pair, so tracers on different streams or threads never share records or queue heads.
size_t bvh_trace_records_bytes(size_t P) { return (P + 8) * 128 + 8 * 64; }

void bvh_pack_traversal(hipStream_t s, int P, const int32_t* nodes, const float* aabbs, const float* means, const float* covs,
                        const float* opac, const float* normals, void* records)
{
    if (P <= 0) return;
    char* rec = reinterpret_cast<char*>(records);
    TNode* tn = reinterpret_cast<TNode*>(rec);
    TLeaf* tl = reinterpret_cast<TLeaf*>(rec + (size_t)P * 64);
    pack_traversal_kernel<<<(P + 255) / 256, 256, 0, s>>>(P, nodes, aabbs, means, covs, opac, normals, tn, tl);
}

// the phase-separated trace over records written by bvh_pack_traversal
void bvh_trace_opacity_packed(hipStream_t s, int num_rays, int P, void* records, const float* rays_o, const float* rays_d,
                              int32_t* contributes, float* out, int* overflow)
{
    if (num_rays <= 0 || P <= 0) return;
    char* rec = reinterpret_cast<char*>(records);
    TNode* tn = reinterpret_cast<TNode*>(rec);
    TLeaf* tl = reinterpret_cast<TLeaf*>(rec + (size_t)P * 64);
    int* queues = reinterpret_cast<int*>(rec + (size_t)P * 128);               // 8 x 64 bytes behind the records
    const int nblk = (num_rays + 255) / 256, chunk = (nblk + 7) / 8;
    const int cus = persistent_cus();                                           // leaves CUs to a concurrent collective
    R3DG_HIP(hipMemsetAsync(queues, 0, 8 * 64, s));
    const int cap = cus * 8;                                                    // 8 waves per SIMD, all resident
    const int grid = chunk * 8 < cap ? chunk * 8 : cap;
    const ArrayRays rays = {rays_o, rays_d};
    if (opt(R3DG_OPT_TRACE_COUNT_VISITS))
        trace_opacity_phased_kernel<true, ArrayRays><<<grid, 256, 0, s>>>(num_rays, P, tn, tl, rays, contributes, out, overflow,
                                                                         queues, opt(R3DG_OPT_TRACE_REFILL),
                                                                         opt(R3DG_OPT_TRACE_NODE_WEIGHT), opt(R3DG_OPT_TRACE_LEAF_WEIGHT));
    else
        trace_opacity_phased_kernel<false, ArrayRays><<<grid, 256, 0, s>>>(num_rays, P, tn, tl, rays, contributes, out, overflow,
                                                                          queues, opt(R3DG_OPT_TRACE_REFILL),
                                                                          opt(R3DG_OPT_TRACE_NODE_WEIGHT), opt(R3DG_OPT_TRACE_LEAF_WEIGHT));
}

// the same trace with the rays generated in the kernel: the K rays of every Gaussian of the leaf slots [leaf_lo, leaf_hi) of the
// tree `nodes` / `records` describe (BundleRays); results at rows g * K + k of out / contributes (NULL: not wanted) / dirs_out
// (NULL: not wanted), rows of other leaves untouched
void bvh_trace_bundles(hipStream_t s, int P, int K, void* records, const int32_t* nodes, const float* zsamples, int leaf_lo,
                       int leaf_hi, float origin_offset, float* out, int32_t* contributes, float* dirs_out, int* overflow)
{
    if (P <= 0 || K <= 0 || leaf_hi <= leaf_lo) return;
    char* rec = reinterpret_cast<char*>(records);
    TNode* tn = reinterpret_cast<TNode*>(rec);
    TLeaf* tl = reinterpret_cast<TLeaf*>(rec + (size_t)P * 64);
    int* queues = reinterpret_cast<int*>(rec + (size_t)P * 128);
    const int num_rays = (leaf_hi - leaf_lo) * K;                               // (<= P * K, which the caller checked)
    const int nblk = (num_rays + 255) / 256, chunk = (nblk + 7) / 8;
    const int cap = persistent_cus() * 8;
    const int grid = chunk * 8 < cap ? chunk * 8 : cap;
    R3DG_HIP(hipMemsetAsync(queues, 0, 8 * 64, s));
    const BundleRays rays = {nodes + 5 * (size_t)(P - 1), zsamples, dirs_out, K, leaf_lo, origin_offset};
    if (opt(R3DG_OPT_TRACE_COUNT_VISITS))
        trace_opacity_phased_kernel<true, BundleRays><<<grid, 256, 0, s>>>(num_rays, P, tn, tl, rays, contributes, out, overflow,
                                                                          queues, opt(R3DG_OPT_TRACE_REFILL),
                                                                          opt(R3DG_OPT_TRACE_NODE_WEIGHT), opt(R3DG_OPT_TRACE_LEAF_WEIGHT));
    else
        trace_opacity_phased_kernel<false, BundleRays><<<grid, 256, 0, s>>>(num_rays, P, tn, tl, rays, contributes, out, overflow,
                                                                           queues, opt(R3DG_OPT_TRACE_REFILL),
                                                                           opt(R3DG_OPT_TRACE_NODE_WEIGHT), opt(R3DG_OPT_TRACE_LEAF_WEIGHT));
}

// the same trace over the T hemisphere rays of every Gaussian of the leaf slots [leaf_lo, leaf_hi) (HemisphereRays): results at rows
// t * P + g of out / contributes (NULL: not wanted) / dirs_out, rows of other leaves untouched
void bvh_trace_hemisphere(hipStream_t s, int P, int T, void* records, const int32_t* nodes, const float* raw_dirs, int leaf_lo,
                          int leaf_hi, float origin_offset, float* out, float* dirs_out, int32_t* contributes, int* overflow)
{
    if (P <= 0 || T <= 0 || leaf_hi <= leaf_lo) return;
    char* rec = reinterpret_cast<char*>(records);
    TNode* tn = reinterpret_cast<TNode*>(rec);
    TLeaf* tl = reinterpret_cast<TLeaf*>(rec + (size_t)P * 64);
    int* queues = reinterpret_cast<int*>(rec + (size_t)P * 128);
    const int num_rays = (leaf_hi - leaf_lo) * T;                               // (<= P * T, which the caller checked)
    const int nblk = (num_rays + 255) / 256, chunk = (nblk + 7) / 8;
    const int cap = persistent_cus() * 8;
    const int grid = chunk * 8 < cap ? chunk * 8 : cap;
    R3DG_HIP(hipMemsetAsync(queues, 0, 8 * 64, s));
    const HemisphereRays rays = {nodes + 5 * (size_t)(P - 1), raw_dirs, dirs_out, T, P, leaf_lo, origin_offset};
    if (opt(R3DG_OPT_TRACE_COUNT_VISITS))
        trace_opacity_phased_kernel<true, HemisphereRays><<<grid, 256, 0, s>>>(num_rays, P, tn, tl, rays, contributes, out, overflow,
                                                                              queues, opt(R3DG_OPT_TRACE_REFILL),
                                                                              opt(R3DG_OPT_TRACE_NODE_WEIGHT), opt(R3DG_OPT_TRACE_LEAF_WEIGHT));
    else
        trace_opacity_phased_kernel<false, HemisphereRays><<<grid, 256, 0, s>>>(num_rays, P, tn, tl, rays, contributes, out, overflow,
                                                                               queues, opt(R3DG_OPT_TRACE_REFILL),
                                                                               opt(R3DG_OPT_TRACE_NODE_WEIGHT), opt(R3DG_OPT_TRACE_LEAF_WEIGHT));
}

// node / leaf steps of the LAST counting trace over these records (sums over the eight queue lines; synchronises the stream)
void bvh_trace_visits(hipStream_t s, int P, const void* records, unsigned long long out[2])
{
    unsigned long long lines[8 * 8];
    R3DG_HIP(hipStreamSynchronize(s));
    R3DG_HIP(hipMemcpy(lines, reinterpret_cast<const char*>(records) + (size_t)P * 128, sizeof(lines), hipMemcpyDeviceToHost));
    out[0] = out[1] = 0ull;
    for (int q = 0; q < 8; ++q) {
        out[0] += lines[8 * q + 4];
        out[1] += lines[8 * q + 5];
    }
}

// scratch records of the reference-shaped entry point: one grow-only buffer per (device, stream) (common.hpp stream_scratch)
static void* trace_scratch(hipStream_t s, size_t bytes) { return stream_scratch(s, 2, bytes); }

// P = number of Gaussians (rows of means / leaves of the tree); P <= 0: unknown -> thread per ray over the caller's tables
void bvh_trace_opacity(hipStream_t s, int num_rays, int P, const int32_t* nodes, const float* aabbs, const float* rays_o,
                       const float* rays_d, const float* means, const float* covs, const float* opac,
                       const float* normals, int32_t* contributes, float* out, int* overflow)
{
    if (num_rays <= 0) return;
    if (opt(R3DG_OPT_TRACE_FORMULATION) == 1 && P > 0) {
        void* rec = trace_scratch(s, bvh_trace_records_bytes((size_t)P));
        bvh_pack_traversal(s, P, nodes, aabbs, means, covs, opac, normals, rec);
        bvh_trace_opacity_packed(s, num_rays, P, rec, rays_o, rays_d, contributes, out, overflow);
    } else
        trace_opacity_kernel<<<(num_rays + 255) / 256, 256, 0, s>>>(num_rays, nodes, aabbs, rays_o, rays_d, means, covs,
                                                                   opac, normals, contributes, out, overflow);
}

}  // namespace r3dg
