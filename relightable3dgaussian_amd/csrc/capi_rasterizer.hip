// C ABI of the rasterizer (include/r3dg_hip.h): state-buffer layouts, orchestration of the forward (one call, two-phase or
// bounded) and of the backward.  Mirrors CudaRasterizer::Rasterizer::forward/backward (rasterizer_impl.cu:199-380, :384-491)
// in the order of work, not in code.
#include "adam_update.hpp"
#include "capi_internal.hpp"

#include <cstring>
#include <mutex>
#include <vector>

namespace r3dg {

// ---- state layouts (opaque to callers; 256-byte aligned sub-arrays) ----
GeometryLayout GeometryLayout::make(size_t P)
{
    GeometryLayout L;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o = align_up(o + bytes, 256); return r; };
    L.depths = take(P * 4);
    L.clamped = take(P * 3);
    L.radii = take(P * 4);
    L.means2D = take(P * 8);
    L.cov3D = take(P * 24);
    L.conic_opacity = take(P * 16);
    L.rgb = take(P * 12);
    L.tiles_touched = take(P * 4);
    L.point_offsets = take(P * 4);
    L.block_sums = take(((P + 255) / 256 + 1) * 4);
    L.total = take(8);
    // packed per-Gaussian record read by the tile kernels (64-byte stride = one line per staged instance):
    // [mean.x mean.y conic.x conic.y | conic.z opacity depth 0 | r g b 0 | unused]
    L.splat = take(P * 64);
    L.bytes = o;
    return L;
}
ImageLayout ImageLayout::make(size_t N, size_t T)
{
    ImageLayout L;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o = align_up(o + bytes, 256); return r; };
    L.final_T = take(N * 4);
    L.n_contrib = take(N * 4);
    L.ranges = take(T * 8);
    L.tile_order = take(T * 4);
    L.big_list = take(T * 4);        // tile-binned ordering: tiles too long for the small in-LDS sort
    L.big_count = take(256);
    L.bytes = o;
    return L;
}
BinningLayout BinningLayout::make(size_t R)
{
    BinningLayout L;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o = align_up(o + bytes, 256); return r; };
    L.keys_unsorted = take(R * 8);
    L.keys = take(R * 8);
    L.vals_unsorted = take(R * 4);
    L.vals = take(R * 4);
    L.sort_temp = take(sort_temp_bytes(R));
    L.bytes = o;
    return L;
}

// reference getHigherMsb (rasterizer_impl.cu:35-50): position of the bit above the MSB of n
static uint32_t higher_msb(uint32_t n)
{
    uint32_t b = 0;
    while (b < 32 && (n >> b)) b++;
    return b;
}

// the direct tile binning (R3DG_OPT_TILE_BINNING 2) keeps its tile counters in LDS: T tiles must fit
static bool direct_binning_usable(long long T)
{
    return opt(R3DG_OPT_TILE_BINNING) == 2 && T <= (long long)tile_binning_max_tiles();
}

// What (P, width, height) fix of a rasterizer call: the tile grid and the two state layouts that do not depend on the
// instance count (BinningLayout is made where R or the capacity is known).
struct RasterView {
    int gx, gy;
    size_t T, N;
    GeometryLayout G;
    ImageLayout I;
    static RasterView make(int P, int width, int height)
    {
        const int gx = (width + R3DG_TILE_X - 1) / R3DG_TILE_X, gy = (height + R3DG_TILE_Y - 1) / R3DG_TILE_Y;
        const size_t T = (size_t)gx * gy, N = (size_t)width * height;
        return RasterView{gx, gy, T, N, GeometryLayout::make((size_t)P), ImageLayout::make(N, T)};
    }
};

// The arguments of r3dg_rasterize_forward_begin[_bounded] (the two structs by value: the caller's may be temporaries), then the
// four that only the bounded forward has (capacity < 0: the exact two-phase forward).
struct ForwardArgs {
    void* stream;
    r3dg_alloc_fn geometry_alloc, binning_alloc, image_alloc;
    void* user;
    r3dg_raster_scene scene;
    r3dg_raster_outputs out;
    long long capacity;
    float* overflow_flag;
    unsigned int* overflow_count;
    void* ordering_stream;          // (may be NULL: the caller's stream)
};

// ---- forward, in two halves -----------------------------------------------------------------------------------------
// begin : validation, state allocation, preprocess (K2/K3), asynchronous read-back of num_rendered (event recorded)
// finish: waits for THAT event only (not for the stream), sizes the binning state, orders the instances, renders.
// Work the caller enqueues on the stream between the two halves (e.g. the shading kernels that produce the feature
// rows) keeps the GPU busy while the host waits for the count and enqueues the second half.
struct ForwardTicket {
    ForwardArgs a;
    RasterView v;
    float focal_x, focal_y;
    int* radii_p;                        // the caller's radii or the geometry state's
    char *gbuf, *ibuf;
    hipEvent_t ready, ordered;           // two-phase forward: the count has arrived | bounded forward: the ordering is queued
    unsigned long long* host_total;      // pinned
    char* bbuf;                          // binning state; bounded forward: laid out for `capacity` instances by _begin_
    bool fused_front;                    // _begin_ allocated bbuf and launched the folded front end (forward_begin_impl)
    uint32_t* point_list;                // the depth-sorted per-tile lists in bbuf (enqueue_ordering)
};

static std::mutex g_ticket_mutex;
static std::vector<ForwardTicket*> g_ticket_pool;

static ForwardTicket* ticket_acquire()
{
    {
        std::lock_guard<std::mutex> lk(g_ticket_mutex);
        if (!g_ticket_pool.empty()) {
            ForwardTicket* t = g_ticket_pool.back();
            g_ticket_pool.pop_back();
            return t;
        }
    }
    ForwardTicket* t = new ForwardTicket();
    R3DG_HIP(hipEventCreateWithFlags(&t->ready, hipEventDisableTiming));     // (the host synchronises on this one: system scope)
    R3DG_HIP(hipEventCreateWithFlags(&t->ordered, hipEventDisableTiming));
    R3DG_HIP(hipHostMalloc((void**)&t->host_total, sizeof(unsigned long long), hipHostMallocDefault));
    return t;
}
static void ticket_release(ForwardTicket* t)
{
    std::lock_guard<std::mutex> lk(g_ticket_mutex);
    g_ticket_pool.push_back(t);
}

// Instance ordering (K5-K7) of a forward whose projection has run: binning state for R instance slots, tile ranges, the
// depth-sorted per-tile lists.  Bounded tickets (capacity >= 0) need the direct tile binning -- the only formulation whose
// launches do not depend on the count.
static int enqueue_ordering(ForwardTicket* t, hipStream_t stream, int R)
{
    const ForwardArgs& a = t->a;
    const GeometryLayout& G = t->v.G;
    const ImageLayout& I = t->v.I;
    const bool debug = a.out.debug != 0;
    const int P = a.scene.P, gx = t->v.gx, gy = t->v.gy, T = (int)t->v.T;
    char *gbuf = t->gbuf, *ibuf = t->ibuf;
    int* radii_p = t->radii_p;
    float* g_depths = (float*)(gbuf + G.depths);
    float* g_means2D = (float*)(gbuf + G.means2D);
    uint32_t* g_tiles = (uint32_t*)(gbuf + G.tiles_touched);
    uint32_t* g_block = (uint32_t*)(gbuf + G.block_sums);
    const bool direct = direct_binning_usable((long long)t->v.T);
    if (a.capacity >= 0 && !direct) {
        set_error("rasterize_forward (bounded): needs the direct tile binning and at most 16384 tiles: ask r3dg_bounded_forward_supported(width, height) first");
        return R3DG_EINVAL;
    }
    BinningLayout B = BinningLayout::make((size_t)R);
    char* bbuf = t->fused_front ? t->bbuf : (char*)a.binning_alloc(a.user, B.bytes);     // (fused: allocated by _begin)
    t->bbuf = bbuf;
    if (!bbuf) { set_error("rasterize_forward: binning resize callback returned NULL"); return R3DG_EALLOC; }
    uint64_t* keys_u = (uint64_t*)(bbuf + B.keys_unsorted);
    uint64_t* keys = (uint64_t*)(bbuf + B.keys);
    uint32_t* vals_u = (uint32_t*)(bbuf + B.vals_unsorted);
    uint32_t* vals = (uint32_t*)(bbuf + B.vals);
    t->point_list = vals;

    uint32_t* ranges = (uint32_t*)(ibuf + I.ranges);
    uint32_t* order = (uint32_t*)(ibuf + I.tile_order);         // (the per-tile sorts walk it whether or not the tile kernels do)
    uint32_t* big_list = (uint32_t*)(ibuf + I.big_list);
    uint32_t* big_count = (uint32_t*)(ibuf + I.big_count);
    if (direct) {
        // direct binning (rasterizer_preprocess.hip): count -> scan (= the tile ranges) -> emit into the segments, then
        // the per-tile sort by (depth, index): same final lists as the global stable sort
        uint32_t* tile_counts = (uint32_t*)(bbuf + B.sort_temp);
        StageTimer t_dup(stream, ST_DUPKEYS);
        launch_tile_binning(stream, P, T, g_means2D, g_depths, radii_p, g_tiles, g_block, gx, gy, tile_counts, tile_counts + T,
                            ranges, (uint32_t*)(gbuf + G.point_offsets), keys_u, (unsigned long long*)(gbuf + G.total), a.capacity,
                            a.overflow_flag, a.overflow_count, t->fused_front, order, tile_sort_small_cap(), big_list, big_count);
        check_launch(stream, debug, "tile_binning");
        t_dup.stop();
        StageTimer t_sort(stream, ST_SORT);
        if (!t->fused_front) {
            launch_tile_order(stream, T, ranges, order, tile_sort_small_cap(), big_list, big_count);
            check_launch(stream, debug, "tile_order");
        }
        launch_tile_sort(stream, T, order, ranges, big_list, big_count, keys, vals, keys_u, true);
        check_launch(stream, debug, "tile_sort");
        t_sort.stop();
        return R3DG_OK;
    }
    // both radix orderings start from the reference's (tile | depth) keys, emitted in Gaussian order
    StageTimer t_dup(stream, ST_DUPKEYS);
    launch_duplicate_with_keys(stream, P, g_means2D, g_depths, g_tiles, g_block, (uint32_t*)(gbuf + G.point_offsets),
                               keys_u, vals_u, radii_p, gx, gy);
    check_launch(stream, debug, "duplicate_with_keys");
    t_dup.stop();
    const int bit = (int)higher_msb((uint32_t)T);
    StageTimer t_sort(stream, ST_SORT);
    if (opt(R3DG_OPT_TILE_BINNING)) {
        // stable partition by tile id (one radix pass over the tile bits), then a per-tile depth sort in LDS: same
        // final order as the global 44-bit sort (radix_sort.hip)
        sort_pairs_range(stream, (size_t)R, keys_u, vals_u, keys, vals, 32, 32 + bit, bbuf + B.sort_temp, debug,
                         /*stable=*/false);
        R3DG_HIP(hipMemsetAsync(ranges, 0, (size_t)T * 8, stream));
        launch_identify_tile_ranges(stream, R, keys, ranges);
        check_launch(stream, debug, "identify_tile_ranges");
        launch_tile_order(stream, T, ranges, order, tile_sort_small_cap(), big_list, big_count);
        check_launch(stream, debug, "tile_order");
        launch_tile_sort(stream, T, order, ranges, big_list, big_count, keys, vals, keys_u, false);
        check_launch(stream, debug, "tile_sort");
        t_sort.stop();
    } else {
        sort_pairs(stream, (size_t)R, keys_u, vals_u, keys, vals, 32 + bit, bbuf + B.sort_temp, debug);
        t_sort.stop();

        StageTimer t_rng(stream, ST_RANGES);
        R3DG_HIP(hipMemsetAsync(ranges, 0, (size_t)T * 8, stream));
        launch_identify_tile_ranges(stream, R, keys, ranges);
        check_launch(stream, debug, "identify_tile_ranges");
        t_rng.stop();
        if (opt(R3DG_OPT_TILE_ORDER)) {
            launch_tile_order(stream, T, ranges, order, 0u, nullptr, nullptr);
            check_launch(stream, debug, "tile_order");
        }
    }
    return R3DG_OK;
}

// The tile forward (K8) over the lists enqueue_ordering made and, where asked for, the pseudo-normals (K9/K10) behind it.
static void render_tiles(const ForwardTicket* t, hipStream_t stream)
{
    const r3dg_raster_scene& s = t->a.scene;
    const r3dg_raster_outputs& o = t->a.out;
    const GeometryLayout& G = t->v.G;
    const ImageLayout& I = t->v.I;
    const bool debug = o.debug != 0;
    StageTimer t_rf(stream, ST_RENDER_FWD);
    launch_render_forward(stream, s.width, s.height, s.S,
                          opt(R3DG_OPT_TILE_ORDER) ? (uint32_t*)(t->ibuf + I.tile_order) : nullptr,
                          (uint32_t*)(t->ibuf + I.ranges), t->point_list, (const float*)(t->gbuf + G.splat), s.d_features,
                          (float*)(t->ibuf + I.final_T), (uint32_t*)(t->ibuf + I.n_contrib), s.d_background, o.d_out_color,
                          o.d_out_opacity, o.d_out_depth, o.d_out_feature, o.d_out_weights);
    check_launch(stream, debug, "render_forward");
    t_rf.stop();
    if (o.compute_pseudo_normal) {
        StageTimer t_n(stream, ST_NORMAL);
        launch_pseudo_normal(stream, s.width, s.height, s.d_viewmatrix, t->focal_x, t->focal_y, s.cx, s.cy, o.d_out_opacity,
                             o.d_out_depth, o.d_out_normal, o.d_out_surface_xyz, debug);
        t_n.stop();
    }
}

static int forward_begin_impl(const ForwardArgs& a, void** ticket_out)
{
    if (!ticket_out) return invalid("rasterize_forward_begin: null ticket pointer");
    *ticket_out = nullptr;
    const r3dg_raster_scene& s = a.scene;
    if (s.P < 0 || s.width <= 0 || s.height <= 0) return invalid("rasterize_forward: bad P/width/height");
    if (s.S < 0 || s.S > R3DG_MAX_S_FWD) return invalid("rasterize_forward: feature channels S must be in [0,36]");
    if (!a.geometry_alloc || !a.binning_alloc || !a.image_alloc) return invalid("rasterize_forward: null resize callback");
    if (s.d_shs == nullptr && s.d_colors_precomp == nullptr)
        return invalid("rasterize_forward: provide SHs or precomputed colours");
    if (s.d_shs != nullptr && s.d_colors_precomp == nullptr && (s.M < (s.D + 1) * (s.D + 1) || s.D > 3 || s.D < 0))
        return invalid("rasterize_forward: SH degree/coefficients mismatch");
    if (s.d_cov3D_precomp == nullptr && (s.d_scales == nullptr || s.d_rotations == nullptr))
        return invalid("rasterize_forward: provide scales+rotations or a precomputed 3D covariance");
    if (s.P == 0) return R3DG_OK;                  // no ticket: nothing was launched (finish accepts NULL)

    return guarded([&]() -> int {
        hipStream_t stream = (hipStream_t)a.stream;
        const bool debug = a.out.debug != 0;
        const RasterView v = RasterView::make(s.P, s.width, s.height);
        const GeometryLayout& G = v.G;
        char* gbuf = (char*)a.geometry_alloc(a.user, G.bytes);
        char* ibuf = (char*)a.image_alloc(a.user, v.I.bytes);
        if (!gbuf || !ibuf) { set_error("rasterize_forward: resize callback returned NULL"); return R3DG_EALLOC; }

        ForwardTicket* t = ticket_acquire();
        struct Release { ForwardTicket* t; ~Release() { if (t) ticket_release(t); } } on_error{t};      // (a launch check may throw)
        t->a = a;
        t->v = v;
        t->focal_y = s.height / (2.0f * s.tan_fovy);
        t->focal_x = s.width / (2.0f * s.tan_fovx);
        t->radii_p = a.out.d_radii ? a.out.d_radii : (int*)(gbuf + G.radii);
        t->gbuf = gbuf;
        t->ibuf = ibuf;
        t->bbuf = nullptr;
        t->fused_front = false;
        t->point_list = nullptr;
        // bounded with an ordering stream: the projection goes there too, behind everything the caller has queued on `stream`
        // so far -- the whole front end of the rasterizer then runs beside what the caller queues on `stream` next, and
        // r3dg_rasterize_forward_finish_bounded joins it
        const hipStream_t order_stream = a.capacity >= 0 && a.ordering_stream ? (hipStream_t)a.ordering_stream : stream;
        stream_wait_stream(order_stream, stream);
        // bounded + direct binning: the front end is one chain whose launches do not depend on the count, so three of them fold
        // into their neighbours (launch_tile_binning `fused`): the projection zeroes the tile counters, the tile scan also scans
        // the projection's block sums, an extra block of the emit kernel orders the tiles
        uint32_t* zero_words = nullptr;
        int zero_n = 0;
        if (a.capacity >= 0 && direct_binning_usable((long long)v.T)) {
            BinningLayout B = BinningLayout::make((size_t)a.capacity);
            t->bbuf = (char*)a.binning_alloc(a.user, B.bytes);
            if (!t->bbuf) { set_error("rasterize_forward: binning resize callback returned NULL"); return R3DG_EALLOC; }
            t->fused_front = true;
            zero_words = (uint32_t*)(t->bbuf + B.sort_temp);
            zero_n = (int)v.T;
        }
        unsigned long long* g_total = (unsigned long long*)(gbuf + G.total);
        StageTimer t_pre(order_stream, ST_PREPROCESS);
        launch_preprocess(order_stream, s.P, s.D, s.M, s.d_means3D, s.d_scales, s.scale_modifier, s.d_rotations, s.d_opacities,
                          s.d_shs, (uint8_t*)(gbuf + G.clamped), s.d_cov3D_precomp, s.d_colors_precomp, s.d_viewmatrix,
                          s.d_projmatrix, s.d_campos, s.width, s.height, s.tan_fovx, s.tan_fovy, t->focal_x, t->focal_y, t->radii_p,
                          (float*)(gbuf + G.means2D), (float*)(gbuf + G.depths), (float*)(gbuf + G.cov3D),
                          (float*)(gbuf + G.rgb), (float*)(gbuf + G.conic_opacity), (float*)(gbuf + G.splat), v.gx, v.gy,
                          (uint32_t*)(gbuf + G.tiles_touched), (uint32_t*)(gbuf + G.block_sums), g_total, !t->fused_front,
                          zero_words, zero_n);
        check_launch(order_stream, debug, "preprocess");
        t_pre.stop();

        if (a.capacity >= 0) {
            // bounded: nobody reads the count; the ordering follows the projection right away
            const int st_order = enqueue_ordering(t, order_stream, (int)a.capacity);
            if (st_order != R3DG_OK) return st_order;
            R3DG_HIP(hipEventRecord(t->ordered, order_stream));
        } else {
            // the one device->host read-back of the forward (reference rasterizer_impl.cu:291), asynchronous here
            R3DG_HIP(hipMemcpyAsync(t->host_total, g_total, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
            R3DG_HIP(hipEventRecord(t->ready, stream));
        }
        on_error.t = nullptr;
        *ticket_out = t;
        return R3DG_OK;
    });
}

}  // namespace r3dg

using namespace r3dg;

extern "C" {

int r3dg_bounded_forward_supported(int width, int height)
{
    if (width <= 0 || height <= 0) return 0;
    const long long gx = (width + R3DG_TILE_X - 1) / R3DG_TILE_X, gy = (height + R3DG_TILE_Y - 1) / R3DG_TILE_Y;
    return direct_binning_usable(gx * gy) ? 1 : 0;
}

size_t r3dg_geometry_state_bytes(int P) { return GeometryLayout::make((size_t)(P > 0 ? P : 0)).bytes; }
size_t r3dg_image_state_bytes(int width, int height)
{
    const size_t T = (size_t)((width + 15) / 16) * ((height + 15) / 16);
    return ImageLayout::make((size_t)width * height, T).bytes;
}
size_t r3dg_binning_state_bytes(int64_t R) { return BinningLayout::make((size_t)(R > 0 ? R : 0)).bytes; }

int r3dg_geometry_state_offsets(int P, size_t* o)
{
    GeometryLayout L = GeometryLayout::make((size_t)P);
    o[0] = L.depths; o[1] = L.clamped; o[2] = L.radii; o[3] = L.means2D; o[4] = L.cov3D; o[5] = L.conic_opacity;
    o[6] = L.rgb; o[7] = L.tiles_touched; o[8] = L.point_offsets;
    return R3DG_OK;
}
size_t r3dg_geometry_state_total_offset(int P)
{
    return GeometryLayout::make((size_t)(P < 0 ? 0 : P)).total;
}
int r3dg_image_state_offsets(int width, int height, size_t* o)
{
    const size_t T = (size_t)((width + 15) / 16) * ((height + 15) / 16);
    ImageLayout L = ImageLayout::make((size_t)width * height, T);
    o[0] = L.final_T; o[1] = L.n_contrib; o[2] = L.ranges;
    return R3DG_OK;
}
int r3dg_binning_state_offsets(int64_t R, size_t* o)
{
    BinningLayout L = BinningLayout::make((size_t)R);
    o[0] = L.keys_unsorted; o[1] = L.keys; o[2] = L.vals_unsorted; o[3] = L.vals;
    return R3DG_OK;
}

int r3dg_rasterize_forward_begin(void* stream_, r3dg_alloc_fn geometry_alloc, r3dg_alloc_fn binning_alloc,
                                 r3dg_alloc_fn image_alloc, void* user, const r3dg_raster_scene* scene,
                                 const r3dg_raster_outputs* outputs, void** ticket_out)
{
    if (!scene || !outputs) return invalid("rasterize_forward_begin: null scene or outputs");
    return forward_begin_impl(ForwardArgs{stream_, geometry_alloc, binning_alloc, image_alloc, user, *scene, *outputs, -1, nullptr,
                                          nullptr, nullptr}, ticket_out);
}

int r3dg_rasterize_forward_begin_bounded(void* stream_, r3dg_alloc_fn geometry_alloc, r3dg_alloc_fn binning_alloc,
                                         r3dg_alloc_fn image_alloc, void* user, const r3dg_raster_scene* scene,
                                         const r3dg_raster_outputs* outputs, void* ordering_stream, long long capacity,
                                         float* overflow_flag, unsigned int* overflow_count, void** ticket_out)
{
    if (!scene || !outputs) return invalid("rasterize_forward_begin: null scene or outputs");
    if (capacity < 0 || capacity > 0x7fffffffll) return invalid("rasterize_forward (bounded): capacity must be in [0, 2^31)");
    return forward_begin_impl(ForwardArgs{stream_, geometry_alloc, binning_alloc, image_alloc, user, *scene, *outputs, capacity,
                                          overflow_flag, overflow_count, ordering_stream}, ticket_out);
}
int r3dg_rasterize_forward_finish_bounded(void* ticket_, void* main_stream_)
{
    if (!ticket_) return R3DG_OK;                // P == 0
    ForwardTicket* t = (ForwardTicket*)ticket_;
    if (t->a.capacity < 0) return invalid("rasterize_forward_finish_bounded: not a bounded ticket");
    const int st = guarded([&]() -> int {
        const hipStream_t stream = (hipStream_t)main_stream_;
        // join: the tile kernel needs the ordering (begin's stream) AND whatever the caller queued on `stream` (feature rows)
        R3DG_HIP(hipStreamWaitEvent(stream, t->ordered, 0));
        render_tiles(t, stream);
        return R3DG_OK;
    });
    ticket_release(t);
    return st;
}

int r3dg_rasterize_forward_finish(void* ticket_, int* num_rendered_out)
{
    return r3dg_rasterize_forward_finish_on(ticket_, nullptr, num_rendered_out);
}

int r3dg_rasterize_forward_finish_on(void* ticket_, void* ordering_stream_, int* num_rendered_out)
{
    if (num_rendered_out) *num_rendered_out = 0;
    if (!ticket_) return R3DG_OK;                // P == 0
    ForwardTicket* t = (ForwardTicket*)ticket_;
    if (t->a.capacity >= 0) return invalid("rasterize_forward_finish: bounded ticket (use r3dg_rasterize_forward_finish_bounded)");
    const int st = guarded([&]() -> int {
        const hipStream_t main_stream = (hipStream_t)t->a.stream;
        // instance ordering (K5-K7) may run on its own stream: it depends on the projection only, so it can overlap the
        // kernels the caller queued on the main stream after _begin (the shading that produces the feature rows)
        const hipStream_t order_stream = ordering_stream_ ? (hipStream_t)ordering_stream_ : main_stream;

        R3DG_HIP(hipEventSynchronize(t->ready));
        const unsigned long long total = *t->host_total;
        if (order_stream != main_stream) R3DG_HIP(hipStreamWaitEvent(order_stream, t->ready, 0));
        if (total > 0x7fffffffull) { set_error("rasterize_forward: num_rendered exceeds 2^31-1"); return R3DG_EINVAL; }
        const int R = (int)total;

        const int st_order = enqueue_ordering(t, order_stream, R);
        if (st_order != R3DG_OK) return st_order;
        stream_wait_stream(main_stream, order_stream);          // join: the tile kernel needs the ordering AND the feature rows
        render_tiles(t, main_stream);
        if (num_rendered_out) *num_rendered_out = R;
        return R3DG_OK;
    });
    ticket_release(t);
    return st;
}

// (the reference's list; parameters carry the names of the struct fields they fill, in the structs' order of declaration)
int r3dg_rasterize_forward(void* stream_, r3dg_alloc_fn geometry_alloc, r3dg_alloc_fn binning_alloc,
                           r3dg_alloc_fn image_alloc, void* user, int P, int S, int D, int M,
                           const float* d_background, int width, int height, const float* d_means3D, const float* d_shs,
                           const float* d_colors_precomp, const float* d_features, const float* d_opacities,
                           const float* d_scales, float scale_modifier, const float* d_rotations,
                           const float* d_cov3D_precomp, const float* d_viewmatrix, const float* d_projmatrix,
                           const float* d_campos, float tan_fovx, float tan_fovy, float cx, float cy, int prefiltered,
                           int compute_pseudo_normal, float* d_out_color, float* d_out_opacity, float* d_out_depth,
                           float* d_out_feature, float* d_out_normal, float* d_out_surface_xyz, float* d_out_weights,
                           int32_t* d_radii, int debug, int* num_rendered_out)
{
    if (num_rendered_out) *num_rendered_out = 0;
    const r3dg_raster_scene scene = {P, S, D, M, width, height,
                                     d_background, d_means3D, d_shs, d_colors_precomp, d_features, d_opacities, d_scales,
                                     scale_modifier, d_rotations, d_cov3D_precomp, d_viewmatrix, d_projmatrix, d_campos,
                                     tan_fovx, tan_fovy, cx, cy};
    const r3dg_raster_outputs outputs = {prefiltered, compute_pseudo_normal, debug,
                                         d_out_color, d_out_opacity, d_out_depth, d_out_feature, d_out_normal, d_out_surface_xyz,
                                         d_out_weights, d_radii};
    void* ticket = nullptr;
    const int st = r3dg_rasterize_forward_begin(stream_, geometry_alloc, binning_alloc, image_alloc, user, &scene, &outputs, &ticket);
    if (st != R3DG_OK) return st;
    return r3dg_rasterize_forward_finish(ticket, num_rendered_out);
}

// the optional list of feature channels whose gradients the caller wants (n < 0: all S of them)
static int check_active_features(const char* name, int n, const int* list, int S)
{
    if (n < 0) return R3DG_OK;
    if (n > S || !list) return invalid(std::string(name) + ": bad active feature list");
    for (int i = 0; i < n; i++)
        if (list[i] < 0 || list[i] >= S) return invalid(std::string(name) + ": active feature index out of range");
    return R3DG_OK;
}

// the backward behind r3dg_rasterize_backward[_split]: `adam` != nullptr: the geometry kernel applies the SH colour group's Adam
// and does not write dL_dsh; `records_out` != nullptr: no scatter pass -- the geometry kernel reads the gradient record rows in
// place, the rows and their layout are handed to the caller, whose kernels read the rest; *supported_out = 0 and nothing enqueued
// where the instance has no 16-float rows (the entry point has reset the three outputs)
static int backward_split_impl(void* stream_, void* geometry_stream_, const r3dg_raster_scene& s, const r3dg_raster_backward& c,
                               const ShAdamArgs* adam, void** records_out, int* layout_out, int* supported_out)
{
    if (s.P < 0 || s.width <= 0 || s.height <= 0 || c.R < 0) return invalid("rasterize_backward: bad P/R/width/height");
    if (s.S < 0 || s.S > R3DG_MAX_S_BWD) return invalid("rasterize_backward: feature channels S must be in [0,36]");
    if (s.P == 0) return R3DG_OK;
    if (!c.d_geom_buffer || !c.d_img_buffer || (c.R > 0 && !c.d_binning_buffer)) return invalid("rasterize_backward: null state buffer");
    if (!c.d_dL_dpix || !c.d_dL_dpix_o || (s.S > 0 && !c.d_dL_dpix_f)) return invalid("rasterize_backward: null upstream gradient");
    if (int e = check_active_features("rasterize_backward", c.n_active_features, c.active_features, s.S)) return e;
    const bool in_place = records_out != nullptr;
    if (in_place) {
        const GradRecordLayout L = render_backward_layout(s.S, c.n_active_features, c.active_features, c.d_dL_dpix_d != nullptr,
                                                          c.backward_geometry);
        if (L.nvp != 16) return R3DG_OK;                 // (not an error: the caller calls again without record outputs)
        *supported_out = 1;
    }

    return guarded([&]() -> int {
        hipStream_t stream = (hipStream_t)stream_;
        const bool debug = c.debug != 0;
        const int P = s.P, S = s.S, width = s.width, height = s.height;
        const float focal_y = height / (2.0f * s.tan_fovy);
        const float focal_x = width / (2.0f * s.tan_fovx);
        const RasterView v = RasterView::make(P, width, height);
        const GeometryLayout& G = v.G;
        const ImageLayout& I = v.I;
        BinningLayout B = BinningLayout::make((size_t)c.R);
        const char* gbuf = (const char*)c.d_geom_buffer;
        const char* ibuf = (const char*)c.d_img_buffer;
        const char* bbuf = (const char*)c.d_binning_buffer;
        const int* radii_p = c.d_radii ? c.d_radii : (const int*)(gbuf + G.radii);

        float* rec = nullptr;
        GradRecordLayout layout;
        if (in_place) {
            StageTimer t_rb(stream, ST_RENDER_BWD);
            rec = launch_render_backward_fill(stream, P, width, height, S, c.n_active_features, c.active_features,
                                              opt(R3DG_OPT_TILE_ORDER) ? (const uint32_t*)(ibuf + I.tile_order) : nullptr,
                                              (const uint32_t*)(ibuf + I.ranges), (const uint32_t*)(bbuf + B.vals), s.d_background,
                                              (const float*)(gbuf + G.splat), s.d_features, (const float*)(ibuf + I.final_T),
                                              (const uint32_t*)(ibuf + I.n_contrib), c.d_dL_dpix, c.d_dL_dpix_o, c.d_dL_dpix_d,
                                              c.d_dL_dpix_f, c.backward_geometry, c.R > 0, &layout);
            check_launch(stream, debug, "render_backward");
            t_rb.stop();
            *records_out = rec;
            std::memcpy(layout_out, &layout, sizeof(layout));
        } else if (c.R > 0) {
            StageTimer t_rb(stream, ST_RENDER_BWD);
            launch_render_backward(stream, P, width, height, S, c.n_active_features, c.active_features,
                                   opt(R3DG_OPT_TILE_ORDER) ? (const uint32_t*)(ibuf + I.tile_order) : nullptr,
                                   (const uint32_t*)(ibuf + I.ranges),
                                   (const uint32_t*)(bbuf + B.vals), s.d_background, (const float*)(gbuf + G.splat),
                                   s.d_features, (const float*)(ibuf + I.final_T), (const uint32_t*)(ibuf + I.n_contrib),
                                   c.d_dL_dpix, c.d_dL_dpix_o, c.d_dL_dpix_d, c.d_dL_dpix_f, c.d_dL_dmean2D, c.d_dL_dconic,
                                   c.d_dL_dopacity, c.d_dL_dcolor, c.d_dL_dfeature, c.backward_geometry);
            check_launch(stream, debug, "render_backward");
            t_rb.stop();
        } else {
            // nothing was rendered: the five per-Gaussian outputs the tile pass writes are zero
            R3DG_HIP(hipMemsetAsync(c.d_dL_dmean2D, 0, (size_t)P * 3 * sizeof(float), stream));
            R3DG_HIP(hipMemsetAsync(c.d_dL_dconic, 0, (size_t)P * 4 * sizeof(float), stream));
            R3DG_HIP(hipMemsetAsync(c.d_dL_dopacity, 0, (size_t)P * sizeof(float), stream));
            R3DG_HIP(hipMemsetAsync(c.d_dL_dcolor, 0, (size_t)P * 3 * sizeof(float), stream));
            if (S > 0 && c.d_dL_dfeature != nullptr)
                R3DG_HIP(hipMemsetAsync(c.d_dL_dfeature, 0, (size_t)P * S * sizeof(float), stream));
        }
        const float* cov3D_ptr = s.d_cov3D_precomp != nullptr ? s.d_cov3D_precomp : (const float*)(gbuf + G.cov3D);
        // the per-Gaussian geometry backward may run on a second stream, ordered after the tile kernel by an event
        hipStream_t gstream = (hipStream_t)geometry_stream_;
        stream_wait_stream(gstream, stream);
        stream = gstream;
        StageTimer t_pb(stream, ST_PREPROCESS_BWD);
        launch_preprocess_backward(stream, P, s.D, s.M, s.d_means3D, radii_p, s.d_colors_precomp == nullptr ? s.d_shs : nullptr,
                                   (const uint8_t*)(gbuf + G.clamped), s.d_cov3D_precomp == nullptr ? s.d_scales : nullptr,
                                   s.d_rotations, s.scale_modifier, cov3D_ptr, s.d_viewmatrix, s.d_projmatrix, focal_x, focal_y,
                                   s.tan_fovx, s.tan_fovy, s.d_campos, c.d_dL_dmean2D, c.d_dL_dconic,
                                   (const float*)(gbuf + G.conic_opacity), width, height, c.d_dL_dmean3D, c.d_dL_dcolor,
                                   c.d_dL_dcov3D, c.d_dL_dsh, c.d_dL_dscale, c.d_dL_drot, adam, rec, in_place ? &layout : nullptr);
        check_launch(stream, debug, "preprocess_backward");
        t_pb.stop();
        return R3DG_OK;
    });
}

// (the reference's list, as r3dg_rasterize_forward above)
int r3dg_rasterize_backward(void* stream_, int P, int S, int D, int M, int R, const float* d_background, int width,
                            int height, const float* d_means3D, const float* d_shs, const float* d_features,
                            const float* d_colors_precomp, const float* d_scales, float scale_modifier,
                            const float* d_rotations, const float* d_cov3D_precomp, const float* d_viewmatrix,
                            const float* d_projmatrix, const float* d_campos, float tan_fovx, float tan_fovy,
                            const int32_t* d_radii, const void* d_geom_buffer, const void* d_binning_buffer,
                            const void* d_img_buffer, const float* d_dL_dpix, const float* d_dL_dpix_o,
                            const float* d_dL_dpix_d, const float* d_dL_dpix_f, float* d_dL_dmean2D, float* d_dL_dconic,
                            float* d_dL_dopacity, float* d_dL_dcolor, float* d_dL_dfeature, float* d_dL_dmean3D,
                            float* d_dL_dcov3D, float* d_dL_dsh, float* d_dL_dscale, float* d_dL_drot,
                            int backward_geometry, int debug)
{
    const r3dg_raster_scene scene = {P, S, D, M, width, height,
                                     d_background, d_means3D, d_shs, d_colors_precomp, d_features, /*d_opacities=*/nullptr, d_scales,
                                     scale_modifier, d_rotations, d_cov3D_precomp, d_viewmatrix, d_projmatrix, d_campos,
                                     tan_fovx, tan_fovy, /*cx, cy=*/0.0f, 0.0f};
    const r3dg_raster_backward call = {R, d_radii, d_geom_buffer, d_binning_buffer, d_img_buffer,
                                       d_dL_dpix, d_dL_dpix_o, d_dL_dpix_d, d_dL_dpix_f,
                                       d_dL_dmean2D, d_dL_dconic, d_dL_dopacity, d_dL_dcolor, d_dL_dfeature,
                                       d_dL_dmean3D, d_dL_dcov3D, d_dL_dsh, d_dL_dscale, d_dL_drot,
                                       backward_geometry, debug, /*n_active_features=*/-1, /*active_features=*/nullptr};
    return backward_split_impl(stream_, stream_, scene, call, nullptr, nullptr, nullptr, nullptr);
}

int r3dg_rasterize_backward_sh_adam_supported(int M) { return preprocess_backward_applies_adam(M) ? 1 : 0; }

// r3dg_rasterize_backward_split's arguments behind `sh_adam`, checked and made into what the geometry kernel takes
static int make_sh_adam(const r3dg_raster_scene& s, const r3dg_adam_group& g, float beta1, float beta2, float eps, int step,
                        float grad_scale, const float* skip_flag, ShAdamArgs* adam)
{
    const std::string me = "rasterize_backward_split (sh_adam): ";
    if (s.P < 0 || s.M < 0) return invalid(me + "bad P/M");
    if (step < 1) return invalid(me + "step counts from 1");
    if (!preprocess_backward_applies_adam(s.M)) return invalid(me + "no such kernel for this M / with STAGE_SH_ROWS off");
    if (!s.d_shs || s.d_colors_precomp) return invalid(me + "needs SH input");
    if (g.param != s.d_shs || g.n != (uint64_t)s.P * 3 * (uint64_t)s.M || g.n >= (1ull << 32))
        return invalid(me + "the group must be the [P,M,3] SH tensor itself (below 2^32 elements)");
    if (s.P > 0 && (!g.exp_avg || !g.exp_avg_sq || (((uintptr_t)g.param | (uintptr_t)g.exp_avg | (uintptr_t)g.exp_avg_sq) & 15)))
        return invalid(me + "null or unaligned buffer in group");
    const AdamBias b = adam_bias(beta1, beta2, step);
    *adam = ShAdamArgs{g, beta1, beta2, eps, b.bias1, b.inv_sqrt_bias2, grad_scale, skip_flag};
    return R3DG_OK;
}

int r3dg_rasterize_backward_split(void* stream_, void* geometry_stream_, const r3dg_raster_scene* scene,
                                  const r3dg_raster_backward* call, const r3dg_adam_group* sh_adam, float beta1, float beta2,
                                  float eps, int step, float grad_scale, const float* skip_flag, void** records_out,
                                  int* layout_out, int* supported_out)
{
    const std::string me = "rasterize_backward_split: ";
    if (records_out ? !layout_out || !supported_out : layout_out || supported_out)
        return invalid(me + "records, layout and supported outputs go together");
    if (records_out) {
        *records_out = nullptr;
        *supported_out = 0;
    }
    if (!scene || !call) return invalid(me + "null scene or call");
    if (records_out && scene->P > 0 && !call->d_dL_dmean2D) return invalid(me + "null dL_dmean2D");
    ShAdamArgs adam = {};
    if (sh_adam)
        if (int e = make_sh_adam(*scene, *sh_adam, beta1, beta2, eps, step, grad_scale, skip_flag, &adam)) return e;
    return backward_split_impl(stream_, geometry_stream_, *scene, *call, sh_adam ? &adam : nullptr, records_out, layout_out,
                               supported_out);
}

int r3dg_gradient_records_scatter(void* stream_, int P, int S, float* records, const int* layout_, float* dL_dmean2D,
                                  float* dL_dconic, float* dL_dopacity, float* dL_dcolor, float* dL_dfeature)
{
    if (P < 0 || S < 0 || S > R3DG_MAX_S_BWD) return invalid("gradient_records_scatter: bad P/S");
    if (P == 0) return R3DG_OK;
    if (!records || !layout_ || !dL_dmean2D || !dL_dconic || !dL_dopacity || !dL_dcolor || (S > 0 && !dL_dfeature))
        return invalid("gradient_records_scatter: null buffer");
    GradRecordLayout L;
    std::memcpy(&L, layout_, sizeof(L));
    if (!gradient_record_layout_valid(L, S)) return invalid("gradient_records_scatter: not a gradient record layout");
    return guarded([&]() -> int {
        launch_gradient_records_scatter((hipStream_t)stream_, P, S, records, L, dL_dmean2D, dL_dconic, dL_dopacity, dL_dcolor,
                                        dL_dfeature);
        check_launch((hipStream_t)stream_, false, "gradient_records_scatter");
        return R3DG_OK;
    });
}

int r3dg_rasterize_backward_features(void* stream_, int P, int S, int R, int width, int height, const void* geom_buffer,
                                     const void* binning_buffer, const void* img_buffer, const float* dL_dpix_f,
                                     float* dL_dfeature, int n_active_features, const int* active_features, int debug_)
{
    if (P < 0 || width <= 0 || height <= 0 || R < 0) return invalid("rasterize_backward_features: bad P/R/width/height");
    if (S <= 0 || S > R3DG_MAX_S_BWD) return invalid("rasterize_backward_features: feature channels S must be in [1,36]");
    if (P == 0 || R == 0) return R3DG_OK;
    if (!geom_buffer || !img_buffer || !binning_buffer || !dL_dpix_f || !dL_dfeature)
        return invalid("rasterize_backward_features: null buffer");
    if (int e = check_active_features("rasterize_backward_features", n_active_features, active_features, S)) return e;
    return guarded([&]() -> int {
        hipStream_t stream = (hipStream_t)stream_;
        const RasterView v = RasterView::make(P, width, height);
        const GeometryLayout& G = v.G;
        const ImageLayout& I = v.I;
        BinningLayout B = BinningLayout::make((size_t)R);
        const char* gbuf = (const char*)geom_buffer;
        const char* ibuf = (const char*)img_buffer;
        const char* bbuf = (const char*)binning_buffer;
        StageTimer t_rb(stream, ST_RENDER_BWD);
        launch_render_backward_features(stream, width, height, S, n_active_features, active_features,
                                        opt(R3DG_OPT_TILE_ORDER) ? (const uint32_t*)(ibuf + I.tile_order) : nullptr,
                                        (const uint32_t*)(ibuf + I.ranges), (const uint32_t*)(bbuf + B.vals),
                                        (const float*)(gbuf + G.splat), (const float*)(ibuf + I.final_T),
                                        (const uint32_t*)(ibuf + I.n_contrib), dL_dpix_f, dL_dfeature);
        check_launch(stream, debug_ != 0, "render_backward_features");
        t_rb.stop();
        return R3DG_OK;
    });
}

int r3dg_mark_visible(void* stream_, int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                      uint8_t* present)
{
    (void)projmatrix;
    if (P < 0) return invalid("mark_visible: bad P");
    if (P == 0) return R3DG_OK;
    return guarded([&]() -> int {
        launch_mark_visible((hipStream_t)stream_, P, means3D, viewmatrix, present);
        check_launch((hipStream_t)stream_, false, "mark_visible");
        return R3DG_OK;
    });
}

size_t r3dg_sort_temp_bytes(int64_t n) { return sort_temp_bytes((size_t)(n > 0 ? n : 0)); }

int r3dg_sort_pairs(void* stream_, int64_t n, uint64_t* keys_in, uint32_t* vals_in, uint64_t* keys_out,
                    uint32_t* vals_out, int end_bit, void* temp)
{
    if (n < 0 || end_bit < 1 || end_bit > 64) return invalid("sort_pairs: bad n/end_bit");
    if (n == 0) return R3DG_OK;
    return guarded([&]() -> int {
        sort_pairs((hipStream_t)stream_, (size_t)n, keys_in, vals_in, keys_out, vals_out, end_bit, temp, false);
        return R3DG_OK;
    });
}

}  // extern "C"
