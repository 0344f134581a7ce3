// C ABI of libr3dg_hip.so (declared in include/r3dg_hip.h), the part that belongs to no one domain: error plumbing, library
// scratch, tuning options and option contexts, per-stage profiling, stream joins and the small measurement kernels.
#include "capi_internal.hpp"

#include <map>
#include <mutex>
#include <new>
#include <tuple>
#include <vector>

namespace r3dg {

static thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }

// ---- tuning / experiment knobs; not part of the drop-in surface (include/r3dg_hip.h "r3dg_option") ----
// One row per member of enum r3dg_option, in its order: default and accepted range.
struct OptionRow { int id, def, lo, hi; };
constexpr OptionRow kOptions[] = {
    {R3DG_OPT_TILE_ORDER, 1, 0, 1},         // 1: longest-tile-first block order, 0: XCD-contiguous natural order
    {R3DG_OPT_CULL, 1, 0, 1},               // conservative per-block cull of the staged entries (results do not depend on it)
    // 2: instances emitted straight into their tile's segment + per-tile LDS sort; 1: emitted in Gaussian order,
    // radix-partitioned by tile, per-tile LDS sort; 0: the reference's global (tile|depth) radix sort
    {R3DG_OPT_TILE_BINNING, 2, 0, 2},
    {R3DG_OPT_BINNING_BLOCK_K, 2, 1, 4},    // (measured at 2M Gaussians too: 2 / 3 / 4 -> 163 / 156 / 161 it/s, no trend)
    {R3DG_OPT_STAGE_SH_ROWS, 1, 0, 1},      // 1 = SH / dL_dsh rows through LDS, 0 = direct per-thread walks
    {R3DG_OPT_SHADE_FWD_BLOCKS_PER_CU, 0, 0, 8},    // persistent row blocks per CU, 0 = all that fit
    // 1 = packed records, phase-separated persistent waves; 0 = thread per ray over the reference's tables
    {R3DG_OPT_TRACE_FORMULATION, 1, 0, 1},
    {R3DG_OPT_TRACE_REFILL, 16, 1, 64},     // a wave pulls new rays when at least this many lanes are idle (or all of them)
    {R3DG_OPT_TRACE_NODE_WEIGHT, 1, 1, 15},
    {R3DG_OPT_TRACE_LEAF_WEIGHT, 1, 1, 15},
    // CUs the persistent kernels (shading forward / backward, visibility trace) leave unoccupied so that a collective running
    // beside them on another stream (RCCL's workgroups need LDS and registers on SOME CU) is not serialised behind them:
    // their grids are sized for (CUs - this).  0 on a single GPU; set by the data-parallel iteration.
    {R3DG_OPT_RESERVE_CUS, 0, 0, 128},
    {R3DG_OPT_TRACE_COUNT_VISITS, 0, 0, 1},
    {R3DG_OPT_BWD_LEAN, 1, 0, 1},
};
constexpr bool option_rows_in_enum_order()
{
    for (int i = 0; i < (int)(sizeof(kOptions) / sizeof(kOptions[0])); i++)
        if (kOptions[i].id != i) return false;
    return true;
}
static_assert(sizeof(kOptions) / sizeof(kOptions[0]) == R3DG_OPT_COUNT && option_rows_in_enum_order(),
              "kOptions needs one row per r3dg_option, in the order of the enum");

static bool option_known(int option) { return option >= 0 && option < R3DG_OPT_COUNT; }
static bool option_in_range(int option, int value) { return value >= kOptions[option].lo && value <= kOptions[option].hi; }

// ---- option contexts: per-object settings instead of process-global ones ----
// The values that differ from the defaults: one set per context, and one for the process (r3dg_set_option).
struct OptionContext {
    int value[R3DG_OPT_COUNT];
    unsigned int set_mask;
};
static OptionContext g_process_options;         // (zero-initialised: nothing set)
static thread_local const OptionContext* tl_context = nullptr;

int opt(int option)
{
    const OptionContext* c = tl_context;
    if (c != nullptr && ((c->set_mask >> option) & 1u)) return c->value[option];
    return (g_process_options.set_mask >> option) & 1u ? g_process_options.value[option] : kOptions[option].def;
}

int persistent_cus()
{
    int dev = 0, cus = 256;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    return cus > opt(R3DG_OPT_RESERVE_CUS) ? cus - opt(R3DG_OPT_RESERVE_CUS) : 1;
}

namespace {
struct ScratchBuf { void* p = nullptr; size_t cap = 0; };
std::mutex g_scratch_mu;
std::map<std::tuple<int, hipStream_t, int>, ScratchBuf> g_scratch;
}

void* stream_scratch(hipStream_t stream, int slot, size_t bytes)
{
    int dev = 0;
    R3DG_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_scratch_mu);
    ScratchBuf& b = g_scratch[std::make_tuple(dev, stream, slot)];
    if (b.cap < bytes) {
        // geometric growth: a scene that densifies outgrows its buffer O(log) times, not at every 12 % (each growth is a stream
        // synchronise + hipFree, a device-wide wait)
        const size_t want = b.p == nullptr ? bytes + bytes / 8 + 4096 : std::max(bytes + 4096, 2 * b.cap);
        if (b.p != nullptr) {
            R3DG_HIP(hipStreamSynchronize(stream));        // only this stream ever used the old buffer
            R3DG_HIP(hipFree(b.p));
            b.p = nullptr;
            b.cap = 0;
        }
        R3DG_HIP(hipMalloc(&b.p, want));
        b.cap = want;
    }
    return b.p;
}

static void release_all_scratch()
{
    R3DG_HIP(hipDeviceSynchronize());
    {
        std::lock_guard<std::mutex> lk(g_scratch_mu);
        for (auto& kv : g_scratch)
            if (kv.second.p != nullptr) (void)hipFree(kv.second.p);
        g_scratch.clear();
    }
    release_gradient_records();
}

// ---- per-stage timing ----
static int g_profiling = 0;
struct EventPair { hipEvent_t a, b; };
static std::vector<EventPair> g_events[ST_COUNT];
static std::mutex g_prof_mutex;

StageTimer::StageTimer(hipStream_t s_, int stage_) : s(s_), stage(stage_), on(g_profiling != 0)
{
    if (on) {
        R3DG_HIP(hipEventCreate(&a));
        R3DG_HIP(hipEventCreate(&b));
        R3DG_HIP(hipEventRecord(a, s));
    }
}
void StageTimer::stop()
{
    if (on) {
        R3DG_HIP(hipEventRecord(b, s));
        std::lock_guard<std::mutex> lk(g_prof_mutex);
        g_events[stage].push_back(EventPair{a, b});
        on = false;
    }
}

// Events come from a ring created once: creating and destroying one per call costs the host several microseconds, 8 such
// calls per iteration (651-656 it/s against 646 with per-call events).
// (hipEventReleaseToDevice on these events measured the same as the default system-scope release: 652-655 vs 656.)
void stream_wait_stream(hipStream_t waiter, hipStream_t signaller)
{
    if (waiter == signaller) return;
    constexpr int RING = 64;
    static std::mutex mu;
    static std::map<int, std::vector<hipEvent_t>> rings;
    static std::map<int, int> next;
    int dev = 0;
    R3DG_HIP(hipGetDevice(&dev));
    hipEvent_t ev;
    {
        std::lock_guard<std::mutex> lk(mu);
        std::vector<hipEvent_t>& r = rings[dev];
        if (r.empty()) {
            r.resize(RING);
            for (auto& e : r) R3DG_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
        int& i = next[dev];
        ev = r[i];
        i = (i + 1) % RING;
    }
    R3DG_HIP(hipEventRecord(ev, signaller));
    R3DG_HIP(hipStreamWaitEvent(waiter, ev, 0));
}

}  // namespace r3dg

using namespace r3dg;

extern "C" {

const char* r3dg_last_error(void) { return g_last_error.c_str(); }
int r3dg_release_scratch(void)
{
    return guarded([&]() {
        release_all_scratch();
        return R3DG_OK;
    });
}
int r3dg_version(void) { return 100; }
int r3dg_max_features_forward(void) { return R3DG_MAX_S_FWD; }
int r3dg_max_features_backward(void) { return R3DG_MAX_S_BWD; }

int r3dg_set_option(int option, int value)
{
    if (!option_known(option)) return invalid("set_option: unknown option");
    if (!option_in_range(option, value)) return invalid("set_option: value out of range");
    g_process_options.value[option] = value;
    g_process_options.set_mask |= 1u << option;
    return R3DG_OK;
}

int r3dg_get_option(int option, int* value)
{
    if (!option_known(option) || value == nullptr) return invalid("get_option: unknown option or null pointer");
    *value = r3dg::opt(option);              // (what a launch on this thread would see right now)
    return R3DG_OK;
}

void* r3dg_context_create(void)
{
    return new (std::nothrow) OptionContext();          // (value-initialised: nothing set)
}

void r3dg_context_destroy(void* ctx)
{
    if (tl_context == ctx) tl_context = nullptr;
    delete static_cast<OptionContext*>(ctx);
}

int r3dg_context_set_option(void* ctx, int option, int value)
{
    if (ctx == nullptr || !option_known(option)) return invalid("context_set_option: null context or unknown option");
    if (!option_in_range(option, value)) return invalid("context_set_option: value out of range");
    OptionContext* c = static_cast<OptionContext*>(ctx);
    c->value[option] = value;
    c->set_mask |= 1u << option;
    return R3DG_OK;
}

int r3dg_context_make_current(void* ctx, void** previous)
{
    if (previous != nullptr) *previous = const_cast<OptionContext*>(tl_context);
    tl_context = static_cast<const OptionContext*>(ctx);
    return R3DG_OK;
}

int r3dg_selftest_transpose_reduce(void* stream_, int N, int dpp, const float* d_in, float* d_out, int* d_chan,
                                   int* d_owner)
{
    if (N != 12 && N != 16 && N != 32 && N != 64) return invalid("selftest_transpose_reduce: N must be 12, 16, 32 or 64");
    return guarded([&]() -> int {
        launch_transpose_selftest((hipStream_t)stream_, N, dpp, d_in, d_out, d_chan, d_owner);
        check_launch((hipStream_t)stream_, true, "transpose_selftest");
        return R3DG_OK;
    });
}

// Per-stage HIP-event timing. r3dg_profile_enable(1) starts recording (and clears), r3dg_profile_read waits for
// the recorded events and returns, per stage, the summed milliseconds and the number of timed launches.
int r3dg_profile_enable(int on)
{
    std::lock_guard<std::mutex> lk(g_prof_mutex);
    for (int s = 0; s < ST_COUNT; s++) {
        for (auto& e : g_events[s]) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
        g_events[s].clear();
    }
    g_profiling = on;
    return R3DG_OK;
}
// suspend / resume the recording without discarding what was recorded (sampled profiling: the event pairs cost ~2 us of
// host time each, so a caller may time every n-th iteration only)
int r3dg_profile_pause(int paused)
{
    std::lock_guard<std::mutex> lk(g_prof_mutex);
    g_profiling = paused ? 0 : 1;
    return R3DG_OK;
}
int r3dg_profile_num_stages(void) { return ST_COUNT; }
const char* r3dg_profile_stage_name(int stage) { return (stage >= 0 && stage < ST_COUNT) ? kStageNames[stage] : ""; }
int r3dg_profile_read(double* ms_out, int* count_out)
{
    return guarded([&]() -> int {
        std::lock_guard<std::mutex> lk(g_prof_mutex);
        for (int s = 0; s < ST_COUNT; s++) {
            double total = 0;
            for (auto& e : g_events[s]) {
                R3DG_HIP(hipEventSynchronize(e.b));
                float ms = 0;
                R3DG_HIP(hipEventElapsedTime(&ms, e.a, e.b));
                total += ms;
            }
            ms_out[s] = total;
            count_out[s] = (int)g_events[s].size();
        }
        return R3DG_OK;
    });
}

int r3dg_stream_wait_stream(void* waiter, void* signaller)
{
    return guarded([&]() -> int {
        stream_wait_stream((hipStream_t)waiter, (hipStream_t)signaller);
        return R3DG_OK;
    });
}

// one wave that does nothing for `us` microseconds of the device's constant-rate wall clock (s_memrealtime)
__global__ void __launch_bounds__(64) spin_kernel(unsigned long long ticks)
{
    const unsigned long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
}

// one thread: *dst = *src (dst: device address of pinned host memory)
__global__ void store_u64_kernel(const unsigned long long* __restrict__ src, volatile unsigned long long* dst) { *dst = *src; }

int r3dg_store_u64_to_host(void* stream_, const void* d_src, void* h_pinned_dst)
{
    if (d_src == nullptr || h_pinned_dst == nullptr) return invalid("store_u64_to_host: null pointer");
    return guarded([&]() -> int {
        void* mapped = nullptr;
        R3DG_HIP(hipHostGetDevicePointer(&mapped, h_pinned_dst, 0));
        store_u64_kernel<<<1, 1, 0, (hipStream_t)stream_>>>((const unsigned long long*)d_src, (volatile unsigned long long*)mapped);
        check_launch((hipStream_t)stream_, false, "store_u64_kernel");
        return R3DG_OK;
    });
}

int r3dg_spin(void* stream_, float microseconds)
{
    if (!(microseconds >= 0.f) || microseconds > 1e6f) return invalid("spin: 0 .. 1e6 microseconds");
    return guarded([&]() -> int {
        int dev = 0, khz = 100000;
        R3DG_HIP(hipGetDevice(&dev));
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0) khz = 100000;
        const unsigned long long ticks = (unsigned long long)((double)microseconds * 1e-3 * (double)khz);
        spin_kernel<<<1, 64, 0, (hipStream_t)stream_>>>(ticks);
        check_launch((hipStream_t)stream_, false, "spin_kernel");
        return R3DG_OK;
    });
}

// every wave of a device-filling grid: `iters` x 16 independent fp32 FMAs per lane (VALU issue is the only thing it does), the
// shader-clock counter (s_memtime) and the constant-rate wall clock (s_memrealtime) read on both sides.  out[0] += shader cycles,
// out[1] += wall ticks, out[2] += 1 per wave: sum(cycles) / sum(ticks) x wall-clock rate = the shader clock UNDER VALU LOAD.
__global__ void __launch_bounds__(256) clock_probe_kernel(int iters, unsigned long long* __restrict__ out, float* __restrict__ sink)
{
    float a[16];
#pragma unroll
    for (int i = 0; i < 16; i++) a[i] = (float)(threadIdx.x + i) * 1e-3f;
    const float m = 0.999f, c = 1e-4f;
    const unsigned long long w0 = wall_clock64();
    const long long t0 = clock64();
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int i = 0; i < 16; i++) a[i] = __builtin_fmaf(a[i], m, c);
    }
    const long long t1 = clock64();
    const unsigned long long w1 = wall_clock64();
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 16; i++) s += a[i];
    if (s == 123456.789f) sink[0] = s;                       // (keeps the loop)
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&out[0], (unsigned long long)(t1 - t0));
        atomicAdd(&out[1], w1 - w0);
        atomicAdd(&out[2], 1ull);
    }
}

int r3dg_clock_probe(void* stream_, int iters, unsigned long long* d_out3, float* d_sink, int* wall_clock_khz)
{
    if (iters <= 0 || !d_out3 || !d_sink) return invalid("clock_probe: bad arguments");
    return guarded([&]() -> int {
        int dev = 0, khz = 100000, cus = 256;
        R3DG_HIP(hipGetDevice(&dev));
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0) khz = 100000;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
        if (wall_clock_khz) *wall_clock_khz = khz;
        R3DG_HIP(hipMemsetAsync(d_out3, 0, 3 * sizeof(unsigned long long), (hipStream_t)stream_));
        clock_probe_kernel<<<cus * 8, 256, 0, (hipStream_t)stream_>>>(iters, d_out3, d_sink);      // 8 waves per SIMD
        check_launch((hipStream_t)stream_, false, "clock_probe_kernel");
        return R3DG_OK;
    });
}

}  // extern "C"
