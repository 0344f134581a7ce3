// What the C-ABI translation units (capi_*.hip) share: the mapping of exceptions to return codes, the per-stage timer and
// the event-ring stream join.  The state behind them lives in capi_core.hip.
#pragma once
#include "launchers.hpp"

#include <exception>

namespace r3dg {

template <typename F>
static int guarded(F&& f)
{
    try {
        return f();
    } catch (const HipError& e) {
        (void)hipGetLastError();
        return e.code == -1 ? R3DG_EINVAL : R3DG_EHIP;
    } catch (const std::exception& e) {
        set_error(e.what());
        return R3DG_EHIP;
    }
}

inline int invalid(const std::string& msg)
{
    set_error(msg);
    return R3DG_EINVAL;
}

// ---- optional per-stage timing with HIP events on the launch stream (bench.py's roofline numbers) ----
// r3dg_profile_stage_name(i) is kStageNames[i]: the enum and the names are one list in two notations.
enum Stage { ST_PREPROCESS = 0, ST_DUPKEYS, ST_SORT, ST_RANGES, ST_RENDER_FWD, ST_NORMAL, ST_RENDER_BWD, ST_PREPROCESS_BWD,
             ST_SHADE_FWD, ST_SHADE_BWD, ST_SHADE_AUX, ST_SHADE_LISTED, ST_BVH_BUILD, ST_BVH_TRACE, ST_S2_ACTIVATE, ST_S2_PACK, ST_S2_LOSS,
             ST_S2_UNPACK, ST_S2_ACTIVATE_BWD, ST_ADAM, ST_KNN, ST_SSIM, ST_DENSIFY, ST_RELIGHT_PACK, ST_RELIGHT_COMPOSE,
             ST_COUNT };
inline constexpr const char* kStageNames[] = {"preprocess", "duplicate_with_keys", "sort_pairs", "identify_tile_ranges",
                                              "render_forward", "pseudo_normal", "render_backward", "preprocess_backward",
                                              "shade_forward", "shade_backward", "shade_frs_aux", "shade_frs_listed", "bvh_build", "bvh_trace",
                                              "stage2_activate", "stage2_pack_features", "stage2_loss",
                                              "stage2_unpack_gradients", "stage2_activate_backward", "adam_step",
                                              "knn_dist2", "ssim", "densify", "relight_pack_features", "relight_compose"};
static_assert(sizeof(kStageNames) / sizeof(kStageNames[0]) == ST_COUNT, "one name per Stage");

// Times what `s` runs between construction and stop() (or destruction) while r3dg_profile_enable is on; nothing otherwise.
struct StageTimer {
    hipStream_t s;
    int stage;
    hipEvent_t a, b;
    bool on;
    StageTimer(hipStream_t s_, int stage_);
    ~StageTimer() { try { stop(); } catch (...) {} }
    void stop();
};

// `waiter` waits for everything queued on `signaller` so far (nothing to do when they are the same stream).
void stream_wait_stream(hipStream_t waiter, hipStream_t signaller);

}  // namespace r3dg
