// What the launchers of the three shading units (shading.hip, shading_frs.hip, shading_relight.hip) share on the host.  The
// persistent-grid CU count they size their grids by is persistent_cus() (launchers.hpp).
#pragma once
#include "launchers.hpp"

namespace r3dg {

constexpr int ENV_LDS_MAX = 12288;           // floats (48 KB) -- larger maps are sampled from global/L2

// The words a backward kernel scales its fixed-point texture accumulation by: max |upstream gradient|, either handed over as
// block maxima by the producer of g_pbr / g_diff (r3dg_stage2_unpack_gradients) or reduced here into the per-device scratch
// word.  *gmax_n = number of words.  (shading.hip; library-internal, not part of the exported surface)
__attribute__((visibility("hidden"))) const unsigned int* shade_upstream_absmax(hipStream_t s, int P, const float* g_pbr,
                                                                              const float* g_diff, const float* block_absmax,
                                                                              int n_block_absmax, int* gmax_n);

// every sample of the Fibonacci set carries the same area, 2 pi (fibonacci_sphere_sampling, utils/graphics_utils.py:26-37);
// uniform_area == 0 means that value
static inline float frs_area(float uniform_area) { return uniform_area > 0.f ? uniform_area : 6.283185307179586f; }

}  // namespace r3dg
