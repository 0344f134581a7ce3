// Per-pixel expressions of an eval frame's capture maps (gaussian_renderer/neilf.py:146-182, render.py:107-113), shared by the
// kernels that evaluate them: eval_capture.hip (the maps as float images) and training_sheet.hip (the same maps as panels of the
// training contact sheet).  One definition, so that the two cannot drift apart by a rounding.
#pragma once
#include "glue_math.hpp"

namespace r3dg {

// depth2 - depth^2: a difference of two nearly equal terms, where a fused multiply-add is a visibly different value
__device__ __forceinline__ float variance_of(float d, float d2)
{
#pragma clang fp contract(off)
    const float sq = d * d;
    return d2 - sq;
}

// the divisor of a pixel: rendered_feature / opacity.clamp_min(1e-5) * (num_contrib > 0) (neilf.py:146-147); 0 stands for
// num_contrib == 0
__device__ __forceinline__ float capture_divisor(float opacity, int n_contrib) { return n_contrib > 0 ? fmaxf(opacity, 1e-5f) : 0.f; }

// feature / max(opacity, 1e-5) * (num_contrib > 0) with the reference's own rounding (a true division: depth_var is a
// difference of two nearly equal terms, a reciprocal's extra half ulp would show there); den == 0 stands for num_contrib == 0
__device__ __forceinline__ float normalised(float f, float den) { return den > 0.f ? __fdiv_rn(f, den) : 0.f; }

// results["pbr"] = rgb_to_srgb(pbr * opacity + (1 - opacity) * background) (neilf.py:174-182)
__device__ __forceinline__ float pbr_over_background(float pbr, float op, float bg) { return srgb_of(pbr * op + (1.f - op) * bg); }

}  // namespace r3dg
