// Launchers of the transport-cache builders that regenerate the ray set -- from traced [P,K] visibility or from the baked
// visibility SH -- and of the expansion of that SH into [P,K] (shading_transport_rayset.hpp).  A unit of its own, beside
// shading_relight.hip, for its floating-point regime.  The lat-long lookup is singular at its poles: what a direction is off by
// reaches the lookup multiplied by 1 / sin(polar angle), and among a few hundred thousand samples some sit within a tenth of
// a degree of a pole (a factor of 760 at 0.075 degrees).  So the cache agrees with the two-kernel path on the directions the
// trace generated (r3dg_shade_build_taps + r3dg_shade_build_transport) only as far as the direction AND its rotation into the
// light's frame do, to the bit:
//   * ray_set.hpp is included first, without contraction, and the unit is compiled without -ffast-math (build.py): the regime
//     of the visibility trace, so this kernel regenerates the directions r3dg_bvh_trace_bundles traced bit for bit.  Under the
//     shading units' -ffast-math (approximate division and square root in the normalisation) the records were 2.3e-5 of the
//     largest one off the two-kernel path at 3000 x 16, five times what the two exact direction sets cost each other.
//   * the kernel spells the rotation out with explicit fused multiply-adds.  Left to contraction (which of the three products
//     is rounded on its own is the compiler's choice, and it chose differently here than in shade_build_taps_kernel) one
//     record of 300 000 was 1.4e-4 of the largest one off at 3000 x 100 under a rotated light.
#include <hip/hip_runtime.h>
#pragma clang fp contract(off)
#include "ray_set.hpp"
#pragma clang fp contract(fast)
#include "shading_host.hpp"
#include "shading_transport_rayset.hpp"

namespace r3dg {

void launch_shade_build_transport_rayset(hipStream_t s, int P, int K, int M, const float* normals, const float* incidents,
                                         const float* visibility, const float* zsamples, float uniform_area, const float* env,
                                         int He, int We, const float* tr, float* transport, float* consts)
{
    if (P == 0) return;
    shade_build_transport_rayset_kernel<false><<<(P + TR_WAVES - 1) / TR_WAVES, 64 * TR_WAVES, 0, s>>>(
        P, K, M, normals, incidents, visibility, zsamples, uniform_area, env, He, We, tr, transport, consts);
    check_launch(s, false, "shade_build_transport_rayset_kernel");
}

void launch_shade_build_transport_baked(hipStream_t s, int P, int K, int M, const float* normals, const float* incidents,
                                        const float* visibility_sh, const float* zsamples, float uniform_area, const float* env,
                                        int He, int We, const float* tr, float* transport, float* consts)
{
    if (P == 0) return;
    shade_build_transport_rayset_kernel<true><<<(P + TR_WAVES - 1) / TR_WAVES, 64 * TR_WAVES, 0, s>>>(
        P, K, M, normals, incidents, visibility_sh, zsamples, uniform_area, env, He, We, tr, transport, consts);
    check_launch(s, false, "shade_build_transport_rayset_kernel<baked>");
}

void launch_visibility_sh_expand(hipStream_t s, int P, int K, const float* normals, const float* zsamples,
                                 const float* visibility_sh, float* out)
{
    if (P == 0) return;
    visibility_sh_expand_kernel<<<(P + TR_WAVES - 1) / TR_WAVES, 64 * TR_WAVES, 0, s>>>(P, K, normals, zsamples, visibility_sh, out);
    check_launch(s, false, "visibility_sh_expand_kernel");
}

}  // namespace r3dg
