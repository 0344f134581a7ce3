// The fixed ray set of a visibility update: sample k of the Gaussian with normal n is d_k = normalize(R(n) z_k), z_k the
// K-entry Fibonacci table around +z (sampling.fibonacci_z_samples) and R = rotation_between_z (utils/sh_utils.py:36-68).
// ONE definition for everybody who regenerates the directions instead of reading a [P,K,3] tensor: the fixed-ray-set shading
// kernels (shading_frs.hip, shading_split.hpp, shading_transport.hpp, shading_transport_rayset.hpp) and the bundle source of the
// visibility trace (bvh_trace.hip), so that trace and shading see one ray set.  The units are compiled with different
// floating-point flags (-ffast-math for the shading units, -ffp-contract=off for the trace): the operations are the same, their
// last bits are not -- except in shading_relight_rayset.hip, which includes this header under the trace's regime.
#pragma once

namespace r3dg {

// rotation_between_z(n) (utils/sh_utils.py:36-68), fp32 operation for operation as sampling.rotation_between_z: the rotation
// that takes +z to n (the identity's negative when n_z + 1 <= 0)
__device__ __forceinline__ void rotation_between_z(const float n0, const float n1, const float n2, float (&R)[9])
{
    const float v1 = -n1, v2 = n0, cp = fmaxf(n2 + 1.f, 1e-7f);
    const bool regular = n2 + 1.f > 0.f;
    R[0] = regular ? 1.f + (-v2 * v2) / cp : -1.f;
    R[1] = regular ? v1 * v2 / cp : 0.f;
    R[2] = regular ? v2 : 0.f;
    R[3] = R[1];
    R[4] = regular ? 1.f + (-v1 * v1) / cp : -1.f;
    R[5] = regular ? -v1 : 0.f;
    R[6] = regular ? -v2 : 0.f;
    R[7] = regular ? v1 : 0.f;
    R[8] = regular ? 1.f + (-v2 * v2 - v1 * v1) / cp : -1.f;
}

// normalize(R z) as sampling.py / graphics_utils.py:9-37 evaluate it: matrix product, then x / max(|x|, 1e-12)
__device__ __forceinline__ void ray_set_direction(const float (&R)[9], const float zx, const float zy, const float zz, float& dx,
                                                  float& dy, float& dz)
{
    dx = R[0] * zx + R[1] * zy + R[2] * zz; dy = R[3] * zx + R[4] * zy + R[5] * zz; dz = R[6] * zx + R[7] * zy + R[8] * zz;
    const float len = fmaxf(sqrtf(dx * dx + dy * dy + dz * dz), 1e-12f);
    dx /= len; dy /= len; dz /= len;
}

}  // namespace r3dg
