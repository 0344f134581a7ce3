// What every kernel that writes or reads the relight frame's transport cache agrees on (shading_transport.hpp, and the builder
// from the ray set in shading_transport_rayset.hpp, which lives in another unit and so cannot include a header that defines
// kernels): the launch shape, the per-Gaussian constants and the wave reduction.  Compiled by the CPU emulation in tests/emu too.
#pragma once

namespace r3dg {

constexpr int TR_WAVES = 4;
constexpr int TR_CONSTS = 16;     // floats per Gaussian: diffuse_light 3 | incident light 3 | local 3 | global 3 | visibility 1 | pad

// (common.hpp's wave_sum, restated: the CPU emulation compiles this header and cannot include the HIP-only common.hpp)
__device__ __forceinline__ float wave_sum64(float x)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

}  // namespace r3dg
