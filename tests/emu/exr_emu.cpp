// TEST INFRASTRUCTURE ONLY: the OpenEXR chunk-decode kernels (csrc/exr_decode.hpp -- the very file exr_unpack.hip compiles for
// gfx950) run through a lock-step CPU emulation: every lane of a workgroup is a std::thread, `__shared__` variables are function
// statics (workgroups run one after the other), __syncthreads is a barrier over the workgroup, __shfl_xor / __shfl_up are
// barrier-fenced exchanges inside the 64-lane wave.  hip_emu.hpp's model, with the integer shuffles and the 2-D grid these
// kernels use.
//   g++ -std=c++20 -O1 -pthread -shared -fPIC -I relightable3dgaussian_amd/csrc tests/emu/exr_emu.cpp -o libexr_emu.so
#include <barrier>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <thread>
#include <vector>

struct emu_uint3 { unsigned x, y, z; };
struct alignas(16) uint4 { uint32_t x, y, z, w; };
inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
inline thread_local emu_uint3 threadIdx, blockIdx, blockDim, gridDim;

struct EmuBlock {
    std::unique_ptr<std::barrier<>> block_barrier;
    std::vector<std::unique_ptr<std::barrier<>>> wave_barrier;
    std::vector<uint32_t> exchange;          // one slot per lane
};
inline EmuBlock* g_emu_block = nullptr;

inline void __syncthreads() { g_emu_block->block_barrier->arrive_and_wait(); }

inline uint32_t emu_exchange(uint32_t v, unsigned from_lane)
{
    const unsigned t = threadIdx.x, wave = t >> 6;
    g_emu_block->exchange[t] = v;
    g_emu_block->wave_barrier[wave]->arrive_and_wait();
    const uint32_t r = g_emu_block->exchange[(t & ~63u) | (from_lane & 63u)];
    g_emu_block->wave_barrier[wave]->arrive_and_wait();
    return r;
}
inline uint32_t __shfl_xor(uint32_t v, int mask) { return emu_exchange(v, (threadIdx.x ^ (unsigned)mask) & 63u); }
inline uint32_t __shfl_up(uint32_t v, int delta)          // lanes below `delta` keep their own value, as on the device
{
    const unsigned lane = threadIdx.x & 63u;
    return emu_exchange(v, lane >= (unsigned)delta ? lane - (unsigned)delta : lane);
}

#define __global__
#define __device__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(...)
#define __shared__ static
#define R3DG_EXR_TILE 4096
#define R3DG_EXR_MAX_KEPT 8

// A thread that returns early must do so together with its whole workgroup before any barrier -- the kernels' early returns are
// uniform over the workgroup.
template <typename K, typename... A>
void emu_launch(K kernel, unsigned grid_x, unsigned grid_y, unsigned block, A... args)
{
    for (unsigned by = 0; by < grid_y; by++)
        for (unsigned bx = 0; bx < grid_x; bx++) {
            EmuBlock blk;
            blk.block_barrier = std::make_unique<std::barrier<>>(block);
            for (unsigned w = 0; w < block / 64; w++) blk.wave_barrier.push_back(std::make_unique<std::barrier<>>(64));
            blk.exchange.assign(block, 0u);
            g_emu_block = &blk;
            std::vector<std::thread> lanes;
            lanes.reserve(block);
            for (unsigned t = 0; t < block; t++)
                lanes.emplace_back([=]() {
                    threadIdx = {t, 0, 0};
                    blockIdx = {bx, by, 0};
                    blockDim = {block, 1, 1};
                    gridDim = {grid_x, grid_y, 1};
                    kernel(args...);
                });
            for (auto& th : lanes) th.join();
            g_emu_block = nullptr;
        }
}

#include "exr_decode.hpp"

extern "C" {

// r3dg_exr_unpack_chunks with host pointers; tile_sums: chunks * 2 * tiles uint32, tiles as the launcher computes them
void emu_exr_unpack_chunks(int W, int H, int C, int B, int chunks, int max_rows, const uint8_t* inflated, long long inflated_bytes,
                           const int32_t* table, int kept, const int32_t* kept_channels, uint32_t* tile_sums, void* planes)
{
    const size_t half = (size_t)max_rows * W * C * B / 2;
    const unsigned tiles = (unsigned)((half + r3dg::TILE - 1) / r3dg::TILE);
    emu_launch(r3dg::exr_tile_sums_kernel, tiles, (unsigned)chunks, (unsigned)r3dg::THREADS, W, H, C, B, max_rows, inflated,
               inflated_bytes, table, tile_sums);
    if (B == 2)
        emu_launch(r3dg::exr_unpack_kernel<2>, tiles, (unsigned)chunks, (unsigned)r3dg::THREADS, W, H, C, max_rows, inflated,
                   inflated_bytes, table, kept, kept_channels, (const uint32_t*)tile_sums, planes);
    else
        emu_launch(r3dg::exr_unpack_kernel<4>, tiles, (unsigned)chunks, (unsigned)r3dg::THREADS, W, H, C, max_rows, inflated,
                   inflated_bytes, table, kept, kept_channels, (const uint32_t*)tile_sums, planes);
}

}
