// The image-space tail of a stage-2 iteration as ONE launch for gfx950: what s2_normals_srgb_kernel, ssim_forward_kernel,
// ssim_backward_kernel and s2_loss_kernel<true> (stage2_glue.hip, ssim.hip) do as four dependent launches between the tile
// forward and the tile backward -- each bound by latency, nothing beside them on the device -- with everything only the next
// launch would read kept on chip: the sRGB PBR image, the 2 x 9 SSIM partial-derivative planes, the 2 x 3 SSIM gradient planes.
//
// One 32x32 tile of one image per 256-thread workgroup.  The SSIM gradient at a pixel needs the partial derivatives of the
// eleven-tap window around it, and each of those the image values of the window around IT, so a workgroup stages tile + 10
// pixels, forms the SSIM map and its partials over tile + 5 (recomputing what the neighbouring tiles' workgroups also form:
// (42/32)^2 = 1.72x the forward's arithmetic instead of 27 planes through HBM and two launch boundaries), and filters those
// over the tile.  Per channel, all in LDS (44.7 KB: every stage takes the place of the one before it, results wait in
// registers across a barrier where the two overlap):
//   load   52x52 of x, y (zero outside the image; the PBR image's x is the sRGB value, computed here, never stored)
//   rows   52 rows x 42 columns of the five window averages' row sums          (items of 3 columns: 728 on 256 threads)
//   cols   42x42 window averages -> SSIM value + three partials per pixel     (items of 7 rows: 252 of them)
//          partials at pixels outside the image are 0 -- windows centred there do not exist; the SSIM SUM takes the tile's
//          own pixels only
//   rows   42 rows x 32 columns of the three partial maps' row sums            (items of 4 columns: 336)
//   cols   32x32: the thread's own 4 pixels, as in ssim_backward_kernel
// Jobs: the PBR image's three channels meet in ONE workgroup (dL_dopacity sums over them: one deterministic sum per pixel, in
// s2_loss_kernel's order, no atomics), which also writes the pseudo normals / surface points and the normal term; the SH image
// runs one channel per workgroup.  The three-channel jobs are the longer ones and come first in the grid.
// Arithmetic: ssim_window.hpp, stage2_loss_math.hpp, pseudo_normal.hpp -- the functions the four kernels compile.
#include "launchers.hpp"
#include "ssim_window.hpp"
#include "stage2_loss_math.hpp"
#include "pseudo_normal.hpp"
#include "r3dg_hip.h"

namespace r3dg {

constexpr int TAIL_T = 32;                        // tile edge (outputs)
constexpr int TAIL_P = TAIL_T + 2 * SSIM_R;       // 42: the region whose partials the tile's gradient reads
constexpr int TAIL_E = TAIL_T + 4 * SSIM_R;       // 52: the region whose pixels those partials read
constexpr int TAIL_NLOAD = (TAIL_E * TAIL_E + 255) / 256;                 // staged elements per thread (11)
constexpr int TAIL_FB = 3;                        // forward row pass: adjacent columns per item (42 = 14 x 3)
constexpr int TAIL_FV = 7;                        // forward column pass: adjacent rows per item (42 = 6 x 7)
constexpr int TAIL_BB = 4;                        // backward passes: outputs per item, as ssim_backward_kernel
constexpr int TAIL_IN_FLOATS = 2 * TAIL_E * (TAIL_E + 1);                 // x, y staged: 5512
constexpr int TAIL_H_FLOATS = 5 * TAIL_E * (TAIL_P + 1);                  // forward row sums: 11180
constexpr int TAIL_PART_FLOATS = 3 * TAIL_P * (TAIL_P + 1);               // partials: 5418
constexpr int TAIL_G_FLOATS = 3 * TAIL_P * (TAIL_T + 1);                  // backward row sums: 4158
// the backward row sums lie behind the staged inputs: the next channel's load stage may start while a wave still reads them
constexpr int TAIL_G_AT = TAIL_IN_FLOATS;
static_assert(TAIL_G_AT % 2 == 0 && TAIL_PART_FLOATS <= TAIL_G_AT && TAIL_G_AT + TAIL_G_FLOATS <= TAIL_H_FLOATS, "LDS regions of the tail overlap");
static_assert(TAIL_P % TAIL_FB == 0 && TAIL_P % TAIL_FV == 0 && TAIL_P * (TAIL_P / TAIL_FV) <= 256, "forward items");
static_assert(TAIL_T % TAIL_BB == 0 && TAIL_T * (TAIL_T / TAIL_BB) == 256, "backward items");

// what a pixel of the sRGB PBR image is made of
struct TailPbrRaw {
    float op;
    int nc;
    float F, y;
};

struct ImageTail {
    int W, H, tiles_x, n_tiles;
    float focal_x, focal_y, cx, cy;
    const float* vm;
    const float* image;
    const float* opacity;
    const float* depths;
    const float* feature;
    const int* n_contrib;
    const float* gt;
    const float* bg;
    const float* image_mask;
    float w_l1, w_pbr, w_normal, scale_image, scale_pbr;
    float* pseudo_normal;
    float* surface_xyz;
    float* dL_dimage;
    float* dL_dopacity;
    float* dL_dfeature;
    float* sums;
    float* ssim_sum_image;
    float* ssim_sum_pbr;
};

// pseudo_normal_pixel as a function of its own.  Inlined into the tail kernel's loop it is vectorised and contracted in another
// grouping than in s2_normals_srgb_kernel and pseudo_normal_kernel, whose one-pixel threads it is the whole body of, and the normals
// come out an ulp apart; compiled on its own it has the arithmetic it has there (tests/test_image_tail_gpu.py holds the two equal).
__device__ __noinline__ void tail_pseudo_normal(int x, int y, int W, int H, float focal_x, float focal_y, float cx, float cy,
                                                const float* __restrict__ vm, const float* __restrict__ opacities,
                                                const float* __restrict__ depths, float* __restrict__ normals,
                                                float* __restrict__ surface_xyz)
{
    pseudo_normal_pixel(x, y, W, H, focal_x, focal_y, cx, cy, vm, opacities, depths, normals, surface_xyz);
}

// One channel of one image over the tile at (bx, by): fetch(o) reads what the pair at pixel offset o (always inside the image) is
// made of, make(raw, x, y) forms the pair from it -- two steps, so that every load of the region is in flight before any
// arithmetic (the sRGB curve has a branch: as one step the compiler waited for memory once per element, eleven times per channel).  -> acc[m][o]: the window average of partial map m at the thread's own pixel (tx, ty0 + o); ssim_sum += the SSIM
// values this thread formed for pixels of the tile itself.
template <class Raw, class Fetch, class Make>
__device__ __forceinline__ void tail_ssim_channel(float* s_raw, int W, int H, int bx, int by, Fetch fetch, Make make, float (&acc)[3][TAIL_BB],
                                                  float& ssim_sum)
{
    // maps that are filtered alike lie side by side as pairs -- (x, y); (mu1, mu2), (E[x^2], E[y^2]); (dS/dmu1, dS/dE[x^2]) -- so that
    // one 8-byte LDS access and one packed instruction serve both
    float2v (*s_xy)[TAIL_E + 1] = reinterpret_cast<float2v (*)[TAIL_E + 1]>(s_raw);
    float2v (*s_h01)[TAIL_P + 1] = reinterpret_cast<float2v (*)[TAIL_P + 1]>(s_raw);
    float2v (*s_h23)[TAIL_P + 1] = reinterpret_cast<float2v (*)[TAIL_P + 1]>(s_raw + 2 * TAIL_E * (TAIL_P + 1));
    float (*s_h4)[TAIL_P + 1] = reinterpret_cast<float (*)[TAIL_P + 1]>(s_raw + 4 * TAIL_E * (TAIL_P + 1));
    float2v (*s_p01)[TAIL_P + 1] = reinterpret_cast<float2v (*)[TAIL_P + 1]>(s_raw);
    float (*s_p2)[TAIL_P + 1] = reinterpret_cast<float (*)[TAIL_P + 1]>(s_raw + 2 * TAIL_P * (TAIL_P + 1));
    float2v (*s_g01)[TAIL_T + 1] = reinterpret_cast<float2v (*)[TAIL_T + 1]>(s_raw + TAIL_G_AT);
    float (*s_g2)[TAIL_T + 1] = reinterpret_cast<float (*)[TAIL_T + 1]>(s_raw + TAIL_G_AT + 2 * TAIL_P * (TAIL_T + 1));
    // (an opaque copy of the thread index per call: inside the three-channel loop the compiler otherwise hoists every index, mask
    // and LDS address of every stage in front of the loop and keeps them alive through it -- 350 registers and 800 bytes of
    // scratch per lane instead of 150 and none)
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    {
        // (every load of the region is issued before the first one is used, see ssim_forward_tile)
        float2v xy[TAIL_NLOAD];
        Raw raw[TAIL_NLOAD];
        bool in[TAIL_NLOAD];
#pragma unroll
        for (int j = 0; j < TAIL_NLOAD; j++) {
            const int i = tid + j * 256;
            const int r = i / TAIL_E, q = i % TAIL_E;
            const int gy = by + r - 2 * SSIM_R, gx = bx + q - 2 * SSIM_R;
            in[j] = i < TAIL_E * TAIL_E && gx >= 0 && gx < W && gy >= 0 && gy < H;             // zero padding
            raw[j] = fetch((size_t)(in[j] ? gy : 0) * W + (in[j] ? gx : 0));
        }
#pragma unroll
        for (int j = 0; j < TAIL_NLOAD; j++) {
            float vx, vy;
            make(raw[j], vx, vy);
            xy[j].x = in[j] ? vx : 0.f;
            xy[j].y = in[j] ? vy : 0.f;
        }
#pragma unroll
        for (int j = 0; j < TAIL_NLOAD; j++) {
            const int i = tid + j * 256;
            if (i < TAIL_E * TAIL_E) s_xy[i / TAIL_E][i % TAIL_E] = xy[j];
        }
    }
    __syncthreads();
    float w[11];
    ssim_load_window(w);
    {
        constexpr int GROUPS = TAIL_P / TAIL_FB, ITEMS = TAIL_E * GROUPS, ROUNDS = (ITEMS + 255) / 256;
        float2v h01[ROUNDS][TAIL_FB], h23[ROUNDS][TAIL_FB];
        float h4[ROUNDS][TAIL_FB];
#pragma unroll
        for (int rd = 0; rd < ROUNDS; rd++) {
            const int i = tid + rd * 256;
            if (i < ITEMS) {
                const int r = i / GROUPS, q0 = (i % GROUPS) * TAIL_FB;
                float2v xy[TAIL_FB + 10];
#pragma unroll
                for (int k = 0; k < TAIL_FB + 10; k++) xy[k] = s_xy[r][q0 + k];
#pragma unroll
                for (int o = 0; o < TAIL_FB; o++) ssim_taps_pair_packed(w, xy + o, h01[rd][o], h23[rd][o], h4[rd][o]);
            }
        }
        __syncthreads();                               // every read of the staged inputs is done: reuse their storage
#pragma unroll
        for (int rd = 0; rd < ROUNDS; rd++) {
            const int i = tid + rd * 256;
            if (i < ITEMS) {
                const int r = i / GROUPS, q0 = (i % GROUPS) * TAIL_FB;
#pragma unroll
                for (int o = 0; o < TAIL_FB; o++) {
                    s_h01[r][q0 + o] = h01[rd][o];
                    s_h23[r][q0 + o] = h23[rd][o];
                    s_h4[r][q0 + o] = h4[rd][o];
                }
            }
        }
    }
    __syncthreads();
    {
        constexpr int ITEMS = TAIL_P * (TAIL_P / TAIL_FV);
        const int qx = tid % TAIL_P, r0 = (tid / TAIL_P) * TAIL_FV;
        float2v p01[TAIL_FV];
        float p2[TAIL_FV];
        if (tid < ITEMS) {
            float2v mu[TAIL_FV], ee[TAIL_FV];
            float e12[TAIL_FV];
            {
                float2v col[TAIL_FV + 10];
#pragma unroll
                for (int k = 0; k < TAIL_FV + 10; k++) col[k] = s_h01[r0 + k][qx];
#pragma unroll
                for (int o = 0; o < TAIL_FV; o++) mu[o] = ssim_taps(w, col + o);
#pragma unroll
                for (int k = 0; k < TAIL_FV + 10; k++) col[k] = s_h23[r0 + k][qx];
#pragma unroll
                for (int o = 0; o < TAIL_FV; o++) ee[o] = ssim_taps(w, col + o);
            }
            {
                float col[TAIL_FV + 10];
#pragma unroll
                for (int k = 0; k < TAIL_FV + 10; k++) col[k] = s_h4[r0 + k][qx];
#pragma unroll
                for (int o = 0; o < TAIL_FV; o++) e12[o] = ssim_taps(w, col + o);
            }
            const int gx = bx + qx - SSIM_R;
#pragma unroll
            for (int o = 0; o < TAIL_FV; o++) {
                const int gy = by + r0 + o - SSIM_R;
                float q0, q1, q2;
                const float ssim = ssim_pixel<true>(mu[o].x, mu[o].y, ee[o].x, ee[o].y, e12[o], q0, q1, q2);
                // windows centred outside the image do not exist (on zero padding the formulas give -1/C2 and 2/C2, not 0)
                const bool in = gx >= 0 && gx < W && gy >= 0 && gy < H;
                p01[o].x = in ? q0 : 0.f;
                p01[o].y = in ? q1 : 0.f;
                p2[o] = in ? q2 : 0.f;
                const bool own = in && gx >= bx && gx < bx + TAIL_T && gy >= by && gy < by + TAIL_T;
                ssim_sum += own ? ssim : 0.f;
            }
        }
        __syncthreads();                               // every read of the row sums is done: reuse their storage
        if (tid < ITEMS) {
#pragma unroll
            for (int o = 0; o < TAIL_FV; o++) {
                s_p01[r0 + o][qx] = p01[o];
                s_p2[r0 + o][qx] = p2[o];
            }
        }
    }
    __syncthreads();
    {
        constexpr int GROUPS = TAIL_T / TAIL_BB, ITEMS = TAIL_P * GROUPS, ROUNDS = (ITEMS + 255) / 256;
#pragma unroll
        for (int rd = 0; rd < ROUNDS; rd++) {
            const int i = tid + rd * 256;
            if (i < ITEMS) {
                const int r = i / GROUPS, q0 = (i % GROUPS) * TAIL_BB;
                float2v v01[TAIL_BB + 10];
                float v2[TAIL_BB + 10];
#pragma unroll
                for (int k = 0; k < TAIL_BB + 10; k++) { v01[k] = s_p01[r][q0 + k]; v2[k] = s_p2[r][q0 + k]; }
#pragma unroll
                for (int o = 0; o < TAIL_BB; o++) {                                       // (storage of their own)
                    s_g01[r][q0 + o] = ssim_taps(w, v01 + o);
                    s_g2[r][q0 + o] = ssim_taps(w, v2 + o);
                }
            }
        }
    }
    __syncthreads();
    const int tx = tid % TAIL_T, ty0 = (tid / TAIL_T) * TAIL_BB;
    {
        float2v c01[TAIL_BB + 10];
        float c2[TAIL_BB + 10];
#pragma unroll
        for (int k = 0; k < TAIL_BB + 10; k++) { c01[k] = s_g01[ty0 + k][tx]; c2[k] = s_g2[ty0 + k][tx]; }
#pragma unroll
        for (int o = 0; o < TAIL_BB; o++) {
            const float2v a01 = ssim_taps(w, c01 + o);
            acc[0][o] = a01.x;
            acc[1][o] = a01.y;
            acc[2][o] = ssim_taps(w, c2 + o);
        }
    }
}

// (three workgroups per CU, what the LDS allows: 168 registers per lane; the kernel takes 136)
__global__ void __launch_bounds__(256, 3)
s2_image_tail_kernel(const ImageTail a)
{
    __shared__ __attribute__((aligned(16))) float s_raw[TAIL_H_FLOATS];
    __shared__ float s_part[4];
    const int W = a.W, H = a.H;
    const size_t HW = (size_t)H * W;
    const bool pbr_job = (int)blockIdx.x < a.n_tiles;
    const int job = pbr_job ? (int)blockIdx.x : (int)blockIdx.x - a.n_tiles;
    const int tile = job % a.n_tiles;
    const int bx = (tile % a.tiles_x) * TAIL_T, by = (tile / a.tiles_x) * TAIL_T;
    const int tx = threadIdx.x % TAIL_T, ty0 = (threadIdx.x / TAIL_T) * TAIL_BB;
    const int px = bx + tx;
    float acc[3][TAIL_BB];
    float ssim_sum = 0.f;

    if (!pbr_job) {
        // ---- the SH image, channel c: L1 + SSIM -> dL_dimage[c] -------------------------------------------------------------
        const int c = job / a.n_tiles;
        const float* __restrict__ xc = a.image + c * HW;
        const float* __restrict__ yc = a.gt + c * HW;
        tail_ssim_channel<float2v>(s_raw, W, H, bx, by, [&](size_t o) { float2v r; r.x = xc[o]; r.y = yc[o]; return r; },
                                   [](const float2v r, float& vx, float& vy) { vx = r.x; vy = r.y; }, acc, ssim_sum);
        float s_l1 = 0.f;
        float im[TAIL_BB], g[TAIL_BB];
        size_t off[TAIL_BB];
#pragma unroll
        for (int o = 0; o < TAIL_BB; o++) {               // (every load first)
            const int py = by + ty0 + o;
            off[o] = px < W && py < H ? (size_t)py * W + px : 0;
            im[o] = xc[off[o]];
            g[o] = yc[off[o]];
        }
#pragma unroll
        for (int o = 0; o < TAIL_BB; o++) {
            if (px < W && by + ty0 + o < H) {
                const float extra = ssim_grad_pixel(a.scale_image, acc[0][o], acc[1][o], acc[2][o], im[o], g[o]);
                a.dL_dimage[c * HW + off[o]] = s2_loss_image(im[o], g[o], a.w_l1, extra, s_l1);
            }
        }
        const float t0 = block_sum_256(s_l1, s_part);
        __syncthreads();
        const float t1 = block_sum_256(ssim_sum, s_part);
        if (threadIdx.x == 0) {
            atomicAdd(sum_slot(a.sums + 0 * R3DG_SUM_SLOTS), t0);
            atomicAdd(sum_slot(a.ssim_sum_image), t1);
        }
        return;
    }

    // ---- the sRGB PBR image, all three channels: L1 + SSIM + the normal term -> dL_dfeature, dL_dopacity; pseudo normals ---------
    const bool normal_on = a.w_normal != 0.f;
    float g_op[TAIL_BB] = {0.f, 0.f, 0.f, 0.f};
    // the rasterizer forward's deferred pseudo-normal pass for the thread's own pixels, first: its stores travel under the SSIM
    // stages, and the normal term below reads back what this thread stored (a loop, not unrolled: 18 loads per pixel)
#pragma unroll 1
    for (int o = 0; o < TAIL_BB; o++) {
        const int py = by + ty0 + o;
        if (px < W && py < H)
            tail_pseudo_normal(px, py, W, H, a.focal_x, a.focal_y, a.cx, a.cy, a.vm, a.opacity, a.depths, a.pseudo_normal,
                               a.surface_xyz);
    }
    float s_pbr = 0.f, s_n = 0.f;
#pragma unroll 1
    for (int c = 0; c < 3; c++) {
        const float* __restrict__ Fc = a.feature + (size_t)(2 + c) * HW;
        const float* __restrict__ yc = a.gt + c * HW;
        const float bgc = a.bg[c];
        // (opaque copies of everything the body derives its indices from, per channel: see tail_ssim_channel -- with the indices
        // hoisted in front of the loop the kernel took 237 registers, and two workgroups fit a CU instead of three)
        int txo = threadIdx.x % TAIL_T, tyo = (threadIdx.x / TAIL_T) * TAIL_BB, bxo = bx, byo = by, Wo = W, Ho = H;
        asm volatile("" : "+v"(txo), "+v"(tyo), "+s"(bxo), "+s"(byo), "+s"(Wo), "+s"(Ho));
        tail_ssim_channel<TailPbrRaw>(s_raw, Wo, Ho, bxo, byo,
                                      [&](size_t o) { return TailPbrRaw{a.opacity[o], a.n_contrib[o], Fc[o], yc[o]}; },
                                      [&](const TailPbrRaw r, float& vx, float& vy) {
                                          vx = s2_pbr_srgb_pixel(r.F, s2_divide_scale(r.op, r.nc), r.op, bgc);
                                          vy = r.y;
                                      },
                                      acc, ssim_sum);
        // the thread's own pixels: every load first, then the arithmetic (opacity, the division and the mask per channel again,
        // from cache, instead of sixteen registers held across the SSIM stages)
        const int px = bxo + txo;
        TailPbrRaw own[TAIL_BB];
        float mk[TAIL_BB], Fn[TAIL_BB], pn[TAIL_BB];
        size_t off[TAIL_BB];
#pragma unroll
        for (int o = 0; o < TAIL_BB; o++) {
            const int py = byo + tyo + o;
            off[o] = px < Wo && py < Ho ? (size_t)py * Wo + px : 0;
            own[o] = TailPbrRaw{a.opacity[off[o]], a.n_contrib[off[o]], Fc[off[o]], yc[off[o]]};
            mk[o] = 1.f; Fn[o] = 0.f; pn[o] = 0.f;
            if (normal_on) {
                if (a.image_mask != nullptr) mk[o] = a.image_mask[off[o]];
                Fn[o] = a.feature[(size_t)(5 + c) * HW + off[o]];
                pn[o] = a.pseudo_normal[c * HW + off[o]];
            }
        }
#pragma unroll
        for (int o = 0; o < TAIL_BB; o++) {
            const int py = byo + tyo + o;
            if (px < Wo && py < Ho) {
                const float F = own[o].F, g = own[o].y, op = own[o].op;
                const S2Divide dv = s2_divide(op, own[o].nc);
                const float srgb = s2_pbr_srgb_pixel(F, dv.scale, op, bgc);
                const float extra = ssim_grad_pixel(a.scale_pbr, acc[0][o], acc[1][o], acc[2][o], srgb, g);
                a.dL_dfeature[(size_t)(2 + c) * HW + off[o]] = s2_loss_pbr(F, g, op, bgc, dv, a.w_pbr, extra, s_pbr, g_op[o]);
                if (normal_on)
                    a.dL_dfeature[(size_t)(5 + c) * HW + off[o]] = s2_loss_normal(Fn[o], pn[o], mk[o], dv, a.w_normal, s_n, g_op[o]);
            }
        }
    }
#pragma unroll
    for (int o = 0; o < TAIL_BB; o++) {
        const int py = by + ty0 + o;
        if (px < W && py < H) a.dL_dopacity[(size_t)py * W + px] = g_op[o];
    }
    const float t1 = block_sum_256(s_pbr, s_part);
    __syncthreads();
    const float t2 = block_sum_256(s_n, s_part);
    __syncthreads();
    const float t3 = block_sum_256(ssim_sum, s_part);
    if (threadIdx.x == 0) {
        atomicAdd(sum_slot(a.sums + 1 * R3DG_SUM_SLOTS), t1);
        if (normal_on) atomicAdd(sum_slot(a.sums + 2 * R3DG_SUM_SLOTS), t2);
        atomicAdd(sum_slot(a.ssim_sum_pbr), t3);
    }
}

bool image_tail_applies(int W, int H)
{
    // (pixel coordinates and the linear grid are ints)
    return W > 0 && H > 0 && (long long)W * H <= 0x7fffffffLL;
}

void launch_s2_image_tail(hipStream_t s, int W, int H, const float* vm, float focal_x, float focal_y, float cx, float cy,
                          const float* image, const float* opacity, const float* depths, const float* feature, const int* n_contrib,
                          const float* gt, const float* bg, const float* image_mask, float w_l1, float w_pbr, float w_normal,
                          float scale_image, float scale_pbr, float* pseudo_normal, float* surface_xyz, float* dL_dimage,
                          float* dL_dopacity, float* dL_dfeature, float* sums, float* ssim_sum_image, float* ssim_sum_pbr)
{
    ImageTail a;
    a.W = W; a.H = H;
    a.tiles_x = (W + TAIL_T - 1) / TAIL_T;
    a.n_tiles = a.tiles_x * ((H + TAIL_T - 1) / TAIL_T);
    a.focal_x = focal_x; a.focal_y = focal_y; a.cx = cx; a.cy = cy;
    a.vm = vm; a.image = image; a.opacity = opacity; a.depths = depths; a.feature = feature; a.n_contrib = n_contrib; a.gt = gt;
    a.bg = bg; a.image_mask = image_mask;
    a.w_l1 = w_l1; a.w_pbr = w_pbr; a.w_normal = w_normal; a.scale_image = scale_image; a.scale_pbr = scale_pbr;
    a.pseudo_normal = pseudo_normal; a.surface_xyz = surface_xyz; a.dL_dimage = dL_dimage; a.dL_dopacity = dL_dopacity;
    a.dL_dfeature = dL_dfeature; a.sums = sums; a.ssim_sum_image = ssim_sum_image; a.ssim_sum_pbr = ssim_sum_pbr;
    // three-channel jobs first: the grid's tail is made of the short ones
    s2_image_tail_kernel<<<4 * a.n_tiles, 256, 0, s>>>(a);
    check_launch(s, false, "s2_image_tail_kernel");
}

}  // namespace r3dg
