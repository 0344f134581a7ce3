// Scores of a held-out view on the device (eval_nvs.py:49-82, eval_relighting_syn4.py:140-224) for gfx950: what is left of
// the metrics once the SSIM tiling (ssim.hip: eval_image_metrics_kernel, one (squared error, SSIM sum) pair of doubles per
// workgroup) has run, and the albedo scale.  Every result goes into a row of the caller's metrics table (R3DG_EVAL_ROW doubles),
// which the host reads once, after the last view.
//
//   eval_metrics_finalize_kernel     ONE workgroup adds the tile totals of each channel in a fixed order (strided per thread,
//                                    then an LDS tree) and writes mse_c, the SSIM sum, psnr = mean_c 20 log10(1 / sqrt(mse_c))
//                                    (utils/image_utils.py:24-29) and ssim = sum / (C H W).  No float atomics anywhere on this
//                                    path: two runs give the same bits.
//   eval_median_histogram_kernel /   masked per-channel LOWER median (index (n - 1) / 2 of the sorted values, what torch.median
//   eval_median_select_kernel        returns) of gt / clamp(pred, 1e-6, 1) (eval_relighting_syn4.py:201) as an 8-bit radix select
//                                    on the float bit patterns -- the ratios are non-negative, so their bits order them.  Four
//                                    passes from the top byte down; a pass recomputes the ratios from the two images (they are
//                                    never stored), counts the byte below the prefix found so far in LDS histograms and adds
//                                    each non-empty bin to the 3 x 256 table with one integer atomic per workgroup; the select
//                                    kernel then picks the bin that holds the wanted rank ON THE DEVICE (no read-back between
//                                    passes) and clears the table for the next pass.
#include "launchers.hpp"

namespace r3dg {

__global__ void __launch_bounds__(256)
eval_metrics_finalize_kernel(int tiles, int C, double inv_hw, const double* __restrict__ tile_sums, double* __restrict__ row)
{
    __shared__ double s_a[256], s_b[256];
    double psnr_sum = 0.0, ssim_sum = 0.0;
    for (int c = 0; c < C; c++) {
        const double* t = tile_sums + 2 * (size_t)c * tiles;
        double a = 0.0, b = 0.0;
        for (int k = threadIdx.x; k < tiles; k += 256) { a += t[2 * (size_t)k]; b += t[2 * (size_t)k + 1]; }
        s_a[threadIdx.x] = a;
        s_b[threadIdx.x] = b;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) { s_a[threadIdx.x] += s_a[threadIdx.x + o]; s_b[threadIdx.x] += s_b[threadIdx.x + o]; }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            const double mse = s_a[0] * inv_hw;
            row[c] = mse;
            psnr_sum += 20.0 * log10(1.0 / sqrt(mse));
            ssim_sum += s_b[0];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        for (int c = C; c < 3; c++) row[c] = 0.0;
        row[3] = ssim_sum;
        row[4] = psnr_sum / C;
        row[5] = ssim_sum * inv_hw / C;
        row[6] = (double)C;
        row[7] = 0.0;
    }
}

// ---- masked median of the albedo ratio ---------------------------------------------------------------------------------
// state (R3DG_EVAL_MEDIAN_STATE_WORDS uint32): [0, 768) the 3 x 256 histogram, 768.. the prefix found so far per channel,
// 771.. the rank still wanted inside that prefix, 774 the number of selected pixels
constexpr int MED_PREFIX = 768, MED_RANK = 771, MED_N = 774;

__device__ __forceinline__ uint32_t ratio_bits(float gt, float pred)
{
    // (+ 0: a negative zero would sort behind every positive value)
    return __float_as_uint(__fdiv_rn(gt, fminf(fmaxf(pred, 1e-6f), 1.f)) + 0.f);
}

__global__ void __launch_bounds__(256)
eval_median_histogram_kernel(int HW_, int shift, const float* __restrict__ pred, const float* __restrict__ gt,
                             const float* __restrict__ mask, uint32_t* __restrict__ state)
{
    __shared__ uint32_t s_h[3 * 256];
    __shared__ uint32_t s_prefix[3];
    for (int j = threadIdx.x; j < 3 * 256; j += 256) s_h[j] = 0u;
    if (threadIdx.x < 3) s_prefix[threadIdx.x] = state[MED_PREFIX + threadIdx.x];
    __syncthreads();
    const uint32_t above = shift == 24 ? 0u : 0xffffffffu << (shift + 8);     // the bytes earlier passes have fixed
    const size_t HW = (size_t)HW_;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < HW; i += (size_t)gridDim.x * 256) {
        if (mask != nullptr && !(mask[i] > 0.f)) continue;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const uint32_t bits = ratio_bits(gt[c * HW + i], pred[c * HW + i]);
            if ((bits & above) == s_prefix[c]) atomicAdd(&s_h[c * 256 + ((bits >> shift) & 255u)], 1u);
        }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < 3 * 256; j += 256) {
        const uint32_t v = s_h[j];
        if (v != 0u) atomicAdd(&state[j], v);
    }
}

__global__ void __launch_bounds__(256)
eval_median_select_kernel(int shift, uint32_t* __restrict__ state, double* __restrict__ row)
{
    __shared__ uint32_t s_h[3 * 256];
    for (int j = threadIdx.x; j < 3 * 256; j += 256) {
        s_h[j] = state[j];
        state[j] = 0u;                              // ready for the next pass
    }
    __syncthreads();
    if (threadIdx.x >= 3) return;
    const int c = threadIdx.x;
    uint32_t n, rank;
    if (shift == 24) {                              // first pass: every selected pixel was counted
        n = 0u;
        for (int b = 0; b < 256; b++) n += s_h[c * 256 + b];
        rank = n != 0u ? (n - 1u) / 2u : 0u;
        if (c == 0) state[MED_N] = n;
    } else {
        n = state[MED_N];
        rank = state[MED_RANK + c];
    }
    uint32_t prefix = state[MED_PREFIX + c];
    if (n != 0u) {
        uint32_t below = 0u;
        int b = 0;
        for (; b < 255; b++) {
            const uint32_t h = s_h[c * 256 + b];
            if (below + h > rank) break;
            below += h;
        }
        prefix |= (uint32_t)b << shift;
        state[MED_PREFIX + c] = prefix;
        state[MED_RANK + c] = rank - below;
    }
    if (shift == 0) {
        row[c] = n != 0u ? (double)__uint_as_float(prefix) : (double)__uint_as_float(0x7fc00000u);
        if (c == 0) {
            row[3] = (double)n;
            row[4] = row[5] = row[6] = row[7] = 0.0;
        }
    }
}

void launch_eval_image_metrics(hipStream_t s, int W, int H, int C, const float* pred, const float* gt, const float* mask,
                               const float* fill, int fill_is_image, double* tile_sums, double* row)
{
    launch_eval_metric_tiles(s, W, H, C, pred, gt, mask, fill, fill_is_image, tile_sums);
    const int tiles = ((W + 31) / 32) * ((H + 31) / 32);
    eval_metrics_finalize_kernel<<<1, 256, 0, s>>>(tiles, C, 1.0 / ((double)W * (double)H), tile_sums, row);
    check_launch(s, false, "eval_metrics_finalize_kernel");
}

void launch_eval_median_ratio(hipStream_t s, int W, int H, const float* pred, const float* gt, const float* mask,
                              uint32_t* state, double* row)
{
    const int HW = W * H;
    R3DG_HIP(hipMemsetAsync(state, 0, R3DG_EVAL_MEDIAN_STATE_WORDS * sizeof(uint32_t), s));
    const int blocks = HW > 0 ? (int)(((size_t)HW + 1023) / 1024 < 1024 ? ((size_t)HW + 1023) / 1024 : 1024) : 1;
    for (int shift = 24; shift >= 0; shift -= 8) {
        eval_median_histogram_kernel<<<blocks, 256, 0, s>>>(HW, shift, pred, gt, mask, state);
        check_launch(s, false, "eval_median_histogram_kernel");
        eval_median_select_kernel<<<1, 256, 0, s>>>(shift, state, row);
        check_launch(s, false, "eval_median_select_kernel");
    }
}

}  // namespace r3dg
