// The training contact sheet (train.py:276-317 save_training_vis; r3dg_hip.h "r3dg_training_sheet") for gfx950: the finished
// 8-bit picture [out_h,out_w,3] straight from the raw outputs of an eval frame, in ONE streaming launch.  The reference builds
// 7 (stage 1) or 16 (stage 2) float panels, stacks them, runs torchvision's make_grid (nrow 4, padding 2), resamples the grid
// to 800 rows by nearest neighbour and quantises in save_image; here no panel, grid or resampled grid exists: every output byte
// walks that chain BACKWARDS and evaluates one channel of one panel at one source pixel.
//
//   training_sheet_kernel   lane = four consecutive output bytes (one aligned dword of the [out_h,out_w,3] array: parts of at
//                           most two pixels), so a wave's store is 256 contiguous bytes whatever the row length (a row of the
//                           sheet at 800 x 800 is 4797 bytes: no pixel-per-lane layout gives whole lines).  Per byte:
//                             1. nearest-neighbour source of the resample, torch's rule: src = min((int)floorf(dst * scale),
//                                in - 1) with scale = (float)in / out (what view_resize.hip restates for its mask);
//                             2. the make_grid cell of that grid pixel: panel k at y = (k / 4) * (H + 2) + 2,
//                                x = (k % 4) * (W + 2) + 2; padding and cells past the last panel are 0;
//                             3. that panel's expression (capture_math.hpp: the ones eval_capture.hip writes as float maps);
//                             4. the quantisation of r3dg_relight_quantize (glue_math.hpp quantize_byte).
//                           No atomics, no synchronisation, no LDS.  Reads are gathers of 4-byte elements: without a downscale
//                           neighbouring lanes read neighbouring floats of one plane.
#include "capture_math.hpp"
#include "launchers.hpp"
#include "turbo_table.hpp"

namespace r3dg {

namespace {

// feature channels of the two layouts (render.py:91: normal3, depth, depth2; r3dg_relight_pack_features for S = 28)
struct SheetChannels {
    int depth, depth2, normal;
};
__device__ __forceinline__ SheetChannels channels_of(int layout) { return layout == 0 ? SheetChannels{3, 4, 0} : SheetChannels{0, 1, 5}; }

// visualize_depth(depth) with its defaults (utils/image_utils.py:6-21) needs no reduction: near = 0.2 - eps and far = 13 + eps are
// float32 constants (NumPy 2 keeps a Python float beside a float32 scalar in float32), curve(x) = -log(x + eps), and
// min(curve(near), curve(far)) = curve(far), |curve(far) - curve(near)| are the two constants below (NumPy's float32 results;
// tests/golden/make_training_vis_golden.py records them).  -> the bin of matplotlib's colormap call: t * 256 truncated, 256 -> 255.
__device__ __forceinline__ int turbo_bin(float depth)
{
#pragma clang fp contract(off)
    const float eps = 1.1920928955078125e-07f;                 // np.finfo(np.float32).eps
    const float c_far = -0x1.485042p+1f, span = 0x1.0b2928p+2f;     // -log(13), log(13) - log(0.2) as NumPy rounds them
    const float c = -logf(__fadd_rn(depth, eps));
    const float q = __fdiv_rn(__fsub_rn(c, c_far), span);
    const float t = q != q ? 0.f : fminf(fmaxf(q, 0.f), 1.f);  // np.nan_to_num(np.clip(., 0, 1))
    const int bin = (int)__fmul_rn(t, 256.f);
    return bin > 255 ? 255 : bin;
}

struct SheetArgs {
    int W, H, layout, panels, grid_w, grid_h, out_w, out_h, env_rows;
    float scale_x, scale_y, env_scale_x, env_scale_y;          // (float)in / out of the resample and of the env panels
    const float *render, *gt, *opacity, *feature, *pseudo_normal, *background, *env;
    const int* n_contrib;
    size_t n;                                                  // bytes of the sheet
};

// torch's nearest-neighbour source index
__device__ __forceinline__ int nearest_source(int dst, float scale, int in) { return min((int)floorf(__fmul_rn((float)dst, scale)), in - 1); }

// the value of channel c of output pixel (oy, ox) before the quantisation
__device__ float sheet_value(const SheetArgs& a, int oy, int ox, int c)
{
    const int gy = nearest_source(oy, a.scale_y, a.grid_h) - 2, gx = nearest_source(ox, a.scale_x, a.grid_w) - 2;
    if (gy < 0 || gx < 0) return 0.f;                          // the grid's top / left border
    const int H = a.H, W = a.W;
    const int ry = gy / (H + 2), rx = gx / (W + 2);
    const int py = gy - ry * (H + 2), px = gx - rx * (W + 2);
    const int k = ry * 4 + rx;
    if (py >= H || px >= W || k >= a.panels) return 0.f;       // padding between the cells; the empty cell of the stage-1 grid
    const size_t HW = (size_t)W * H, i = (size_t)py * W + px;
    const size_t ci = (size_t)c * HW + i;
    if (k == 0) return a.render[ci];
    if (k == 1) return a.gt[ci];
    if (k == 6) return __fadd_rn(__fmul_rn(a.pseudo_normal[ci], 0.5f), 0.5f);
    if (k >= 14) {                                             // the two halves of F.interpolate(env, (H, 2W)), through sRGB
        const int R = a.env_rows;
        const int sy = nearest_source(py, a.env_scale_y, R), sx = nearest_source(px + (k == 15 ? W : 0), a.env_scale_x, 2 * R);
        return srgb_of(a.env[((size_t)sy * (2 * R) + sx) * 3 + c]);
    }
    const float op = a.opacity[i];
    if (k == 4) return op;
    const float den = capture_divisor(op, a.n_contrib[i]);
    const SheetChannels ch = channels_of(a.layout);
    const float* f = a.feature + i;                            // f[ch * HW]: channel ch of this pixel
    switch (k) {
    case 2: return kTurboTable[turbo_bin(normalised(f[ch.depth * HW], den))][c];
    case 3: {
        const float q = __fdiv_rn(variance_of(normalised(f[ch.depth * HW], den), normalised(f[ch.depth2 * HW], den)), 0.001f);
        return q > 1.f ? 1.f : q;                              // clamp_max(1); a NaN stays one (and quantises to 0)
    }
    case 5: return __fadd_rn(__fmul_rn(normalised(f[(ch.normal + c) * HW], den), 0.5f), 0.5f);
    case 7: return srgb_of(normalised(f[(8 + c) * HW], den));                   // base colour
    case 8: return normalised(f[11 * HW], den);                                 // roughness
    case 9: return normalised(f[27 * HW], den);                                 // visibility
    case 10: return srgb_of(normalised(f[(12 + c) * HW], den));                 // diffuse
    case 11: return srgb_of(normalised(f[(15 + c) * HW], den));                 // specular
    case 12: return srgb_of(normalised(f[(24 + c) * HW], den));                 // global lights
    default: return pbr_over_background(normalised(f[(2 + c) * HW], den), op, a.background[c]);       // 13: pbr
    }
}

__global__ void __launch_bounds__(256)
training_sheet_kernel(SheetArgs a, uint8_t* __restrict__ bytes)
{
    const size_t b0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (b0 >= a.n) return;
    const unsigned p0 = (unsigned)(b0 / 3);                    // (fewer than 2^31 pixels)
    int c = (int)(b0 - (size_t)p0 * 3);
    int oy = (int)(p0 / (unsigned)a.out_w), ox = (int)(p0 - (unsigned)oy * (unsigned)a.out_w);
    const int count = a.n - b0 < 4 ? (int)(a.n - b0) : 4;
    uint32_t word = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (j < count) {
            word |= (uint32_t)quantize_byte(sheet_value(a, oy, ox, c)) << (8 * j);
            if (++c == 3) {
                c = 0;
                if (++ox == a.out_w) { ox = 0; oy++; }
            }
        }
    }
    if (count == 4) {
        *reinterpret_cast<uint32_t*>(bytes + b0) = word;       // (bytes is 4-byte aligned: checked by the entry point)
    } else {
#pragma unroll
        for (int j = 0; j < 3; j++)
            if (j < count) bytes[b0 + j] = (uint8_t)(word >> (8 * j));
    }
}

}  // namespace

void launch_training_sheet(hipStream_t s, int W, int H, int layout, const float* render, const float* gt, const float* opacity,
                           const int* n_contrib, const float* feature, const float* pseudo_normal, const float* background,
                           const float* env, int env_rows, int out_w, int out_h, uint8_t* bytes)
{
    SheetArgs a = {};
    a.W = W, a.H = H, a.layout = layout, a.panels = layout == 0 ? 7 : 16;
    a.grid_h = ((a.panels + 3) / 4) * (H + 2) + 2, a.grid_w = 4 * (W + 2) + 2;
    a.out_w = out_w, a.out_h = out_h, a.env_rows = env_rows;
    // torch's scale of a resample to a given size: static_cast<float>(input_size) / output_size
    a.scale_x = (float)a.grid_w / (float)out_w, a.scale_y = (float)a.grid_h / (float)out_h;
    if (layout == 1) a.env_scale_x = (float)(2 * env_rows) / (float)(2 * W), a.env_scale_y = (float)env_rows / (float)H;
    a.render = render, a.gt = gt, a.opacity = opacity, a.feature = feature, a.pseudo_normal = pseudo_normal;
    a.background = background, a.env = env, a.n_contrib = n_contrib;
    a.n = (size_t)out_w * out_h * 3;
    const size_t lanes = (a.n + 3) / 4;
    training_sheet_kernel<<<(unsigned)((lanes + 255) / 256), 256, 0, s>>>(a, bytes);
    check_launch(s, false, "training_sheet_kernel");
}

}  // namespace r3dg
