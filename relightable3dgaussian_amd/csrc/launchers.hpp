// Host functions that one translation unit of libr3dg_hip.so defines for another to call (the kernel launchers and the few
// queries beside them; the callers are the C-ABI wrappers in capi_*.hip), each declared here ONCE.  Every file that defines
// one includes this header, so a definition that drifts from its declaration stands next to it and fails to link.
#pragma once
#include "common.hpp"

namespace r3dg {

// CUs a persistent grid may fill: the device's CUs minus the R3DG_OPT_RESERVE_CUS left to a collective running beside it on
// another stream, at least 1 (capi_core.hip; library-internal, not part of the exported surface)
__attribute__((visibility("hidden"))) int persistent_cus();

void release_gradient_records();        // rasterizer_render_bwd.hip; the device is idle when r3dg_release_scratch calls it
void launch_mark_visible(hipStream_t s, int P, const float* means3D, const float* vm, uint8_t* present);
void launch_preprocess(hipStream_t s, int P, int D, int M, const float* means3D, const float* scales, float scale_modifier,
                       const float* rotations, const float* opacities, const float* shs, uint8_t* clamped,
                       const float* cov3D_precomp, const float* colors_precomp, const float* vm, const float* pm,
                       const float* cam_pos, int W, int H, float tan_fovx, float tan_fovy, float focal_x, float focal_y,
                       int* radii, float* means2D, float* depths, float* cov3Ds, float* rgb, float* conic_opacity,
                       float* splat, int gx, int gy, uint32_t* tiles_touched, uint32_t* block_sums,
                       unsigned long long* total, bool scan_now, uint32_t* zero_words, int zero_n);
void launch_duplicate_with_keys(hipStream_t s, int P, const float* means2D, const float* depths,
                                const uint32_t* tiles_touched, const uint32_t* block_offsets, uint32_t* point_offsets,
                                uint64_t* keys, uint32_t* values, const int* radii, int gx, int gy);
void launch_identify_tile_ranges(hipStream_t s, int L, const uint64_t* keys, uint32_t* ranges);
void launch_tile_order(hipStream_t s, int T, const uint32_t* ranges, uint32_t* order, uint32_t small_cap, uint32_t* big_list,
                       uint32_t* big_count);
void launch_render_forward(hipStream_t s, int W, int H, int S, const uint32_t* tile_order, const uint32_t* ranges,
                           const uint32_t* point_list, const float* splat, const float* features, float* final_T,
                           uint32_t* n_contrib, const float* bg, float* out_color, float* out_opacity, float* out_depth,
                           float* out_feature, float* out_weights);
void launch_pseudo_normal(hipStream_t s, int W, int H, const float* vm, float focal_x, float focal_y, float cx, float cy,
                          const float* opacities, const float* depths, float* normals, float* surface_xyz, bool debug);
void launch_render_backward(hipStream_t s, int P, int W, int H, int S, int n_active, const int* active,
                            const uint32_t* tile_order, const uint32_t* ranges, const uint32_t* point_list, const float* bg,
                            const float* splat, const float* features, const float* final_Ts, const uint32_t* n_contrib,
                            const float* dL_dpix, const float* dL_dpix_o, const float* dL_dpix_d, const float* dL_dpix_f,
                            float* dL_dmean2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolor, float* dL_dfeature,
                            int bg_geom);
// launch_render_backward is (a) + (c) of three parts (rasterizer_render_bwd.hip):
//   (a) launch_render_backward_fill: the tile kernel adds into the per-Gaussian gradient records of stream `s` (library scratch,
//       zero between calls) -> the records; `tiles` false (nothing was rendered): no launch, the rows are zeros;
//   (b) GradRecordLayout: the record channel of every value the tile kernel left (-1: not carried, the value is +0.f) -- what a
//       kernel that reads the rows in place needs (r3dg_hip.h: the same R3DG_GRAD_RECORD_LAYOUT_INTS ints, in this order);
//   (c) launch_gradient_records_scatter: rows -> the op's five arrays, zeros -> the rows.
// Between (a) and the launch that zeroes the rows the buffer counts as dirty; (c) and gradient_records_zeroed end that.
struct GradRecordLayout {
    int nvp;                         // floats per record
    int color[3];
    int sx, sy, depth;               // first moments; the depth side channel (-1 in the instances without one)
    int sxx, sxy, syy, opacity;
    int feature[R3DG_MAX_S_BWD];     // by feature column
};
static_assert(sizeof(GradRecordLayout) == R3DG_GRAD_RECORD_LAYOUT_INTS * sizeof(int), "GradRecordLayout is the C ABI's int array");
GradRecordLayout render_backward_layout(int S, int n_active, const int* active, bool depth_gradient, int bg_geom);
float* launch_render_backward_fill(hipStream_t s, int P, int W, int H, int S, int n_active, const int* active,
                                   const uint32_t* tile_order, const uint32_t* ranges, const uint32_t* point_list,
                                   const float* bg, const float* splat, const float* features, const float* final_Ts,
                                   const uint32_t* n_contrib, const float* dL_dpix, const float* dL_dpix_o,
                                   const float* dL_dpix_d, const float* dL_dpix_f, int bg_geom, bool tiles,
                                   GradRecordLayout* layout);
void launch_gradient_records_scatter(hipStream_t s, int P, int S, float* rec, const GradRecordLayout& layout, float* dL_dmean2D,
                                     float* dL_dconic, float* dL_dopacity, float* dL_dcolor, float* dL_dfeature);
bool gradient_record_layout_valid(const GradRecordLayout& layout, int S);
void gradient_records_zeroed(const float* rec);
void launch_render_backward_features(hipStream_t s, int W, int H, int S, int n_active, const int* active,
                                     const uint32_t* tile_order, const uint32_t* ranges, const uint32_t* point_list,
                                     const float* splat, const float* final_Ts, const uint32_t* n_contrib,
                                     const float* dL_dpix_f, float* dL_dfeature);
// the SH colour group's Adam step as the projection backward applies it itself (`g.param` IS its `shs`; `g.grad` is not read:
// the gradient rows are in LDS); the bias corrections from adam_bias (adam_update.hpp)
struct ShAdamArgs {
    r3dg_adam_group g;
    float beta1, beta2, eps, bias1, inv_sqrt_bias2, grad_scale;
    const float* skip_flag;
};
bool preprocess_backward_applies_adam(int M);
// Where the per-Gaussian kernel finds the sums the tile backward left for Gaussian g: value k of a group at
// base[g * stride + off[k]].  Either the op's arrays (dL_dmean2D [P,3], dL_dconic [P,4], dL_dcolor [P,3]: tile_grad_arrays) or the
// gradient record rows, read in place (tile_grad_records).  `records` != 0 also means that nothing has written dL_dmean2D yet:
// the kernel then writes all three of its columns, for Gaussians outside the view too.
struct TileGradSource {
    const float* mean2D;
    const float* conic;
    const float* color;
    int mean2D_stride, conic_stride, color_stride;
    int sx, sy, depth;               // depth < 0: the side channel is +0.f
    int sxx, sxy, syy;
    int c[3];
    int records;
};
inline TileGradSource tile_grad_arrays(const float* dL_dmean2D, const float* dL_dconic, const float* dL_dcolor)
{
    return TileGradSource{dL_dmean2D, dL_dconic, dL_dcolor, 3, 4, 3, 0, 1, 2, 0, 1, 3, {0, 1, 2}, 0};
}
inline TileGradSource tile_grad_records(const float* rec, const GradRecordLayout& L)
{
    return TileGradSource{rec, rec, rec, L.nvp, L.nvp, L.nvp, L.sx, L.sy, L.depth, L.sxx, L.sxy, L.syy,
                          {L.color[0], L.color[1], L.color[2]}, 1};
}
// `adam` != nullptr: dL_dsh is NOT written; parameters and moments of the group are updated in place instead.
// `records` != nullptr: the tile backward's sums are read from the record rows (`layout`), not from dL_dmean2D / dL_dconic /
// dL_dcolor (the latter two may then be NULL); dL_dmean2D is written in full.
void launch_preprocess_backward(hipStream_t s, int P, int D, int M, const float* means, const int* radii, const float* shs,
                                const uint8_t* clamped, const float* scales, const float* rotations, float scale_modifier,
                                const float* cov3Ds, const float* vm, const float* proj, float h_x, float h_y,
                                float tan_fovx, float tan_fovy, const float* campos, float* dL_dmean2D,
                                const float* dL_dconic, const float* conic_opacity, int W, int H, float* dL_dmeans,
                                const float* dL_dcolor, float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot,
                                const ShAdamArgs* adam, const float* records = nullptr,
                                const GradRecordLayout* layout = nullptr);
void launch_shade_forward(hipStream_t s, int P, int K, int M, const float* base_color, const float* roughness,
                          const float* normals, const float* viewdirs, const float* incidents, const float* env, int He,
                          int We, const float* tr, const float* visibility, const float* dirs, const float* areas,
                          float* out, const uint32_t* taps, bool train_outputs, float uniform_area, bool taps_are_radiance,
                          bool leave_room);
size_t shade_frs_table_floats(int K);
bool shade_frs_supported(int K, int M, int He, int We);
void launch_shade_frs_build_tables(hipStream_t s, int K, const float* zsamples, float* tables);
void launch_shade_frs_classify(hipStream_t s, int P, const float* ray_normals, uint8_t* valid);
void launch_shade_frs_build_taps(hipStream_t s, int P, int K, const float* ray_normals, const float* zsamples, int He,
                                 int We, uint32_t* taps);
void launch_shade_frs_forward_aux(hipStream_t s, int P, const float* incidents, const float* ray_normals, float* cprime);
void launch_shade_frs_forward_main(hipStream_t s, int P, int K, const float* base_color, const float* roughness,
                                   const float* normals, const float* viewdirs, const float* env, int He, int We,
                                   const float* visibility, float uniform_area, const uint32_t* taps,
                                   const float* ray_normals, const float* tables, const uint8_t* valid, const float* cprime,
                                   bool leave_room, float* out, float* feat);
void launch_shade_frs_forward_listed(hipStream_t s, int K, const float* base_color, const float* roughness,
                                     const float* normals, const float* viewdirs, const float* incidents, const float* env,
                                     int He, int We, const float* visibility, const float* ray_normals,
                                     const float* zsamples, float uniform_area, const int* invalid_list, int n_invalid,
                                     float* out, float* feat);
void launch_shade_frs_incident_chain(hipStream_t s, int P, const float* ray_normals, const uint8_t* valid, const float* dcp,
                                     float* d_inc, float* incidents, float* exp_avg, float* exp_avg_sq, float* cprime,
                                     float lr, float lr_tail, float beta1, float beta2, float eps, int step,
                                     float grad_scale, const float* skip_flag, int listed_in_dcprime, bool write_gradient);
const unsigned int* launch_shade_frs_backward_aux(hipStream_t s, int P, const float* g_pbr, const float* g_diff,
                                                  const float* block_absmax, int n_block_absmax, int* gmax_n);
void launch_shade_frs_backward_main(hipStream_t s, int P, int K, const float* base_color, const float* roughness,
                                    const float* normals, const float* viewdirs, const float* env, int He, int We,
                                    const float* visibility, float uniform_area, const uint32_t* taps,
                                    const float* ray_normals, const float* tables, const uint8_t* valid, const float* cprime,
                                    float* dcp, const float* g_pbr, const float* g_diff, float* d_base, float* d_rough,
                                    float* d_view, float* d_env, const unsigned int* gmax, int gmax_n);
void launch_shade_frs_backward_rotate(hipStream_t s, int P, const float* ray_normals, const float* dcp, float* d_inc,
                                      const uint8_t* valid);
void launch_shade_frs_backward_listed(hipStream_t s, int K, const float* base_color, const float* roughness,
                                      const float* normals, const float* viewdirs, const float* incidents, const float* env,
                                      int He, int We, const float* visibility, const float* ray_normals,
                                      const float* zsamples, float uniform_area, const int* invalid_list, int n_invalid,
                                      const float* g_pbr, const float* g_diff, float* d_base, float* d_rough, float* d_view,
                                      float* d_inc, float* d_env, const unsigned int* gmax, int gmax_n);
void launch_shade_build_taps(hipStream_t s, size_t n, const float* dirs, const float* tr, int He, int We, const float* env,
                             uint32_t* taps);
void launch_shade_build_split(hipStream_t s, int P, int K, const int* perm, const float* normals, const float* incidents,
                              const float* visibility, const float* dirs, const float* zsamples, float uniform_area,
                              float* lt, float* vis_t, float* consts);
void launch_shade_forward_split(hipStream_t s, int P, int K, const int* perm, const float* base_color,
                                const float* roughness, const float* normals, const float* viewdirs, const float* lt,
                                const float* vis_t, const float* consts, const float* zsamples, const float* tr,
                                const float* env4, int He, int We, float* out);
void launch_shade_env_footprints(hipStream_t s, int He, int We, const float* env, float* fp);
void launch_shade_build_transport(hipStream_t s, int P, int K, int M, const float* normals, const float* incidents,
                                  const float* visibility, const float* dirs, const float* areas, float uniform_area,
                                  float* radiance_to_transport, float* consts);
void launch_shade_build_transport_rayset(hipStream_t s, int P, int K, int M, const float* normals, const float* incidents,
                                         const float* visibility, const float* zsamples, float uniform_area, const float* env,
                                         int He, int We, const float* tr, float* transport, float* consts);
void launch_shade_build_transport_baked(hipStream_t s, int P, int K, int M, const float* normals, const float* incidents,
                                        const float* visibility_sh, const float* zsamples, float uniform_area, const float* env,
                                        int He, int We, const float* tr, float* transport, float* consts);
void launch_visibility_sh_expand(hipStream_t s, int P, int K, const float* normals, const float* zsamples,
                                 const float* visibility_sh, float* out);
void launch_shade_forward_transport(hipStream_t s, int P, int K, const float* base_color, const float* roughness,
                                    const float* normals, const float* viewdirs, const float* transport, const float* consts,
                                    const float* zsamples, const float* dirs, float* out);
void launch_shade_backward(hipStream_t s, int P, int K, int M, const float* base_color, const float* roughness,
                           const float* normals, const float* viewdirs, const float* incidents, const float* env, int He,
                           int We, const float* tr, const float* visibility, const float* dirs, const float* areas,
                           const float* g_pbr, const float* g_diff, float* d_base, float* d_rough, float* d_view,
                           float* d_inc, float* d_env, const uint32_t* taps, const float* block_absmax, int n_block_absmax);
void launch_re_forward(hipStream_t s, bool complex_, int P, int Si, int Sd, int Sv, const float* base_color,
                       const float* roughness, const float* metallic, const float* normals, const float* viewdirs,
                       const float* inc, const float* direct, const float* vis, int K, const float* rand_float,
                       float* incident_dirs, float* out_pbr, float* out_lights, float* out_local, float* out_global,
                       float* out_vis, float* out_diffuse, float* out_local_diffuse, float* out_accum, float* out_rgb_d,
                       float* out_rgb_s);
void launch_re_backward(hipStream_t s, int P, int Si, int Sd, int Sv, const float* base_color, const float* roughness,
                        const float* metallic, const float* normals, const float* viewdirs, const float* inc,
                        const float* direct, const float* vis, int K, const float* incident_dirs, const float* dL_dpbr,
                        const float* dL_ddl, float* dL_dbase, float* dL_drough, float* dL_dmetal, float* dL_dnormals,
                        float* dL_dviewdirs, float* dL_dinc, float* dL_ddirect, float* dL_dvis);
void launch_s2_activate(hipStream_t s, int P, const float* xyz, const float* scaling_raw, const float* rotation_raw,
                        const float* opacity_raw, const float* normal_raw, const float* base_raw, const float* rough_raw,
                        const float* campos, float* scales, float* rot, float* opacity, float* normal, float* base_color,
                        float* roughness, float* viewdirs, const float* viewmatrix, float* features, int n_env,
                        const float* env_raw, float* env, float* zero, int n_zero);
void launch_s2_pack(hipStream_t s, int P, const float* xyz, const float* viewmatrix, const float* normal,
                    const float* base_color, const float* roughness, const float* shade_out, float* features,
                    float* light_l1_sum);
void launch_s2_unpack(hipStream_t s, int P, const float* dL_dfeatures, const float* shade_out, float light_weight,
                      float* dL_dpbr, float* dL_ddiffuse, float* block_absmax, float* light_l1_sum,
                      const float* records = nullptr, const GradRecordLayout* layout = nullptr);
// `records` + `layout` (16-float rows): the feature columns and the opacity gradient are read from the gradient record rows, not
// from dL_dfeatures / dL_dopacity (which may then be NULL); launch_s2_activate_backward, the last reader, zeroes the rows
void launch_s2_activate_backward(hipStream_t s, int P, const float* xyz, const float* scaling_raw, const float* rotation_raw,
                                 const float* opacity_raw, const float* normal_raw, const float* base_raw,
                                 const float* rough_raw, const float* viewmatrix, const float* campos,
                                 const float* dL_dfeatures, const float* dL_dbase_shade, const float* dL_drough_shade,
                                 const float* dL_dviewdirs, const float* dL_dscales, const float* dL_drot,
                                 const float* dL_dopacity, const float* dL_dmeans3D, float* g_xyz, float* g_scaling,
                                 float* g_rotation, float* g_opacity, float* g_normal, float* g_base, float* g_rough, int He,
                                 int We, const float* env_raw, const float* env, float* dL_denv, float w_tv,
                                 float* g_env_raw, float* tv_sum, int consume, float* records = nullptr,
                                 const GradRecordLayout* layout = nullptr);
void launch_s2_loss(hipStream_t s, int HW, const float* image, const float* opacity, const float* feature,
                    const float* pseudo_normal, const int* n_contrib, const float* gt, const float* bg,
                    const float* image_mask, float w_l1, float w_pbr, float w_normal, const float* extra_dimage,
                    const float* extra_dsrgb, float* dL_dimage, float* dL_dopacity, float* dL_dfeature, float* sums,
                    int sparse);
void launch_s2_smooth_forward(hipStream_t s, int W, int H, const float* opacity, const float* feature, const int* n_contrib,
                              const float* gt, const float* image_mask, float w_base, float w_rough, float w_light,
                              float* scratch, float* sums3);
void launch_s2_smooth_fused(hipStream_t s, int W, int H, const float* opacity, const float* feature, const int* n_contrib,
                            const float* gt, const float* image_mask, float w_base, float w_rough, float w_light,
                            int accumulate_normal, float* dL_dopacity, float* dL_dfeature, float* sums3);
void launch_s2_smooth_backward(hipStream_t s, int W, int H, const float* opacity, const float* feature, const int* n_contrib,
                               const float* image_mask, const float* scratch, int has_base, int has_rough, int has_light,
                               int accumulate_normal, float* dL_dopacity, float* dL_dfeature);
void launch_s2_pbr_srgb(hipStream_t s, int HW, const float* opacity, const float* feature, const int* n_contrib,
                        const float* bg, float* srgb);
void launch_s2_normals_srgb(hipStream_t s, int W, int H, const float* vm, float focal_x, float focal_y, float cx, float cy,
                            const float* opacity, const float* depths, float* normals, float* surface_xyz,
                            const float* feature, const int* n_contrib, const float* bg, float* srgb);
bool image_tail_applies(int W, int H);
void launch_s2_image_tail(hipStream_t s, int W, int H, const float* vm, float focal_x, float focal_y, float cx, float cy,
                          const float* image, const float* opacity, const float* depths, const float* feature, const int* n_contrib,
                          const float* gt, const float* bg, const float* image_mask, float w_l1, float w_pbr, float w_normal,
                          float scale_image, float scale_pbr, float* pseudo_normal, float* surface_xyz, float* dL_dimage,
                          float* dL_dopacity, float* dL_dfeature, float* sums, float* ssim_sum_image, float* ssim_sum_pbr);
void launch_ssim_forward(hipStream_t s, int W, int H, int C, int n_images, const float* const* x, const float* y,
                         float* const* partials, float* const* sum);
void launch_ssim_backward(hipStream_t s, int W, int H, int C, int n_images, const float* const* x, const float* y,
                          float* const* partials, const float* scale, float* const* grad_x);
void launch_adam(hipStream_t s, int n_groups, const r3dg_adam_group* groups, float beta1, float beta2, float eps, int step,
                 float grad_scale, const float* skip_flag);
void launch_s1_pack(hipStream_t s, int P, const float* xyz, const float* viewmatrix, const float* normal, float* features);
void launch_s1_edge(hipStream_t s, int W, int H, const float* feature, const float* opacity, const int* n_contrib,
                    const float* gt, float* edge_g, float* sum_out);
void launch_s1_loss(hipStream_t s, int W, int H, const float* image, const float* opacity, const float* feature,
                    const float* pseudo_normal, const int* n_contrib, const float* gt, const float* image_mask, float w_l1,
                    float w_entropy, float w_normal, float w_smooth, float w_var, const float* extra_dimage,
                    const float* edge_g, float* dL_dimage, float* dL_dopacity, float* dL_dfeature, float* sums);
void launch_s1_activate_backward(hipStream_t s, int P, const float* xyz, const float* scaling_raw, const float* rotation_raw,
                                 const float* opacity_raw, const float* normal_raw, const float* viewmatrix,
                                 const float* dL_dfeatures, const float* dL_dscales, const float* dL_drot,
                                 const float* dL_dopacity, const float* dL_dmeans3D, float* g_xyz, float* g_scaling,
                                 float* g_rotation, float* g_opacity, float* g_normal);
void launch_s2_env_backward(hipStream_t s, int He, int We, const float* raw, const float* env, float* dL_denv, float w_tv,
                            float* g_raw, float* tv_sum, int consume);
uint32_t tile_sort_small_cap();
void launch_tile_sort(hipStream_t s, int T, const uint32_t* tile_order, const uint32_t* ranges, const uint32_t* big_list,
                      uint32_t* big_count, uint64_t* keys, uint32_t* vals, uint64_t* scratch, bool entries);
void launch_tile_binning(hipStream_t s, int P, int T, const float* means2D, const float* depths, const int* radii,
                         const uint32_t* tiles_touched, uint32_t* block_offsets, int gx, int gy, uint32_t* tile_counts,
                         uint32_t* cursor, uint32_t* ranges, uint32_t* point_offsets, uint64_t* entries,
                         unsigned long long* total, long long capacity, float* overflow_flag, unsigned int* overflow_count,
                         bool fused, uint32_t* order, uint32_t small_cap, uint32_t* big_list, uint32_t* big_count);
int tile_binning_max_tiles();
void launch_densify_accumulate(hipStream_t s, int P, const float* viewspace_grad, const float* normal_grad, const int* radii,
                               const float* weights, float* xyz_accum, float* normal_accum, float* denom,
                               float* weights_accum, float* max_radii2D, const float* skip_flag);
size_t densify_temp_bytes(size_t P);
void launch_densify_plan(hipStream_t s, int P, const r3dg_densify_config& cfg, const float* scaling_raw,
                         const float* opacity_raw, const float* xyz_accum, const float* normal_accum, const float* denom,
                         const float* weights_accum, const float* max_radii2D, int32_t* src_row, int32_t* kind,
                         int32_t* counts, void* temp);
void launch_densify_gather(hipStream_t s, int P_out, const int32_t* src_row, const int32_t* kind, int n_groups,
                           const r3dg_densify_group* groups, const float* xyz, const float* scaling_raw,
                           const float* rotation_raw, const float* normal_table, float split_divisor);
void launch_reset_opacity(hipStream_t s, int P, float cap, float* opacity_raw, float* exp_avg, float* exp_avg_sq);
void launch_relight_pack(hipStream_t s, int P, const float* xyz, const float* viewmatrix, const float* normal,
                         const float* base_color, const float* roughness, const float* shade_out, float* features);
void launch_relight_compose(hipStream_t s, int W, int H, float fx, float fy, float cx, float cy, const float* viewmatrix,
                            const float* tr, const float* env, int He, int We, const float* image, const float* opacity,
                            const float* feature, const int* n_contrib, float* pbr_env, float* render_env, float* env_only);
// eval_capture.hip: the capture maps of an eval frame, each [3,HW] or [1,HW]; NULL = not wanted
struct CaptureMaps {
    float *pbr, *base_color, *roughness, *normal, *visibility, *diffuse, *specular, *lights, *local_lights, *global_lights,
        *depth_var;
};
void launch_relight_capture(hipStream_t s, int W, int H, const float* feature, const float* opacity, const int* n_contrib,
                            const float* background, const float* mask, const CaptureMaps& maps);
// scene_assembly.hip: PLY records <-> the 13 parameter groups (r3dg_hip.h "scene assembly"); a NULL entry = absent group
struct SceneGroups {
    float* p[R3DG_SCENE_GROUPS];
};
void launch_scene_place_records(hipStream_t s, int P, int A, const float* records, const int* column_map, const float* placement,
                                int flags, long long row_offset, const SceneGroups& dst);
void launch_scene_place_groups(hipStream_t s, int P, const SceneGroups& src, const float* placement, int flags,
                               long long row_offset, const SceneGroups& dst);
void launch_scene_pack_records(hipStream_t s, int P, int columns, const SceneGroups& src, float* records);
void launch_relight_quantize(hipStream_t s, int W, int H, int C, const float* image, uint8_t* bytes);
// training_sheet.hip: the 8-bit training contact sheet [out_h,out_w,3] from an eval frame's raw outputs (layout 0: S = 5, 7 panels;
// 1: S = 28, 16 panels, with the activated environment texture env [env_rows,2 env_rows,3]); bytes 4-byte aligned
void launch_training_sheet(hipStream_t s, int W, int H, int layout, const float* render, const float* gt, const float* opacity,
                           const int* n_contrib, const float* feature, const float* pseudo_normal, const float* background,
                           const float* env, int env_rows, int out_w, int out_h, uint8_t* bytes);
// png_encode.hip: the zlib stream of the PNG file of bytes [H,W,C] (filter, table-driven deflate per row segment, Adler-32) in three
// launches; scratch of png_scratch_bytes, 16-byte aligned; zlib of png_zlib_bound bytes at least; the shape is checked by the caller
long long png_zlib_bound(int W, int H, int C);
long long png_scratch_bytes(int W, int H, int C);
void launch_png_encode(hipStream_t s, int W, int H, int C, const uint8_t* bytes, const uint32_t* code_table,
                       const uint8_t* block_header, int header_bits, uint8_t* scratch, uint8_t* zlib, int32_t* zlib_bytes);
// view_store.hip: 8-bit pixels [H,W,C] of a stored ground-truth view -> image [3,H,W] over the background + mask [1,H,W] (or NULL)
void launch_view_unpack(hipStream_t s, int W, int H, int C, const uint8_t* pixels, const float* background, float* image,
                        float* mask);
// ... the same for RGB pixels [H,W,3] with a one-byte mask plane [H,W] of their own (no background)
void launch_view_unpack_masked(hipStream_t s, int W, int H, const uint8_t* pixels, const uint8_t* mask_bytes, float* image,
                               float* mask);
// view_resize.hip: composite at full size, antialiased bilinear downscale to [3,OH,OW], clamp; the mask (or NULL) by nearest
// neighbour.  C = 4: RGBA over the background; C = 3: RGB, with mask_bytes [H,W] or NULL.  Both byte arrays 16-byte aligned.
void launch_view_resize(hipStream_t s, int W, int H, int C, const uint8_t* pixels, const uint8_t* mask_bytes, const float* background,
                        int OW, int OH, float* image, float* mask);
// exr_unpack.hip: inflated OpenEXR chunks -> the planar view [kept,H,W] in the file's sample type (B bytes per sample); tile_sums
// holds chunks * 2 * exr_tiles_per_chunk(...) uint32 of scratch
size_t exr_tiles_per_chunk(int W, int C, int B, int max_rows);
void launch_exr_unpack_chunks(hipStream_t s, int W, int H, int C, int B, int chunks, int max_rows, const uint8_t* inflated,
                              long long inflated_bytes, const int32_t* table, int kept, const int32_t* kept_channels,
                              uint32_t* tile_sums, void* planes);
// ... and a resident planar HDR view [3,H,W] (half or float) + its mask bytes (or NULL) -> image [3,H,W] + mask [1,H,W] (or NULL)
void launch_view_unpack_hdr(hipStream_t s, int W, int H, int is_half, const void* view, const uint8_t* mask_bytes,
                            const float* background, float* image, float* mask);
// ssim.hip: the value-only SSIM tiling; tile_sums [C * ceil(W/32) * ceil(H/32)][2]
void launch_eval_metric_tiles(hipStream_t s, int W, int H, int C, const float* pred, const float* gt, const float* mask,
                              const float* fill, int fill_is_image, double* tile_sums);
// eval_metrics.hip
void launch_eval_image_metrics(hipStream_t s, int W, int H, int C, const float* pred, const float* gt, const float* mask,
                               const float* fill, int fill_is_image, double* tile_sums, double* row);
void launch_eval_median_ratio(hipStream_t s, int W, int H, const float* pred, const float* gt, const float* mask,
                              uint32_t* state, double* row);
size_t knn_temp_bytes(size_t P);
void knn_dist2(hipStream_t s, int P, const float* pts, float* dists, void* temp);
size_t bvh_build_temp_bytes(size_t P);                  // bvh_build.hip
void bvh_build(hipStream_t s, int P, int32_t* nodes, float* aabbs, uint64_t* morton, void* temp);
void bvh_prepare_leaves(hipStream_t s, int P, const float* means, const float* scales, const float* rotations, int32_t* nodes,
                        float* aabbs, float* covs_inv);
// bvh_trace.hip
void bvh_trace_count(hipStream_t s, int num_rays, const int32_t* nodes, const float* aabbs, const float* rays_o,
                     const float* rays_d, int32_t* counts, int* overflow);
void bvh_trace_fill(hipStream_t s, int num_rays, const int32_t* nodes, const float* aabbs, const float* rays_o,
                    const float* rays_d, const float* means, const int32_t* counts, const int64_t* offsets_inclusive,
                    uint64_t* keys, int32_t* points, float* positions, int32_t* ray_ids);
void bvh_trace_opacity(hipStream_t s, int num_rays, int P, const int32_t* nodes, const float* aabbs, const float* rays_o,
                       const float* rays_d, const float* means, const float* covs, const float* opac, const float* normals,
                       int32_t* contributes, float* out, int* overflow);
size_t bvh_trace_records_bytes(size_t P);
void bvh_pack_traversal(hipStream_t s, int P, const int32_t* nodes, const float* aabbs, const float* means,
                        const float* covs, const float* opac, const float* normals, void* records);
void bvh_trace_visits(hipStream_t s, int P, const void* records, unsigned long long out[2]);
void bvh_trace_opacity_packed(hipStream_t s, int num_rays, int P, void* records, const float* rays_o, const float* rays_d,
                              int32_t* contributes, float* out, int* overflow);
void bvh_trace_bundles(hipStream_t s, int P, int K, void* records, const int32_t* nodes, const float* zsamples, int leaf_lo,
                       int leaf_hi, float origin_offset, float* out, int32_t* contributes, float* dirs_out, int* overflow);
void bvh_trace_hemisphere(hipStream_t s, int P, int T, void* records, const int32_t* nodes, const float* raw_dirs, int leaf_lo,
                          int leaf_hi, float origin_offset, float* out, float* dirs_out, int32_t* contributes, int* overflow);
// visibility_bake.hip
int visibility_sh_fit_loss_rows(int P);
void visibility_sh_fit(hipStream_t s, int P, int T, long long steps_done, const float* dirs, const float* visibility, float lr,
                       float beta1, float beta2, float eps, float* coeffs, float* exp_avg, float* exp_avg_sq,
                       float* loss_partials);
void launch_transpose_selftest(hipStream_t s, int N, int dpp, const float* in, float* out, int* chan, int* owner);

}  // namespace r3dg
