// C ABI of the training-iteration glue (include/r3dg_hip.h): stage-1 / stage-2 activations, feature packing and losses,
// SSIM, Adam, relighting, evaluation, densification.  Thin wrappers: argument checks, stage timing, one launcher each.
#include "capi_internal.hpp"
#include <cstring>

using namespace r3dg;

extern "C" {

int r3dg_stage2_activate(void* stream_, int P, const float* xyz, const float* scaling_raw, const float* rotation_raw,
                         const float* opacity_raw, const float* normal_raw, const float* base_raw,
                         const float* rough_raw, const float* campos, float* scales, float* rot, float* opacity,
                         float* normal, float* base_color, float* roughness, float* viewdirs, const float* viewmatrix,
                         float* features)
{
    return r3dg_stage2_activate_with(stream_, P, xyz, scaling_raw, rotation_raw, opacity_raw, normal_raw, base_raw, rough_raw,
                                     campos, scales, rot, opacity, normal, base_color, roughness, viewdirs, viewmatrix, features,
                                     0, nullptr, nullptr, nullptr, 0);
}

int r3dg_stage2_activate_with(void* stream_, int P, const float* xyz, const float* scaling_raw, const float* rotation_raw,
                              const float* opacity_raw, const float* normal_raw, const float* base_raw,
                              const float* rough_raw, const float* campos, float* scales, float* rot, float* opacity,
                              float* normal, float* base_color, float* roughness, float* viewdirs, const float* viewmatrix,
                              float* features, int n_env, const float* env_raw, float* env, float* zero, int n_zero)
{
    if (P < 0) return invalid("stage2_activate: bad P");
    if (n_env < 0 || n_zero < 0) return invalid("stage2_activate: bad side-job size");
    if (n_env > 0 && (!env_raw || !env)) return invalid("stage2_activate: null texture buffer");
    if (n_zero > 0 && !zero) return invalid("stage2_activate: null buffer to zero");
    if (P == 0 && n_env == 0 && n_zero == 0) return R3DG_OK;
    if (P == 0) {                      // (only side jobs: run them behind zero Gaussian workgroups)
        return guarded([&]() -> int {
            launch_s2_activate((hipStream_t)stream_, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                               nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, n_env, env_raw,
                               env, zero, n_zero);
            return R3DG_OK;
        });
    }
    if (!xyz || !scaling_raw || !rotation_raw || !opacity_raw || !normal_raw || !scales || !rot || !opacity || !normal)
        return invalid("stage2_activate: null buffer");
    if (base_raw && (!rough_raw || !campos || !base_color || !roughness || !viewdirs))
        return invalid("stage2_activate: stage-2 inputs/outputs incomplete");
    if (features && (!base_raw || !viewmatrix)) return invalid("stage2_activate: feature rows need the stage-2 inputs and the view matrix");
    return guarded([&]() -> int {
        StageTimer t((hipStream_t)stream_, ST_S2_ACTIVATE);
        launch_s2_activate((hipStream_t)stream_, P, xyz, scaling_raw, rotation_raw, opacity_raw, normal_raw, base_raw,
                           rough_raw, campos, scales, rot, opacity, normal, base_color, roughness, viewdirs, viewmatrix, features,
                           n_env, env_raw, env, zero, n_zero);
        return R3DG_OK;
    });
}

int r3dg_stage2_pack_features(void* stream_, int P, const float* xyz, const float* viewmatrix, const float* normal,
                              const float* base_color, const float* roughness, const float* shade_out, float* features,
                              float* light_l1_sum)
{
    if (P < 0) return invalid("stage2_pack_features: bad P");
    if (P == 0) return R3DG_OK;
    if (!xyz || !viewmatrix || !normal || !base_color || !roughness || !shade_out || !features)
        return invalid("stage2_pack_features: null buffer");
    return guarded([&]() -> int {
        StageTimer t((hipStream_t)stream_, ST_S2_PACK);
        launch_s2_pack((hipStream_t)stream_, P, xyz, viewmatrix, normal, base_color, roughness, shade_out, features,
                       light_l1_sum);
        return R3DG_OK;
    });
}

// the host copy of a gradient record layout (R3DG_GRAD_RECORD_LAYOUT_INTS ints) for the kernels that read 16-float rows in place
static int record_layout_16(const char* name, const int* layout, GradRecordLayout* out)
{
    if (!layout) return invalid(std::string(name) + ": null record layout");
    std::memcpy(out, layout, sizeof(GradRecordLayout));
    if (!gradient_record_layout_valid(*out, 16) || out->nvp != 16)
        return invalid(std::string(name) + ": not a layout of 16-float gradient records over 16 feature columns");
    return R3DG_OK;
}

static int unpack_impl(void* stream_, int P, const float* dL_dfeatures, const float* records, const int* layout,
                       const float* shade_out, float light_weight, float* dL_dpbr, float* dL_ddiffuse, float* block_absmax,
                       float* light_l1_sum)
{
    if (P < 0) return invalid("stage2_unpack_gradients: bad P");
    if (P == 0) return R3DG_OK;
    if (!(dL_dfeatures || records) || !shade_out || !dL_dpbr || !dL_ddiffuse) return invalid("stage2_unpack_gradients: null buffer");
    GradRecordLayout L;
    if (records != nullptr)
        if (int e = record_layout_16("stage2_unpack_gradients_records", layout, &L)) return e;
    return guarded([&]() -> int {
        StageTimer t((hipStream_t)stream_, ST_S2_UNPACK);
        launch_s2_unpack((hipStream_t)stream_, P, dL_dfeatures, shade_out, light_weight, dL_dpbr, dL_ddiffuse, block_absmax,
                         light_l1_sum, records, records != nullptr ? &L : nullptr);
        return R3DG_OK;
    });
}

int r3dg_stage2_unpack_gradients(void* stream_, int P, const float* dL_dfeatures, const float* shade_out,
                                 float light_weight, float* dL_dpbr, float* dL_ddiffuse, float* block_absmax,
                                 float* light_l1_sum)
{
    if (P > 0 && !dL_dfeatures) return invalid("stage2_unpack_gradients: null buffer");
    return unpack_impl(stream_, P, dL_dfeatures, nullptr, nullptr, shade_out, light_weight, dL_dpbr, dL_ddiffuse, block_absmax,
                       light_l1_sum);
}

int r3dg_stage2_unpack_gradients_records(void* stream_, int P, const float* records, const int* layout, const float* shade_out,
                                         float light_weight, float* dL_dpbr, float* dL_ddiffuse, float* block_absmax,
                                         float* light_l1_sum)
{
    if (P > 0 && !records) return invalid("stage2_unpack_gradients_records: null buffer");
    return unpack_impl(stream_, P, nullptr, records, layout, shade_out, light_weight, dL_dpbr, dL_ddiffuse, block_absmax,
                       light_l1_sum);
}

int r3dg_stage2_activate_backward(void* stream_, int P, const float* xyz, const float* scaling_raw,
                                  const float* rotation_raw, const float* opacity_raw, const float* normal_raw,
                                  const float* base_raw, const float* rough_raw, const float* viewmatrix,
                                  const float* campos, const float* dL_dfeatures, const float* dL_dbase_shade,
                                  const float* dL_drough_shade, const float* dL_dviewdirs, const float* dL_dscales,
                                  const float* dL_drot, const float* dL_dopacity, const float* dL_dmeans3D, float* g_xyz,
                                  float* g_scaling, float* g_rotation, float* g_opacity, float* g_normal, float* g_base,
                                  float* g_rough)
{
    return r3dg_stage2_activate_backward_with(stream_, P, xyz, scaling_raw, rotation_raw, opacity_raw, normal_raw, base_raw,
                                              rough_raw, viewmatrix, campos, dL_dfeatures, dL_dbase_shade, dL_drough_shade,
                                              dL_dviewdirs, dL_dscales, dL_drot, dL_dopacity, dL_dmeans3D, g_xyz, g_scaling,
                                              g_rotation, g_opacity, g_normal, g_base, g_rough, 0, 0, nullptr, nullptr, nullptr,
                                              0.f, nullptr, nullptr, 0);
}

static int activate_backward_impl(void* stream_, int P, const float* xyz, const float* scaling_raw,
                                  const float* rotation_raw, const float* opacity_raw, const float* normal_raw,
                                  const float* base_raw, const float* rough_raw, const float* viewmatrix,
                                  const float* campos, const float* dL_dfeatures, const float* dL_dbase_shade,
                                  const float* dL_drough_shade, const float* dL_dviewdirs, const float* dL_dscales,
                                  const float* dL_drot, const float* dL_dopacity, const float* dL_dmeans3D, float* g_xyz,
                                  float* g_scaling, float* g_rotation, float* g_opacity, float* g_normal, float* g_base,
                                  float* g_rough, int He, int We,
                                       const float* env_raw, const float* env, float* dL_denv, float w_tv,
                                       float* g_env_raw, float* tv_sum, int consume, float* records, const int* layout)
{
    if (P < 0) return invalid("stage2_activate_backward: bad P");
    if (He < 0 || We < 0) return invalid("stage2_activate_backward: bad texture size");
    const bool env_job = He * We != 0;
    if (env_job && (!env_raw || !env || !dL_denv || !g_env_raw)) return invalid("stage2_activate_backward: null texture buffer");
    if (P == 0) return env_job ? r3dg_stage2_env_backward(stream_, He, We, env_raw, env, dL_denv, w_tv, g_env_raw, tv_sum, consume) : R3DG_OK;
    if (!base_raw || !rough_raw || !(dL_dfeatures || records) || !dL_dbase_shade || !dL_drough_shade || !g_base || !g_rough)
        return invalid("stage2_activate_backward: null buffer");
    GradRecordLayout L;
    if (records != nullptr) {
        if (int e = record_layout_16("stage2_activate_backward_with_records", layout, &L)) return e;
        if (g_xyz == nullptr) return invalid("stage2_activate_backward_with_records: frozen geometry reads no gradient records");
    }
    // g_xyz == NULL: frozen geometry -- only g_base / g_rough are produced and the geometry inputs are not read
    if (g_xyz != nullptr &&
        (!xyz || !scaling_raw || !rotation_raw || !opacity_raw || !normal_raw || !viewmatrix || !campos || !dL_dviewdirs ||
         !dL_dscales || !dL_drot || !(dL_dopacity || records) || !dL_dmeans3D || !g_scaling || !g_rotation || !g_opacity || !g_normal))
        return invalid("stage2_activate_backward: null buffer");
    return guarded([&]() -> int {
        StageTimer t((hipStream_t)stream_, ST_S2_ACTIVATE_BWD);
        launch_s2_activate_backward((hipStream_t)stream_, P, xyz, scaling_raw, rotation_raw, opacity_raw, normal_raw,
                                    base_raw, rough_raw, viewmatrix, campos, dL_dfeatures, dL_dbase_shade,
                                    dL_drough_shade, dL_dviewdirs, dL_dscales, dL_drot, dL_dopacity, dL_dmeans3D, g_xyz,
                                    g_scaling, g_rotation, g_opacity, g_normal, g_base, g_rough, env_job ? He : 0, env_job ? We : 0,
                                    env_job ? env_raw : nullptr, env, dL_denv, w_tv, g_env_raw, tv_sum, consume, records,
                                    records != nullptr ? &L : nullptr);
        return R3DG_OK;
    });
}

int r3dg_stage2_activate_backward_with(void* stream_, int P, const float* xyz, const float* scaling_raw,
                                  const float* rotation_raw, const float* opacity_raw, const float* normal_raw,
                                  const float* base_raw, const float* rough_raw, const float* viewmatrix,
                                  const float* campos, const float* dL_dfeatures, const float* dL_dbase_shade,
                                  const float* dL_drough_shade, const float* dL_dviewdirs, const float* dL_dscales,
                                  const float* dL_drot, const float* dL_dopacity, const float* dL_dmeans3D, float* g_xyz,
                                  float* g_scaling, float* g_rotation, float* g_opacity, float* g_normal, float* g_base,
                                  float* g_rough, int He, int We,
                                       const float* env_raw, const float* env, float* dL_denv, float w_tv,
                                       float* g_env_raw, float* tv_sum, int consume)
{
    if (P > 0 && (!dL_dfeatures || (g_xyz != nullptr && !dL_dopacity))) return invalid("stage2_activate_backward: null buffer");
    return activate_backward_impl(stream_, P, xyz, scaling_raw, rotation_raw, opacity_raw, normal_raw, base_raw, rough_raw,
                                  viewmatrix, campos, dL_dfeatures, dL_dbase_shade, dL_drough_shade, dL_dviewdirs, dL_dscales,
                                  dL_drot, dL_dopacity, dL_dmeans3D, g_xyz, g_scaling, g_rotation, g_opacity, g_normal, g_base,
                                  g_rough, He, We, env_raw, env, dL_denv, w_tv, g_env_raw, tv_sum, consume, nullptr, nullptr);
}

int r3dg_stage2_activate_backward_with_records(void* stream_, int P, const float* xyz, const float* scaling_raw,
                                  const float* rotation_raw, const float* opacity_raw, const float* normal_raw,
                                  const float* base_raw, const float* rough_raw, const float* viewmatrix,
                                  const float* campos, float* records, const int* layout, const float* dL_dbase_shade,
                                  const float* dL_drough_shade, const float* dL_dviewdirs, const float* dL_dscales,
                                  const float* dL_drot, const float* dL_dmeans3D, float* g_xyz,
                                  float* g_scaling, float* g_rotation, float* g_opacity, float* g_normal, float* g_base,
                                  float* g_rough, int He, int We,
                                       const float* env_raw, const float* env, float* dL_denv, float w_tv,
                                       float* g_env_raw, float* tv_sum, int consume)
{
    if (P > 0 && !records) return invalid("stage2_activate_backward_with_records: null buffer");
    return activate_backward_impl(stream_, P, xyz, scaling_raw, rotation_raw, opacity_raw, normal_raw, base_raw, rough_raw,
                                  viewmatrix, campos, nullptr, dL_dbase_shade, dL_drough_shade, dL_dviewdirs, dL_dscales,
                                  dL_drot, nullptr, dL_dmeans3D, g_xyz, g_scaling, g_rotation, g_opacity, g_normal, g_base,
                                  g_rough, He, We, env_raw, env, dL_denv, w_tv, g_env_raw, tv_sum, consume, records, layout);
}

int r3dg_stage2_loss(void* stream_, int width, int height, const float* image, const float* opacity,
                     const float* feature, const float* pseudo_normal, const int32_t* n_contrib, const float* gt,
                     const float* bg, const float* image_mask, float w_l1, float w_pbr, float w_normal,
                     const float* extra_dimage, const float* extra_dsrgb, float* dL_dimage, float* dL_dopacity,
                     float* dL_dfeature, float* sums, int sparse_feature_gradients)
{
    if (width < 0 || height < 0) return invalid("stage2_loss: bad image size");
    if ((long long)width * height == 0) return R3DG_OK;
    if (!image || !opacity || !feature || !pseudo_normal || !n_contrib || !gt || !bg || !dL_dimage || !dL_dopacity ||
        !dL_dfeature || !sums)
        return invalid("stage2_loss: null buffer");
    return guarded([&]() -> int {
        StageTimer t((hipStream_t)stream_, ST_S2_LOSS);
        launch_s2_loss((hipStream_t)stream_, width * height, image, opacity, feature, pseudo_normal, n_contrib, gt, bg,
                       image_mask, w_l1, w_pbr, w_normal, extra_dimage, extra_dsrgb, dL_dimage, dL_dopacity, dL_dfeature, sums,
                       sparse_feature_gradients);
        return R3DG_OK;
    });
}

int r3dg_stage2_smooth_forward(void* stream_, int width, int height, const float* opacity, const float* feature,
                               const int32_t* n_contrib, const float* gt, const float* image_mask, float w_base_color,
                               float w_roughness, float w_light, float* scratch, float* sums3)
{
    if (width < 0 || height < 0) return invalid("stage2_smooth_forward: bad image size");
    if ((long long)width * height == 0) return R3DG_OK;
    if (!opacity || !feature || !n_contrib || !gt || !scratch || !sums3) return invalid("stage2_smooth_forward: null buffer");
    return guarded([&]() -> int {
        StageTimer t((hipStream_t)stream_, ST_S2_LOSS);
        launch_s2_smooth_forward((hipStream_t)stream_, width, height, opacity, feature, n_contrib, gt, image_mask,
                                 w_base_color, w_roughness, w_light, scratch, sums3);
        return R3DG_OK;
    });
}

int r3dg_stage2_smooth_backward(void* stream_, int width, int height, const float* opacity, const float* feature,
                                const int32_t* n_contrib, const float* image_mask, const float* scratch, float w_base_color,
                                float w_roughness, float w_light, int accumulate_normal, float* dL_dopacity,
                                float* dL_dfeature)
{
    if (width < 0 || height < 0) return invalid("stage2_smooth_backward: bad image size");
    if ((long long)width * height == 0) return R3DG_OK;
    if (!opacity || !feature || !n_contrib || !scratch || !dL_dopacity || !dL_dfeature)
        return invalid("stage2_smooth_backward: null buffer");
    return guarded([&]() -> int {
        StageTimer t((hipStream_t)stream_, ST_S2_LOSS);
        launch_s2_smooth_backward((hipStream_t)stream_, width, height, opacity, feature, n_contrib, image_mask, scratch,
                                  w_base_color != 0.f, w_roughness != 0.f, w_light != 0.f, accumulate_normal, dL_dopacity,
                                  dL_dfeature);
        return R3DG_OK;
    });
}

int r3dg_stage2_smooth_fused(void* stream_, int width, int height, const float* opacity, const float* feature,
                             const int32_t* n_contrib, const float* gt, const float* image_mask, float w_base_color,
                             float w_roughness, float w_light, int accumulate_normal, float* dL_dopacity, float* dL_dfeature,
                             float* sums3)
{
    if (width < 0 || height < 0) return invalid("stage2_smooth_fused: bad image size");
    if ((long long)width * height == 0) return R3DG_OK;
    if (!opacity || !feature || !n_contrib || !gt || !dL_dopacity || !dL_dfeature || !sums3)
        return invalid("stage2_smooth_fused: null buffer");
    return guarded([&]() -> int {
        StageTimer t((hipStream_t)stream_, ST_S2_LOSS);
        launch_s2_smooth_fused((hipStream_t)stream_, width, height, opacity, feature, n_contrib, gt, image_mask, w_base_color,
                               w_roughness, w_light, accumulate_normal, dL_dopacity, dL_dfeature, sums3);
        return R3DG_OK;
    });
}

int r3dg_stage1_pack_features(void* stream_, int P, const float* xyz, const float* viewmatrix, const float* normal,
                              float* features)
{
    if (P < 0) return invalid("stage1_pack_features: bad P");
    if (P == 0) return R3DG_OK;
    if (!xyz || !viewmatrix || !normal || !features) return invalid("stage1_pack_features: null buffer");
    return guarded([&]() -> int {
        StageTimer t((hipStream_t)stream_, ST_S2_PACK);
        launch_s1_pack((hipStream_t)stream_, P, xyz, viewmatrix, normal, features);
        return R3DG_OK;
    });
}

int r3dg_stage1_loss(void* stream_, int width, int height, const float* image, const float* opacity,
                     const float* feature, const float* pseudo_normal, const int32_t* n_contrib, const float* gt,
                     const float* image_mask, float w_l1, float w_mask_entropy, float w_normal, float w_normal_smooth,
                     float w_depth_var, const float* extra_dimage, float* edge_scratch, float* dL_dimage,
                     float* dL_dopacity, float* dL_dfeature, float* sums)
{
    if (width < 0 || height < 0) return invalid("stage1_loss: bad image size");
    if ((long long)width * height == 0) return R3DG_OK;
    if (!image || !opacity || !feature || !pseudo_normal || !n_contrib || !gt || !dL_dimage || !dL_dopacity ||
        !dL_dfeature || !sums)
        return invalid("stage1_loss: null buffer");
    if (w_normal_smooth != 0.f && !edge_scratch) return invalid("stage1_loss: the normal-smoothness term needs edge_scratch");
    return guarded([&]() -> int {
        StageTimer t((hipStream_t)stream_, ST_S2_LOSS);
        if (w_normal_smooth != 0.f)
            launch_s1_edge((hipStream_t)stream_, width, height, feature, opacity, n_contrib, gt, edge_scratch, sums + 4 * R3DG_SUM_SLOTS);
        launch_s1_loss((hipStream_t)stream_, width, height, image, opacity, feature, pseudo_normal, n_contrib, gt, image_mask,
                       w_l1, w_mask_entropy, w_normal, w_normal_smooth, w_depth_var, extra_dimage,
                       w_normal_smooth != 0.f ? edge_scratch : nullptr, dL_dimage, dL_dopacity, dL_dfeature, sums);
        return R3DG_OK;
    });
}

int r3dg_stage1_activate_backward(void* stream_, int P, const float* xyz, const float* scaling_raw,
                                  const float* rotation_raw, const float* opacity_raw, const float* normal_raw,
                                  const float* viewmatrix, const float* dL_dfeatures, const float* dL_dscales,
                                  const float* dL_drot, const float* dL_dopacity, const float* dL_dmeans3D, float* g_xyz,
                                  float* g_scaling, float* g_rotation, float* g_opacity, float* g_normal)
{
    if (P < 0) return invalid("stage1_activate_backward: bad P");
    if (P == 0) return R3DG_OK;
    if (!xyz || !scaling_raw || !rotation_raw || !opacity_raw || !normal_raw || !viewmatrix || !dL_dfeatures ||
        !dL_dscales || !dL_drot || !dL_dopacity || !dL_dmeans3D || !g_xyz || !g_scaling || !g_rotation || !g_opacity ||
        !g_normal)
        return invalid("stage1_activate_backward: null buffer");
    return guarded([&]() -> int {
        StageTimer t((hipStream_t)stream_, ST_S2_ACTIVATE_BWD);
        launch_s1_activate_backward((hipStream_t)stream_, P, xyz, scaling_raw, rotation_raw, opacity_raw, normal_raw,
                                    viewmatrix, dL_dfeatures, dL_dscales, dL_drot, dL_dopacity, dL_dmeans3D, g_xyz,
                                    g_scaling, g_rotation, g_opacity, g_normal);
        return R3DG_OK;
    });
}

int r3dg_stage2_pbr_srgb(void* stream_, int width, int height, const float* opacity, const float* feature,
                         const int32_t* n_contrib, const float* bg, float* srgb)
{
    if (width < 0 || height < 0) return invalid("stage2_pbr_srgb: bad image size");
    if ((long long)width * height == 0) return R3DG_OK;
    if (!opacity || !feature || !n_contrib || !bg || !srgb) return invalid("stage2_pbr_srgb: null buffer");
    return guarded([&]() -> int {
        launch_s2_pbr_srgb((hipStream_t)stream_, width * height, opacity, feature, n_contrib, bg, srgb);
        return R3DG_OK;
    });
}

int r3dg_stage2_normals_srgb(void* stream_, int width, int height, const float* viewmatrix, float tan_fovx, float tan_fovy,
                             float cx, float cy, const float* opacity, const float* depth, float* pseudo_normal,
                             float* surface_xyz, const float* feature, const int32_t* n_contrib, const float* bg, float* srgb)
{
    if (width < 0 || height < 0) return invalid("stage2_normals_srgb: bad image size");
    if ((long long)width * height == 0) return R3DG_OK;
    if ((long long)width * height > 0x7fffffffLL) return invalid("stage2_normals_srgb: image too large");
    if (!viewmatrix || !opacity || !depth || !pseudo_normal || !surface_xyz || !feature || !n_contrib || !bg || !srgb)
        return invalid("stage2_normals_srgb: null buffer");
    return guarded([&]() -> int {
        StageTimer t((hipStream_t)stream_, ST_NORMAL);
        // focal lengths exactly as the rasterizer forward derives them (rasterizer_impl.cu:239-240)
        const float focal_y = height / (2.0f * tan_fovy), focal_x = width / (2.0f * tan_fovx);
        launch_s2_normals_srgb((hipStream_t)stream_, width, height, viewmatrix, focal_x, focal_y, cx, cy, opacity, depth,
                               pseudo_normal, surface_xyz, feature, n_contrib, bg, srgb);
        return R3DG_OK;
    });
}

int r3dg_stage2_image_tail_supported(int width, int height) { return image_tail_applies(width, height) ? 1 : 0; }

int r3dg_stage2_image_tail(void* stream_, int width, int height, const float* viewmatrix, float tan_fovx, float tan_fovy, float cx,
                           float cy, const float* image, const float* opacity, const float* depth, const float* feature,
                           const int32_t* n_contrib, const float* gt, const float* bg, const float* image_mask, float w_l1,
                           float w_pbr, float w_normal, float scale_image, float scale_pbr, float* pseudo_normal,
                           float* surface_xyz, float* dL_dimage, float* dL_dopacity, float* dL_dfeature, float* sums,
                           float* ssim_sum_image, float* ssim_sum_pbr)
{
    if (width < 0 || height < 0) return invalid("stage2_image_tail: bad image size");
    if ((long long)width * height == 0) return R3DG_OK;
    if (!image_tail_applies(width, height)) return invalid("stage2_image_tail: image too large");
    if (!viewmatrix || !image || !opacity || !depth || !feature || !n_contrib || !gt || !bg || !pseudo_normal || !surface_xyz ||
        !dL_dimage || !dL_dopacity || !dL_dfeature || !sums || !ssim_sum_image || !ssim_sum_pbr)
        return invalid("stage2_image_tail: null buffer");
    return guarded([&]() -> int {
        StageTimer t((hipStream_t)stream_, ST_S2_LOSS);
        // focal lengths exactly as the rasterizer forward derives them (rasterizer_impl.cu:239-240)
        const float focal_y = height / (2.0f * tan_fovy), focal_x = width / (2.0f * tan_fovx);
        launch_s2_image_tail((hipStream_t)stream_, width, height, viewmatrix, focal_x, focal_y, cx, cy, image, opacity, depth,
                             feature, n_contrib, gt, bg, image_mask, w_l1, w_pbr, w_normal, scale_image, scale_pbr, pseudo_normal,
                             surface_xyz, dL_dimage, dL_dopacity, dL_dfeature, sums, ssim_sum_image, ssim_sum_pbr);
        return R3DG_OK;
    });
}

int r3dg_ssim_forward_pair(void* stream_, int width, int height, int channels, const float* x0, const float* x1,
                           const float* y, float* partials0, float* partials1, float* sum0, float* sum1)
{
    if (width < 0 || height < 0 || channels < 0) return invalid("ssim_forward: bad shape");
    if ((long long)width * height * channels == 0) return R3DG_OK;
    if (!x0 || !y || !partials0 || (x1 && !partials1)) return invalid("ssim_forward: null buffer");
    if ((long long)channels * 2 > 65535) return invalid("ssim_forward: too many channels");
    return guarded([&]() -> int {
        StageTimer t((hipStream_t)stream_, ST_SSIM);
        const float* x[2] = {x0, x1};
        float* partials[2] = {partials0, partials1};
        float* sum[2] = {sum0, sum1};
        launch_ssim_forward((hipStream_t)stream_, width, height, channels, x1 ? 2 : 1, x, y, partials, sum);
        return R3DG_OK;
    });
}

int r3dg_ssim_backward_pair(void* stream_, int width, int height, int channels, const float* x0, const float* x1,
                            const float* y, const float* partials0, const float* partials1, float scale0, float scale1,
                            float* grad_x0, float* grad_x1)
{
    if (width < 0 || height < 0 || channels < 0) return invalid("ssim_backward: bad shape");
    if ((long long)width * height * channels == 0) return R3DG_OK;
    if (!x0 || !y || !partials0 || !grad_x0 || (x1 && (!partials1 || !grad_x1))) return invalid("ssim_backward: null buffer");
    if ((long long)channels * 2 > 65535) return invalid("ssim_backward: too many channels");
    return guarded([&]() -> int {
        StageTimer t((hipStream_t)stream_, ST_SSIM);
        const float* x[2] = {x0, x1};
        float* partials[2] = {const_cast<float*>(partials0), const_cast<float*>(partials1)};
        const float scale[2] = {scale0, scale1};
        float* grad[2] = {grad_x0, grad_x1};
        launch_ssim_backward((hipStream_t)stream_, width, height, channels, x1 ? 2 : 1, x, y, partials, scale, grad);
        return R3DG_OK;
    });
}

int r3dg_ssim_forward(void* stream_, int width, int height, int channels, const float* x, const float* y,
                      float* partials, float* sum)
{
    return r3dg_ssim_forward_pair(stream_, width, height, channels, x, nullptr, y, partials, nullptr, sum, nullptr);
}

int r3dg_ssim_backward(void* stream_, int width, int height, int channels, const float* x, const float* y,
                       const float* partials, float scale, float* grad_x)
{
    return r3dg_ssim_backward_pair(stream_, width, height, channels, x, nullptr, y, partials, nullptr, scale, 0.f, grad_x,
                                   nullptr);
}

int r3dg_stage2_env_backward(void* stream_, int He, int We, const float* raw, const float* env, float* dL_denv,
                             float w_tv, float* g_raw, float* tv_sum, int consume)
{
    if (He < 0 || We < 0) return invalid("stage2_env_backward: bad texture size");
    if (He * We == 0) return R3DG_OK;
    if (!raw || !env || !dL_denv || !g_raw) return invalid("stage2_env_backward: null buffer");
    return guarded([&]() -> int {
        launch_s2_env_backward((hipStream_t)stream_, He, We, raw, env, dL_denv, w_tv, g_raw, tv_sum, consume);
        return R3DG_OK;
    });
}

int r3dg_adam_step(void* stream_, int n_groups, const r3dg_adam_group* groups, float beta1, float beta2, float eps,
                   int step, float grad_scale, const float* skip_flag)
{
    if (n_groups < 0 || n_groups > R3DG_ADAM_MAX_GROUPS) return invalid("adam_step: bad group count");
    if (step < 1) return invalid("adam_step: step counts from 1");
    if (n_groups == 0) return R3DG_OK;
    if (!groups) return invalid("adam_step: null group table");
    for (int i = 0; i < n_groups; i++) {
        if (groups[i].n >= (1ull << 32)) return invalid("adam_step: group larger than 2^32 elements");
        if (groups[i].n && (!groups[i].param || !groups[i].grad || !groups[i].exp_avg || !groups[i].exp_avg_sq))
            return invalid("adam_step: null buffer in group");
    }
    return guarded([&]() -> int {
        StageTimer t((hipStream_t)stream_, ST_ADAM);
        launch_adam((hipStream_t)stream_, n_groups, groups, beta1, beta2, eps, step, grad_scale, skip_flag);
        return R3DG_OK;
    });
}

int r3dg_relight_pack_features(void* stream_, int P, const float* xyz, const float* viewmatrix, const float* normal,
                               const float* base_color, const float* roughness, const float* shade_out, float* features)
{
    if (P < 0) return invalid("relight_pack_features: bad P");
    if (P == 0) return R3DG_OK;
    if (!xyz || !viewmatrix || !normal || !base_color || !roughness || !shade_out || !features)
        return invalid("relight_pack_features: null buffer");
    if ((size_t)features & 15) return invalid("relight_pack_features: features must be 16-byte aligned");
    return guarded([&]() -> int {
        StageTimer t((hipStream_t)stream_, ST_RELIGHT_PACK);
        launch_relight_pack((hipStream_t)stream_, P, xyz, viewmatrix, normal, base_color, roughness, shade_out, features);
        return R3DG_OK;
    });
}

int r3dg_relight_compose(void* stream_, int width, int height, float focal_x, float focal_y, float cx, float cy,
                         const float* viewmatrix, const float* light_transform, const float* envmap, int He, int We,
                         const float* image, const float* opacity, const float* feature, const int32_t* n_contrib,
                         float* pbr_env, float* render_env, float* env_only)
{
    if (width < 0 || height < 0 || He < 1 || We < 1) return invalid("relight_compose: bad shape");
    if ((long long)width * height == 0) return R3DG_OK;
    if ((long long)width * height >= (1ll << 31)) return invalid("relight_compose: image too large");
    if (!viewmatrix || !envmap || !opacity || !feature || !n_contrib) return invalid("relight_compose: null buffer");
    if (render_env && !image) return invalid("relight_compose: render_env needs the rendered image");
    if (!(focal_x > 0.f) || !(focal_y > 0.f)) return invalid("relight_compose: focal lengths must be positive");
    return guarded([&]() -> int {
        StageTimer t((hipStream_t)stream_, ST_RELIGHT_COMPOSE);
        launch_relight_compose((hipStream_t)stream_, width, height, focal_x, focal_y, cx, cy, viewmatrix, light_transform,
                               envmap, He, We, image, opacity, feature, n_contrib, pbr_env, render_env, env_only);
        return R3DG_OK;
    });
}

// The three evaluation entry points run between iterations, not inside one: they are left out of the per-stage timing, whose
// stages describe a training iteration or a relight frame.
int r3dg_relight_capture(void* stream_, int width, int height, const float* feature, const float* opacity,
                         const int32_t* n_contrib, const float* background, const float* mask, float* pbr,
                         float* base_color, float* roughness, float* normal, float* visibility, float* diffuse,
                         float* specular, float* lights, float* local_lights, float* global_lights, float* depth_var)
{
    if (width < 0 || height < 0) return invalid("relight_capture: bad shape");
    if ((long long)width * height == 0) return R3DG_OK;
    if ((long long)width * height >= (1ll << 31)) return invalid("relight_capture: image too large");
    if (!feature || !opacity || !n_contrib) return invalid("relight_capture: null buffer");
    if ((pbr || mask) && !background) return invalid("relight_capture: the pbr map and the mask need a background");
    const CaptureMaps maps = {pbr, base_color, roughness, normal, visibility, diffuse, specular, lights, local_lights,
                              global_lights, depth_var};
    return guarded([&]() -> int {
        launch_relight_capture((hipStream_t)stream_, width, height, feature, opacity, n_contrib, background, mask, maps);
        return R3DG_OK;
    });
}

int r3dg_eval_image_metrics(void* stream_, int width, int height, int channels, const float* pred, const float* gt,
                            const float* mask, const float* fill, int fill_is_image, double* tile_sums, double* row)
{
    if (width < 1 || height < 1 || channels < 1 || channels > 3) return invalid("eval_image_metrics: bad shape");
    if ((long long)width * height >= (1ll << 31)) return invalid("eval_image_metrics: image too large");
    if (!pred || !gt || !tile_sums || !row) return invalid("eval_image_metrics: null buffer");
    if (fill && !mask) return invalid("eval_image_metrics: a fill needs a mask");
    return guarded([&]() -> int {
        launch_eval_image_metrics((hipStream_t)stream_, width, height, channels, pred, gt, mask, fill, fill_is_image, tile_sums,
                                  row);
        return R3DG_OK;
    });
}

int r3dg_eval_median_ratio(void* stream_, int width, int height, const float* pred, const float* gt, const float* mask,
                           uint32_t* state, double* row)
{
    if (width < 0 || height < 0) return invalid("eval_median_ratio: bad shape");
    if ((long long)width * height >= (1ll << 31)) return invalid("eval_median_ratio: image too large");
    if (!state || !row) return invalid("eval_median_ratio: null buffer");
    if ((long long)width * height != 0 && (!pred || !gt)) return invalid("eval_median_ratio: null image");
    return guarded([&]() -> int {
        launch_eval_median_ratio((hipStream_t)stream_, width, height, pred, gt, mask, state, row);
        return R3DG_OK;
    });
}

int r3dg_densify_accumulate(void* stream_, int P, const float* viewspace_grad, const float* normal_grad,
                            const int32_t* radii, const float* weights, float* xyz_accum, float* normal_accum,
                            float* denom, float* weights_accum, float* max_radii2D, const float* skip_flag)
{
    if (P < 0) return invalid("densify_accumulate: bad P");
    if (P == 0) return R3DG_OK;
    if (!viewspace_grad || !radii || !weights || !xyz_accum || !normal_accum || !denom || !weights_accum || !max_radii2D)
        return invalid("densify_accumulate: null buffer");
    return guarded([&]() -> int {
        StageTimer t((hipStream_t)stream_, ST_DENSIFY);
        launch_densify_accumulate((hipStream_t)stream_, P, viewspace_grad, normal_grad, radii, weights, xyz_accum,
                                  normal_accum, denom, weights_accum, max_radii2D, skip_flag);
        return R3DG_OK;
    });
}

size_t r3dg_densify_temp_bytes(int P) { return densify_temp_bytes((size_t)(P > 0 ? P : 0)); }

int r3dg_densify_plan(void* stream_, int P, const r3dg_densify_config* cfg, const float* scaling_raw,
                      const float* opacity_raw, const float* xyz_accum, const float* normal_accum, const float* denom,
                      const float* weights_accum, const float* max_radii2D, int32_t* src_row, int32_t* kind,
                      int32_t* counts, void* temp)
{
    if (P < 0) return invalid("densify_plan: bad P");
    if (!cfg || !counts) return invalid("densify_plan: null config / counts");
    if (cfg->mode != 0 && cfg->mode != 1) return invalid("densify_plan: mode is 0 (densify_and_prune) or 1 (prune)");
    if (cfg->n_split < 1 || cfg->n_split > 8) return invalid("densify_plan: n_split out of range");
    if (cfg->mode == 0 && !(cfg->split_divisor > 0.f)) return invalid("densify_plan: split_divisor must be positive");
    if ((int64_t)P * (cfg->n_split > 2 ? cfg->n_split : 2) >= (1ll << 31)) return invalid("densify_plan: row map too large");
    if (P > 0 && (!scaling_raw || !opacity_raw || !xyz_accum || !normal_accum || !denom || !weights_accum ||
                  !max_radii2D || !src_row || !kind || !temp))
        return invalid("densify_plan: null buffer");
    return guarded([&]() -> int {
        hipStream_t s = (hipStream_t)stream_;
        if (P == 0) {
            R3DG_HIP(hipMemsetAsync(counts, 0, 8 * sizeof(int32_t), s));
            return R3DG_OK;
        }
        StageTimer t(s, ST_DENSIFY);
        launch_densify_plan(s, P, *cfg, scaling_raw, opacity_raw, xyz_accum, normal_accum, denom, weights_accum,
                            max_radii2D, src_row, kind, counts, temp);
        return R3DG_OK;
    });
}

int r3dg_densify_gather(void* stream_, int rows_out, const int32_t* src_row, const int32_t* kind, int n_groups,
                        const r3dg_densify_group* groups, const float* xyz, const float* scaling_raw,
                        const float* rotation_raw, const float* normal_table, float split_divisor)
{
    if (rows_out < 0) return invalid("densify_gather: bad row count");
    if (n_groups < 0 || n_groups > R3DG_DENSIFY_MAX_GROUPS) return invalid("densify_gather: bad group count");
    if (rows_out == 0 || n_groups == 0) return R3DG_OK;
    if (!groups || !src_row || !kind) return invalid("densify_gather: null table / row map");
    for (int i = 0; i < n_groups; i++) {
        const r3dg_densify_group& g = groups[i];
        if (g.row_floats == 0 || !g.src_param || !g.dst_param) return invalid("densify_gather: empty group");
        if ((g.src_exp_avg != nullptr) != (g.src_exp_avg_sq != nullptr) ||
            (g.src_exp_avg && (!g.dst_exp_avg || !g.dst_exp_avg_sq)))
            return invalid("densify_gather: moments must be given as complete source/destination pairs");
        if (g.role == R3DG_DENSIFY_ROLE_XYZ && g.row_floats != 3) return invalid("densify_gather: xyz rows are 3 floats");
        if (g.role == R3DG_DENSIFY_ROLE_SCALING && g.row_floats != 3)
            return invalid("densify_gather: scaling rows are 3 floats");
        if (g.role > R3DG_DENSIFY_ROLE_SCALING) return invalid("densify_gather: unknown role");
        if (g.role != R3DG_DENSIFY_ROLE_COPY && (!xyz || !scaling_raw || !rotation_raw || !(split_divisor > 0.f)))
            return invalid("densify_gather: split sources missing");
        if ((uint64_t)rows_out * g.row_floats >= (1ull << 41)) return invalid("densify_gather: group too large");
    }
    return guarded([&]() -> int {
        StageTimer t((hipStream_t)stream_, ST_DENSIFY);
        launch_densify_gather((hipStream_t)stream_, rows_out, src_row, kind, n_groups, groups, xyz, scaling_raw,
                              rotation_raw, normal_table, split_divisor);
        return R3DG_OK;
    });
}

int r3dg_reset_opacity(void* stream_, int P, float* opacity_raw, float* exp_avg, float* exp_avg_sq)
{
    if (P < 0) return invalid("reset_opacity: bad P");
    if (P == 0) return R3DG_OK;
    if (!opacity_raw) return invalid("reset_opacity: null buffer");
    return guarded([&]() -> int {
        launch_reset_opacity((hipStream_t)stream_, P, 0.01f, opacity_raw, exp_avg, exp_avg_sq);
        return R3DG_OK;
    });
}

}  // extern "C"
