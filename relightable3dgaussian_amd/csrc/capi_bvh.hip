// C ABI of the BVH build / visibility trace, of the visibility SH fit over its rays and of the nearest-neighbour distances
// (include/r3dg_hip.h).
#include "capi_internal.hpp"

using namespace r3dg;

extern "C" {

size_t r3dg_knn_temp_bytes(int P) { return knn_temp_bytes((size_t)(P > 0 ? P : 0)); }

int r3dg_knn_dist2(void* stream_, int P, const float* points, float* mean_dist2, void* temp)
{
    if (P < 0) return invalid("knn_dist2: bad P");
    if (P == 0) return R3DG_OK;
    if (!points || !mean_dist2 || !temp) return invalid("knn_dist2: null buffer");
    return guarded([&]() -> int {
        StageTimer t((hipStream_t)stream_, ST_KNN);
        knn_dist2((hipStream_t)stream_, P, points, mean_dist2, temp);
        return R3DG_OK;
    });
}

size_t r3dg_bvh_build_temp_bytes(int P) { return bvh_build_temp_bytes((size_t)(P > 0 ? P : 0)); }

int r3dg_bvh_build(void* stream_, int P, int32_t* nodes, float* aabbs, int64_t* morton, void* temp)
{
    if (P < 0) return invalid("bvh_build: bad P");
    if (P == 0) return R3DG_OK;
    if (!nodes || !aabbs || !morton || !temp) return invalid("bvh_build: null buffer");
    return guarded([&]() -> int {
        hipStream_t stream = (hipStream_t)stream_;
        StageTimer t(stream, ST_BVH_BUILD);
        bvh_build(stream, P, nodes, aabbs, (uint64_t*)morton, temp);
        t.stop();
        return R3DG_OK;
    });
}

int r3dg_bvh_prepare_leaves(void* stream_, int P, const float* means3D, const float* scales, const float* rotations,
                            int32_t* nodes, float* aabbs, float* covs3D_inv)
{
    if (P < 0) return invalid("bvh_prepare_leaves: bad P");
    if (P == 0) return R3DG_OK;
    if (!means3D || !scales || !rotations || !nodes || !aabbs || !covs3D_inv) return invalid("bvh_prepare_leaves: null buffer");
    return guarded([&]() -> int {
        hipStream_t stream = (hipStream_t)stream_;
        StageTimer t(stream, ST_BVH_BUILD);
        bvh_prepare_leaves(stream, P, means3D, scales, rotations, nodes, aabbs, covs3D_inv);
        check_launch(stream, false, "bvh_prepare_leaves");
        t.stop();
        return R3DG_OK;
    });
}

int r3dg_bvh_trace_opacity(void* stream_, int64_t num_rays, int num_gaussians, const int32_t* nodes, const float* aabbs,
                           const float* rays_o, const float* rays_d, const float* means3D, const float* covs3D,
                           const float* opacities, const float* normals, int32_t* num_contributes,
                           float* rendered_opacity, int32_t* stack_overflow)
{
    if (num_rays < 0 || num_rays > 0x7fffffffll) return invalid("bvh_trace_opacity: bad ray count");
    if (num_rays == 0) return R3DG_OK;
    if (!stack_overflow) return invalid("bvh_trace_opacity: null overflow counter");
    return guarded([&]() -> int {
        hipStream_t stream = (hipStream_t)stream_;
        StageTimer t(stream, ST_BVH_TRACE);
        bvh_trace_opacity(stream, (int)num_rays, num_gaussians, nodes, aabbs, rays_o, rays_d, means3D, covs3D, opacities,
                          normals, num_contributes, rendered_opacity, stack_overflow);
        check_launch(stream, false, "bvh_trace_opacity");
        t.stop();
        return R3DG_OK;
    });
}

size_t r3dg_bvh_trace_records_bytes(int num_gaussians)
{
    return bvh_trace_records_bytes((size_t)(num_gaussians > 0 ? num_gaussians : 0));
}

int r3dg_bvh_pack_traversal(void* stream_, int num_gaussians, const int32_t* nodes, const float* aabbs, const float* means3D,
                            const float* covs3D, const float* opacities, const float* normals, void* records)
{
    if (num_gaussians < 0) return invalid("bvh_pack_traversal: bad Gaussian count");
    if (num_gaussians == 0) return R3DG_OK;
    if (!nodes || !aabbs || !means3D || !covs3D || !opacities || !normals || !records)
        return invalid("bvh_pack_traversal: null buffer");
    return guarded([&]() -> int {
        bvh_pack_traversal((hipStream_t)stream_, num_gaussians, nodes, aabbs, means3D, covs3D, opacities, normals, records);
        check_launch((hipStream_t)stream_, false, "bvh_pack_traversal");
        return R3DG_OK;
    });
}

int r3dg_bvh_trace_opacity_packed(void* stream_, int64_t num_rays, int num_gaussians, void* records, const float* rays_o,
                                  const float* rays_d, int32_t* num_contributes, float* rendered_opacity,
                                  int32_t* stack_overflow)
{
    if (num_rays < 0 || num_rays > 0x7fffffffll) return invalid("bvh_trace_opacity_packed: bad ray count");
    if (num_gaussians <= 0) return invalid("bvh_trace_opacity_packed: bad Gaussian count");
    if (num_rays == 0) return R3DG_OK;
    if (!records || !rays_o || !rays_d || !num_contributes || !rendered_opacity || !stack_overflow)
        return invalid("bvh_trace_opacity_packed: null buffer");
    return guarded([&]() -> int {
        hipStream_t stream = (hipStream_t)stream_;
        StageTimer t(stream, ST_BVH_TRACE);
        bvh_trace_opacity_packed(stream, (int)num_rays, num_gaussians, records, rays_o, rays_d, num_contributes,
                                 rendered_opacity, stack_overflow);
        check_launch(stream, false, "bvh_trace_opacity_packed");
        t.stop();
        return R3DG_OK;
    });
}

int r3dg_bvh_trace_bundles(void* stream_, int num_gaussians, int K, void* records, const int32_t* nodes, const float* zsamples,
                           int leaf_lo, int leaf_hi, float origin_offset, float* visibility, int32_t* num_contributes,
                           float* dirs_out, int32_t* stack_overflow)
{
    if (num_gaussians < 0) return invalid("bvh_trace_bundles: bad Gaussian count");
    if (K <= 0) return invalid("bvh_trace_bundles: bad sample count");
    if ((int64_t)num_gaussians * K > 0x7fffffffll) return invalid("bvh_trace_bundles: num_gaussians * K does not fit the ray index");
    if (leaf_lo < 0 || leaf_hi < leaf_lo || leaf_hi > num_gaussians) return invalid("bvh_trace_bundles: bad leaf range");
    if (num_gaussians == 0 || leaf_lo == leaf_hi) return R3DG_OK;
    if (!records || !nodes || !zsamples || !visibility || !stack_overflow) return invalid("bvh_trace_bundles: null buffer");
    return guarded([&]() -> int {
        hipStream_t stream = (hipStream_t)stream_;
        StageTimer t(stream, ST_BVH_TRACE);
        bvh_trace_bundles(stream, num_gaussians, K, records, nodes, zsamples, leaf_lo, leaf_hi, origin_offset, visibility,
                          num_contributes, dirs_out, stack_overflow);
        check_launch(stream, false, "bvh_trace_bundles");
        t.stop();
        return R3DG_OK;
    });
}

int r3dg_bvh_trace_hemisphere(void* stream_, int num_gaussians, int T, void* records, const int32_t* nodes, const float* raw_dirs,
                              int leaf_lo, int leaf_hi, float origin_offset, float* visibility, float* dirs_out,
                              int32_t* num_contributes, int32_t* stack_overflow)
{
    if (num_gaussians < 0) return invalid("bvh_trace_hemisphere: bad Gaussian count");
    if (T < 0) return invalid("bvh_trace_hemisphere: bad iteration count");
    if ((int64_t)num_gaussians * T > 0x7fffffffll) return invalid("bvh_trace_hemisphere: num_gaussians * T does not fit the ray index");
    if (leaf_lo < 0 || leaf_hi < leaf_lo || leaf_hi > num_gaussians) return invalid("bvh_trace_hemisphere: bad leaf range");
    if (num_gaussians == 0 || T == 0 || leaf_lo == leaf_hi) return R3DG_OK;
    if (!records || !nodes || !raw_dirs || !visibility || !dirs_out || !stack_overflow)
        return invalid("bvh_trace_hemisphere: null buffer");
    return guarded([&]() -> int {
        hipStream_t stream = (hipStream_t)stream_;
        StageTimer t(stream, ST_BVH_TRACE);
        bvh_trace_hemisphere(stream, num_gaussians, T, records, nodes, raw_dirs, leaf_lo, leaf_hi, origin_offset, visibility,
                             dirs_out, num_contributes, stack_overflow);
        check_launch(stream, false, "bvh_trace_hemisphere");
        t.stop();
        return R3DG_OK;
    });
}

int r3dg_visibility_sh_fit_loss_rows(int P) { return visibility_sh_fit_loss_rows(P); }

int r3dg_visibility_sh_fit(void* stream_, int P, int T, int64_t steps_done, const float* dirs, const float* visibility, float lr,
                           float beta1, float beta2, float eps, float* coeffs, float* exp_avg, float* exp_avg_sq,
                           float* loss_partials)
{
    if (P < 0 || T < 0 || steps_done < 0) return invalid("visibility_sh_fit: bad P, T or step count");
    if ((int64_t)P * T > 0x7fffffffll) return invalid("visibility_sh_fit: P * T does not fit the row index");
    if (!(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f)) return invalid("visibility_sh_fit: betas must be in [0, 1)");
    if (P == 0 || T == 0) return R3DG_OK;
    if (!dirs || !visibility || !coeffs || !exp_avg || !exp_avg_sq) return invalid("visibility_sh_fit: null buffer");
    return guarded([&]() -> int {
        hipStream_t stream = (hipStream_t)stream_;
        StageTimer t(stream, ST_ADAM);
        visibility_sh_fit(stream, P, T, (long long)steps_done, dirs, visibility, lr, beta1, beta2, eps, coeffs, exp_avg, exp_avg_sq,
                          loss_partials);
        check_launch(stream, false, "visibility_sh_fit");
        t.stop();
        return R3DG_OK;
    });
}

int r3dg_bvh_trace_visits(void* stream_, int num_gaussians, const void* records, uint64_t* node_and_leaf_steps)
{
    if (num_gaussians <= 0 || !records || !node_and_leaf_steps) return invalid("bvh_trace_visits: bad arguments");
    return guarded([&]() -> int {
        unsigned long long v[2];
        bvh_trace_visits((hipStream_t)stream_, num_gaussians, records, v);
        node_and_leaf_steps[0] = v[0];
        node_and_leaf_steps[1] = v[1];
        return R3DG_OK;
    });
}

int r3dg_bvh_trace_count(void* stream_, int64_t num_rays, const int32_t* nodes, const float* aabbs, const float* rays_o,
                         const float* rays_d, int32_t* num_contributes, int32_t* stack_overflow)
{
    if (num_rays < 0 || num_rays > 0x7fffffffll) return invalid("bvh_trace_count: bad ray count");
    if (num_rays == 0) return R3DG_OK;
    if (!nodes || !aabbs || !rays_o || !rays_d || !num_contributes || !stack_overflow)
        return invalid("bvh_trace_count: null buffer");
    return guarded([&]() -> int {
        bvh_trace_count((hipStream_t)stream_, (int)num_rays, nodes, aabbs, rays_o, rays_d, num_contributes, stack_overflow);
        check_launch((hipStream_t)stream_, false, "bvh_trace_count");
        return R3DG_OK;
    });
}

int r3dg_bvh_trace_fill(void* stream_, int64_t num_rays, const int32_t* nodes, const float* aabbs, const float* rays_o,
                        const float* rays_d, const float* means3D, const int32_t* num_contributes,
                        const int64_t* offsets_inclusive, uint64_t* keys, int32_t* point_list, float* position_list,
                        int32_t* ray_id_list)
{
    if (num_rays < 0 || num_rays > 0x7fffffffll) return invalid("bvh_trace_fill: bad ray count");
    if (num_rays == 0) return R3DG_OK;
    if (!nodes || !aabbs || !rays_o || !rays_d || !means3D || !num_contributes || !offsets_inclusive || !keys ||
        !point_list || !position_list || !ray_id_list)
        return invalid("bvh_trace_fill: null buffer");
    return guarded([&]() -> int {
        bvh_trace_fill((hipStream_t)stream_, (int)num_rays, nodes, aabbs, rays_o, rays_d, means3D, num_contributes,
                       offsets_inclusive, keys, point_list, position_list, ray_id_list);
        check_launch((hipStream_t)stream_, false, "bvh_trace_fill");
        return R3DG_OK;
    });
}

}  // extern "C"
