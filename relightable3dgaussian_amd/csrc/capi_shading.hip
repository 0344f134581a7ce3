// C ABI of the shading kernels and the render-equation ops (include/r3dg_hip.h): argument checks, stage timing and the
// stream choreography of the fixed-ray-set forward / backward.
#include "capi_internal.hpp"

using namespace r3dg;

extern "C" {

int r3dg_shade_forward_cached(void* stream_, int P, int K, int M, const float* base_color, const float* roughness,
                              const float* normals, const float* viewdirs, const float* incidents, const float* env,
                              int He, int We, const float* env_transform, const float* visibility,
                              const float* incident_dirs, const float* incident_areas, float uniform_area,
                              const uint32_t* taps, int flags, float* out)
{
    if (P < 0 || K <= 0 || He <= 0 || We <= 0) return invalid("shade_forward: bad P/K/env size");
    if (He > 32767 || We > 32767) return invalid("shade_forward: environment map larger than 32767 texels per side");
    if (M != 1 && M != 4 && M != 9 && M != 16) return invalid("shade_forward: incidents must hold 1, 4, 9 or 16 SH coefficients");
    if (P == 0) return R3DG_OK;
    if (!base_color || !roughness || !normals || !viewdirs || !incidents || !env || !visibility || !incident_dirs || !out)
        return invalid("shade_forward: null buffer");
    return guarded([&]() -> int {
        hipStream_t stream = (hipStream_t)stream_;
        StageTimer t(stream, ST_SHADE_FWD);
        launch_shade_forward(stream, P, K, M, base_color, roughness, normals, viewdirs, incidents, env, He, We,
                             env_transform, visibility, incident_dirs, incident_areas, out, taps,
                             (flags & R3DG_SHADE_TRAIN_OUTPUTS) != 0, uniform_area, (flags & R3DG_SHADE_TAPS_ARE_RADIANCE) != 0,
                             (flags & R3DG_SHADE_LEAVE_ROOM) != 0);
        check_launch(stream, false, "shade_forward");
        t.stop();
        return R3DG_OK;
    });
}

int r3dg_shade_forward(void* stream_, int P, int K, int M, const float* base_color, const float* roughness,
                       const float* normals, const float* viewdirs, const float* incidents, const float* env, int He,
                       int We, const float* env_transform, const float* visibility, const float* incident_dirs,
                       const float* incident_areas, float* out)
{
    return r3dg_shade_forward_cached(stream_, P, K, M, base_color, roughness, normals, viewdirs, incidents, env, He, We,
                                     env_transform, visibility, incident_dirs, incident_areas, 0.f, nullptr, 0, out);
}

int r3dg_shade_build_taps(void* stream_, int64_t num_samples, const float* incident_dirs, const float* env_transform,
                          int He, int We, const float* env_radiance, uint32_t* taps)
{
    if (num_samples < 0 || He <= 0 || We <= 0 || He > 32767 || We > 32767) return invalid("shade_build_taps: bad sizes");
    if (num_samples == 0) return R3DG_OK;
    if (!incident_dirs || !taps) return invalid("shade_build_taps: null buffer");
    return guarded([&]() -> int {
        launch_shade_build_taps((hipStream_t)stream_, (size_t)num_samples, incident_dirs, env_transform, He, We,
                                env_radiance, taps);
        return R3DG_OK;
    });
}

int r3dg_shade_build_transport(void* stream_, int P, int K, int M, const float* normals, const float* incidents,
                               const float* visibility, const float* incident_dirs, const float* incident_areas,
                               float uniform_area, float* radiance_inout, float* consts)
{
    if (P < 0 || K <= 0) return invalid("shade_build_transport: bad P/K");
    if (M != 1 && M != 4 && M != 9 && M != 16) return invalid("shade_build_transport: incidents must hold 1, 4, 9 or 16 SH coefficients");
    if (P == 0) return R3DG_OK;
    if (!normals || !incidents || !visibility || !incident_dirs || !radiance_inout || !consts)
        return invalid("shade_build_transport: null buffer");
    return guarded([&]() -> int {
        launch_shade_build_transport((hipStream_t)stream_, P, K, M, normals, incidents, visibility, incident_dirs,
                                     incident_areas, uniform_area, radiance_inout, consts);
        return R3DG_OK;
    });
}

int r3dg_shade_build_transport_rayset(void* stream_, int P, int K, int M, const float* normals, const float* incidents,
                                      const float* visibility, const float* zsamples, float uniform_area, const float* env,
                                      int He, int We, const float* env_transform, float* transport, float* consts)
{
    if (P < 0 || K <= 0) return invalid("shade_build_transport_rayset: bad P/K");
    if (M != 1 && M != 4 && M != 9 && M != 16)
        return invalid("shade_build_transport_rayset: incidents must hold 1, 4, 9 or 16 SH coefficients");
    if (He <= 0 || We <= 0 || He > 32767 || We > 32767) return invalid("shade_build_transport_rayset: bad env size");
    if (P == 0) return R3DG_OK;
    if (!normals || !incidents || !visibility || !zsamples || !env || !transport || !consts)
        return invalid("shade_build_transport_rayset: null buffer");
    return guarded([&]() -> int {
        launch_shade_build_transport_rayset((hipStream_t)stream_, P, K, M, normals, incidents, visibility, zsamples, uniform_area,
                                            env, He, We, env_transform, transport, consts);
        return R3DG_OK;
    });
}

int r3dg_shade_build_transport_baked(void* stream_, int P, int K, int M, const float* normals, const float* incidents,
                                     const float* visibility_sh, const float* zsamples, float uniform_area, const float* env,
                                     int He, int We, const float* env_transform, float* transport, float* consts)
{
    if (P < 0 || K <= 0) return invalid("shade_build_transport_baked: bad P/K");
    if (M != 1 && M != 4 && M != 9 && M != 16)
        return invalid("shade_build_transport_baked: incidents must hold 1, 4, 9 or 16 SH coefficients");
    if (He <= 0 || We <= 0 || He > 32767 || We > 32767) return invalid("shade_build_transport_baked: bad env size");
    if (P == 0) return R3DG_OK;
    if (!normals || !incidents || !visibility_sh || !zsamples || !env || !transport || !consts)
        return invalid("shade_build_transport_baked: null buffer");
    return guarded([&]() -> int {
        launch_shade_build_transport_baked((hipStream_t)stream_, P, K, M, normals, incidents, visibility_sh, zsamples, uniform_area,
                                           env, He, We, env_transform, transport, consts);
        return R3DG_OK;
    });
}

int r3dg_visibility_sh_expand(void* stream_, int P, int K, const float* normals, const float* zsamples,
                              const float* visibility_sh, float* visibility_out)
{
    if (P < 0 || K <= 0) return invalid("visibility_sh_expand: bad P/K");
    if (P == 0) return R3DG_OK;
    if (!normals || !zsamples || !visibility_sh || !visibility_out) return invalid("visibility_sh_expand: null buffer");
    return guarded([&]() -> int {
        launch_visibility_sh_expand((hipStream_t)stream_, P, K, normals, zsamples, visibility_sh, visibility_out);
        return R3DG_OK;
    });
}

int r3dg_shade_build_split(void* stream_, int P, int K, const int32_t* perm, const float* normals, const float* incidents,
                           const float* visibility, const float* incident_dirs, const float* zsamples, float uniform_area,
                           float* lt, float* vis_t, float* consts)
{
    if (P < 0 || K <= 0 || (K % 4) != 0) return invalid("shade_build_split: bad P/K (K must be a multiple of 4)");
    if (P == 0) return R3DG_OK;
    if (!perm || !normals || !incidents || !visibility || (!incident_dirs && !zsamples) || !lt || !vis_t || !consts)
        return invalid("shade_build_split: null buffer");
    return guarded([&]() -> int {
        launch_shade_build_split((hipStream_t)stream_, P, K, perm, normals, incidents, visibility, incident_dirs, zsamples,
                                 uniform_area, lt, vis_t, consts);
        return R3DG_OK;
    });
}

size_t r3dg_shade_env_footprints_bytes(int He, int We)
{
    return He > 0 && We > 0 ? (size_t)(He + 1) * (size_t)(We + 1) * 48 : 0;
}

int r3dg_shade_env_footprints(void* stream_, int He, int We, const float* env, float* footprints)
{
    if (He <= 0 || We <= 0 || He > 4095 || We > 4095 || !env || !footprints)
        return invalid("shade_env_footprints: bad size or null buffer");
    return guarded([&]() -> int {
        launch_shade_env_footprints((hipStream_t)stream_, He, We, env, footprints);
        return R3DG_OK;
    });
}

int r3dg_shade_forward_split(void* stream_, int P, int K, const int32_t* perm, const float* base_color, const float* roughness,
                             const float* normals, const float* viewdirs, const float* lt, const float* vis_t,
                             const float* consts, const float* zsamples, const float* env_transform, const float* env4, int He,
                             int We, float* out)
{
    if (P < 0 || K <= 0 || (K % 4) != 0 || He <= 0 || We <= 0 || He > 4095 || We > 4095)
        return invalid("shade_forward_split: bad sizes (K must be a multiple of 4)");
    if (P == 0) return R3DG_OK;
    if (!perm || !base_color || !roughness || !normals || !viewdirs || !lt || !vis_t || !consts || !zsamples || !env4 || !out)
        return invalid("shade_forward_split: null buffer");
    return guarded([&]() -> int {
        hipStream_t stream = (hipStream_t)stream_;
        StageTimer t(stream, ST_SHADE_FWD);
        launch_shade_forward_split(stream, P, K, perm, base_color, roughness, normals, viewdirs, lt, vis_t, consts, zsamples,
                                   env_transform, env4, He, We, out);
        t.stop();
        return R3DG_OK;
    });
}

int r3dg_shade_forward_transport(void* stream_, int P, int K, const float* base_color, const float* roughness,
                                 const float* normals, const float* viewdirs, const float* transport, const float* consts,
                                 const float* zsamples, const float* incident_dirs, float* out)
{
    if (P < 0 || K <= 0) return invalid("shade_forward_transport: bad P/K");
    if (P == 0) return R3DG_OK;
    if (!base_color || !roughness || !normals || !viewdirs || !transport || !consts || !out)
        return invalid("shade_forward_transport: null buffer");
    if (!zsamples && !incident_dirs) return invalid("shade_forward_transport: needs d_zsamples or d_incident_dirs");
    return guarded([&]() -> int {
        hipStream_t stream = (hipStream_t)stream_;
        StageTimer t(stream, ST_SHADE_FWD);
        launch_shade_forward_transport(stream, P, K, base_color, roughness, normals, viewdirs, transport, consts, zsamples,
                                       incident_dirs, out);
        t.stop();
        return R3DG_OK;
    });
}

int r3dg_shade_backward_cached(void* stream_, int P, int K, int M, const float* base_color, const float* roughness,
                               const float* normals, const float* viewdirs, const float* incidents, const float* env,
                               int He, int We, const float* env_transform, const float* visibility,
                               const float* incident_dirs, const float* incident_areas, const uint32_t* taps,
                               const float* dL_dpbr, const float* dL_ddiffuse_light, float* dL_dbase_color,
                               float* dL_droughness, float* dL_dviewdirs, float* dL_dincidents, float* dL_denv,
                               const float* block_absmax, int n_block_absmax)
{
    if (P < 0 || K <= 0 || He <= 0 || We <= 0) return invalid("shade_backward: bad P/K/env size");
    if (n_block_absmax < 0) return invalid("shade_backward: bad block_absmax count");
    if (He > 32767 || We > 32767) return invalid("shade_backward: environment map larger than 32767 texels per side");
    if (M != 1 && M != 4 && M != 9 && M != 16) return invalid("shade_backward: incidents must hold 1, 4, 9 or 16 SH coefficients");
    if (P == 0) return R3DG_OK;
    return guarded([&]() -> int {
        hipStream_t stream = (hipStream_t)stream_;
        StageTimer t(stream, ST_SHADE_BWD);
        launch_shade_backward(stream, P, K, M, base_color, roughness, normals, viewdirs, incidents, env, He, We,
                              env_transform, visibility, incident_dirs, incident_areas, dL_dpbr, dL_ddiffuse_light,
                              dL_dbase_color, dL_droughness, dL_dviewdirs, dL_dincidents, dL_denv, taps, block_absmax,
                              n_block_absmax);
        check_launch(stream, false, "shade_backward");
        t.stop();
        return R3DG_OK;
    });
}

size_t r3dg_shade_frs_tables_bytes(int K) { return K > 0 ? shade_frs_table_floats(K) * sizeof(float) : 0; }

int r3dg_shade_frs_supported(int K, int M, int He, int We) { return shade_frs_supported(K, M, He, We) ? 1 : 0; }

int r3dg_shade_frs_build_tables(void* stream_, int K, const float* zsamples, float* tables)
{
    if (K <= 0 || !zsamples || !tables) return invalid("shade_frs_build_tables: bad K or null buffer");
    return guarded([&]() -> int {
        launch_shade_frs_build_tables((hipStream_t)stream_, K, zsamples, tables);
        return R3DG_OK;
    });
}

int r3dg_shade_frs_classify(void* stream_, int P, const float* ray_normals, uint8_t* valid)
{
    if (P < 0) return invalid("shade_frs_classify: bad P");
    if (P == 0) return R3DG_OK;
    if (!ray_normals || !valid) return invalid("shade_frs_classify: null buffer");
    return guarded([&]() -> int {
        launch_shade_frs_classify((hipStream_t)stream_, P, ray_normals, valid);
        return R3DG_OK;
    });
}

int r3dg_shade_frs_rotate(void* stream_, int P, const float* incidents, const float* ray_normals, float* cprime)
{
    if (P < 0) return invalid("shade_frs_rotate: bad sizes");
    if (P == 0) return R3DG_OK;
    if (!incidents || !ray_normals || !cprime) return invalid("shade_frs_rotate: null buffer");
    return guarded([&]() -> int {
        hipStream_t stream = (hipStream_t)stream_;
        StageTimer t(stream, ST_SHADE_AUX);
        launch_shade_frs_forward_aux(stream, P, incidents, ray_normals, cprime);
        return R3DG_OK;
    });
}

int r3dg_shade_frs_build_taps(void* stream_, int P, int K, const float* ray_normals, const float* zsamples, int He, int We,
                              uint32_t* taps)
{
    if (P < 0 || K <= 0 || He <= 0 || We <= 0 || He > 511 || We > 511) return invalid("shade_frs_build_taps: bad sizes");
    if (P == 0) return R3DG_OK;
    if (!ray_normals || !zsamples || !taps) return invalid("shade_frs_build_taps: null buffer");
    return guarded([&]() -> int {
        launch_shade_frs_build_taps((hipStream_t)stream_, P, K, ray_normals, zsamples, He, We, taps);
        return R3DG_OK;
    });
}

int r3dg_shade_frs_forward(void* stream_, int P, int K, const float* base_color, const float* roughness,
                           const float* normals, const float* viewdirs, const float* incidents, const float* env, int He,
                           int We, const float* visibility, float uniform_area, const uint32_t* taps,
                           const float* ray_normals, const float* zsamples, const float* tables, const uint8_t* valid,
                           const int32_t* invalid_list, int n_invalid, float* cprime, int flags, float* out,
                           void* listed_stream_, float* feature_rows)
{
    if (P < 0 || K <= 0 || He <= 0 || We <= 0 || n_invalid < 0 || n_invalid > P) return invalid("shade_frs_forward: bad sizes");
    if (!shade_frs_supported(K, 16, He, We))
        return invalid("shade_frs_forward: needs K % 4 == 0 and an environment texture that fits LDS (r3dg_shade_frs_supported)");
    if (P == 0) return R3DG_OK;
    if (!base_color || !roughness || !normals || !viewdirs || !incidents || !env || !visibility || !taps || !ray_normals ||
        !zsamples || !tables || !valid || !cprime || !out || (n_invalid > 0 && !invalid_list))
        return invalid("shade_frs_forward: null buffer");
    return guarded([&]() -> int {
        hipStream_t stream = (hipStream_t)stream_;
        const bool leave_room = (flags & R3DG_SHADE_LEAVE_ROOM) != 0;
        // the kernel on the listed Gaussians (disjoint rows of `out`) may run on a second stream, ordered after everything
        // queued on `stream` so far: it then runs beside the rotation and the main kernel instead of after them (the CALLER
        // joins that stream before anything reads `out`)
        hipStream_t lstream = listed_stream_ != nullptr ? (hipStream_t)listed_stream_ : stream;
        if (n_invalid > 0) {
            stream_wait_stream(lstream, stream);
            StageTimer t(lstream, ST_SHADE_LISTED);
            launch_shade_frs_forward_listed(lstream, K, base_color, roughness, normals, viewdirs, incidents, env, He, We,
                                            visibility, ray_normals, zsamples, uniform_area, invalid_list, n_invalid, out,
                                            feature_rows);
        }
        if ((flags & R3DG_SHADE_ROTATED) == 0) {
            StageTimer t(stream, ST_SHADE_AUX);
            launch_shade_frs_forward_aux(stream, P, incidents, ray_normals, cprime);
        }
        {
            StageTimer t(stream, ST_SHADE_FWD);
            launch_shade_frs_forward_main(stream, P, K, base_color, roughness, normals, viewdirs, env, He, We, visibility,
                                          uniform_area, taps, ray_normals, tables, valid, cprime, leave_room, out, feature_rows);
        }
        return R3DG_OK;
    });
}

int r3dg_shade_frs_backward(void* stream_, int P, int K, const float* base_color, const float* roughness,
                            const float* normals, const float* viewdirs, const float* incidents, const float* env, int He,
                            int We, const float* visibility, float uniform_area, const uint32_t* taps,
                            const float* ray_normals, const float* zsamples, const float* tables, const uint8_t* valid,
                            const int32_t* invalid_list, int n_invalid, const float* cprime, float* dcprime,
                            const float* dL_dpbr, const float* dL_ddiffuse_light, float* dL_dbase_color,
                            float* dL_droughness, float* dL_dviewdirs, float* dL_dincidents, float* dL_denv,
                            const float* block_absmax, int n_block_absmax, void* rotate_stream_)
{
    // rotate_stream_ == R3DG_SHADE_NO_ROTATION_BACK: the caller finishes dL_dincidents itself (r3dg_shade_frs_incident_chain)
    const bool no_rotation_back = rotate_stream_ == R3DG_SHADE_NO_ROTATION_BACK;
    if (no_rotation_back) rotate_stream_ = nullptr;
    if (P < 0 || K <= 0 || He <= 0 || We <= 0 || n_invalid < 0 || n_invalid > P || n_block_absmax < 0)
        return invalid("shade_frs_backward: bad sizes");
    if (!shade_frs_supported(K, 16, He, We))
        return invalid("shade_frs_backward: needs K % 4 == 0 and an environment texture that fits LDS (r3dg_shade_frs_supported)");
    if (P == 0) return R3DG_OK;
    if (!base_color || !roughness || !normals || !viewdirs || !incidents || !env || !visibility || !taps || !ray_normals ||
        !zsamples || !tables || !valid || !cprime || !dcprime || !dL_dpbr || !dL_ddiffuse_light || !dL_dbase_color ||
        !dL_droughness || !dL_dviewdirs || !dL_dincidents || !dL_denv || (n_invalid > 0 && !invalid_list))
        return invalid("shade_frs_backward: null buffer");
    return guarded([&]() -> int {
        hipStream_t stream = (hipStream_t)stream_;
        int gmax_n = 1;
        const unsigned int* gmax;
        {
            StageTimer t(stream, ST_SHADE_AUX);
            gmax = launch_shade_frs_backward_aux(stream, P, dL_dpbr, dL_ddiffuse_light, block_absmax, n_block_absmax, &gmax_n);
        }
        // the kernel on the listed Gaussians goes FIRST (its rows of the per-Gaussian outputs are disjoint from the main
        // kernel's, the texture gradient is accumulated by both): a small launch that a caller can put beside whatever it has
        // running on another stream at this point (fused_step: the rasterizer's per-Gaussian geometry backward)
        // (measured the other way round, round 4: listed AFTER the main kernel lets the geometry backward and the SH group's Adam run
        // into the main kernel's start instead -- shading backward 0.243 -> 0.355 ms, 687 -> 642 it/s)
        if (n_invalid > 0) {
            StageTimer t(stream, ST_SHADE_LISTED);
            launch_shade_frs_backward_listed(stream, K, base_color, roughness, normals, viewdirs, incidents, env, He, We,
                                             visibility, ray_normals, zsamples, uniform_area, invalid_list, n_invalid, dL_dpbr,
                                             dL_ddiffuse_light, dL_dbase_color, dL_droughness, dL_dviewdirs, dL_dincidents,
                                             dL_denv, gmax, gmax_n);
        }
        {
            StageTimer t(stream, ST_SHADE_BWD);
            launch_shade_frs_backward_main(stream, P, K, base_color, roughness, normals, viewdirs, env, He, We, visibility,
                                           uniform_area, taps, ray_normals, tables, valid, cprime, dcprime, dL_dpbr,
                                           dL_ddiffuse_light, dL_dbase_color, dL_droughness, dL_dviewdirs, dL_denv, gmax, gmax_n);
        }
        // the rotation back may run on a second stream (ordered after the main kernel by an event; the CALLER joins that stream
        // before anything reads dL_dincidents): it then overlaps whatever the caller queues next on `stream`.  It leaves the
        // listed Gaussians' rows (written above) alone.
        if (no_rotation_back) return R3DG_OK;
        hipStream_t rstream = rotate_stream_ != nullptr ? (hipStream_t)rotate_stream_ : stream;
        stream_wait_stream(rstream, stream);
        {
            StageTimer t(rstream, ST_SHADE_AUX);
            launch_shade_frs_backward_rotate(rstream, P, ray_normals, dcprime, dL_dincidents, n_invalid > 0 ? valid : nullptr);
        }
        return R3DG_OK;
    });
}

int r3dg_shade_frs_incident_chain(void* stream_, int P, const float* ray_normals, const uint8_t* valid, const float* dcprime,
                                  float* dL_dincidents, float* incidents, float* exp_avg, float* exp_avg_sq, float* cprime,
                                  float lr, float lr_tail, float beta1, float beta2, float eps, int step, float grad_scale,
                                  const float* skip_flag, int chain_flags)
{
    if (P < 0) return invalid("shade_frs_incident_chain: bad sizes");
    if (chain_flags & ~(R3DG_CHAIN_LISTED_ROWS_IN_DCPRIME | R3DG_CHAIN_NO_GRADIENT_OUT))
        return invalid("shade_frs_incident_chain: unknown R3DG_CHAIN_* bit");
    if (step < 1) return invalid("shade_frs_incident_chain: step counts from 1");
    if (P == 0) return R3DG_OK;
    if (!ray_normals || !dcprime || !dL_dincidents || !incidents || !exp_avg || !exp_avg_sq || !cprime)
        return invalid("shade_frs_incident_chain: null buffer");
    return guarded([&]() -> int {
        hipStream_t stream = (hipStream_t)stream_;
        StageTimer t(stream, ST_SHADE_AUX);
        launch_shade_frs_incident_chain(stream, P, ray_normals, valid, dcprime, dL_dincidents, incidents, exp_avg, exp_avg_sq,
                                        cprime, lr, lr_tail, beta1, beta2, eps, step, grad_scale, skip_flag,
                                        (chain_flags & R3DG_CHAIN_LISTED_ROWS_IN_DCPRIME) ? 1 : 0,
                                        !(chain_flags & R3DG_CHAIN_NO_GRADIENT_OUT));
        return R3DG_OK;
    });
}

int r3dg_shade_backward(void* stream_, int P, int K, int M, const float* base_color, const float* roughness,
                        const float* normals, const float* viewdirs, const float* incidents, const float* env, int He,
                        int We, const float* env_transform, const float* visibility, const float* incident_dirs,
                        const float* incident_areas, const float* dL_dpbr, const float* dL_ddiffuse_light,
                        float* dL_dbase_color, float* dL_droughness, float* dL_dviewdirs, float* dL_dincidents,
                        float* dL_denv)
{
    return r3dg_shade_backward_cached(stream_, P, K, M, base_color, roughness, normals, viewdirs, incidents, env, He, We,
                                      env_transform, visibility, incident_dirs, incident_areas, nullptr, dL_dpbr,
                                      dL_ddiffuse_light, dL_dbase_color, dL_droughness, dL_dviewdirs, dL_dincidents, dL_denv,
                                      nullptr, 0);
}

static int re_check(int P, int Si, int Sd, int Sv, int K)
{
    if (P < 0 || K <= 0) return invalid("render_equation: bad P/sample_num");
    if (Si < 0 || Si > 16 || Sd < 0 || Sd > 16 || Sv < 0 || Sv > 16)
        return invalid("render_equation: SH coefficient counts must be in [0,16]");
    return R3DG_OK;
}

int r3dg_render_equation_forward(void* stream_, int P, int Si, int Sd, int Sv, const float* base_color,
                                 const float* roughness, const float* metallic, const float* normals,
                                 const float* viewdirs, const float* incidents_shs, const float* direct_shs,
                                 const float* visibility_shs, int sample_num, const float* rand_float,
                                 float* incident_dirs, float* pbr, float* diffuse_light)
{
    if (int e = re_check(P, Si, Sd, Sv, sample_num)) return e;
    if (P == 0) return R3DG_OK;
    return guarded([&]() -> int {
        hipStream_t stream = (hipStream_t)stream_;
        launch_re_forward(stream, false, P, Si, Sd, Sv, base_color, roughness, metallic, normals, viewdirs, incidents_shs,
                          direct_shs, visibility_shs, sample_num, rand_float, incident_dirs, pbr, nullptr, nullptr,
                          nullptr, nullptr, diffuse_light, nullptr, nullptr, nullptr, nullptr);
        check_launch(stream, false, "render_equation_forward");
        return R3DG_OK;
    });
}

int r3dg_render_equation_forward_complex(void* stream_, int P, int Si, int Sd, int Sv, const float* base_color,
                                         const float* roughness, const float* metallic, const float* normals,
                                         const float* viewdirs, const float* incidents_shs, const float* direct_shs,
                                         const float* visibility_shs, int sample_num, float* incident_dirs, float* pbr,
                                         float* incident_lights, float* local_incident_lights,
                                         float* global_incident_lights, float* incident_visibility, float* diffuse_light,
                                         float* local_diffuse_light, float* accum, float* rgb_d, float* rgb_s)
{
    if (int e = re_check(P, Si, Sd, Sv, sample_num)) return e;
    if (P == 0) return R3DG_OK;
    return guarded([&]() -> int {
        hipStream_t stream = (hipStream_t)stream_;
        launch_re_forward(stream, true, P, Si, Sd, Sv, base_color, roughness, metallic, normals, viewdirs, incidents_shs,
                          direct_shs, visibility_shs, sample_num, nullptr, incident_dirs, pbr, incident_lights,
                          local_incident_lights, global_incident_lights, incident_visibility, diffuse_light,
                          local_diffuse_light, accum, rgb_d, rgb_s);
        check_launch(stream, false, "render_equation_forward_complex");
        return R3DG_OK;
    });
}

int r3dg_render_equation_backward(void* stream_, int P, int Si, int Sd, int Sv, const float* base_color,
                                  const float* roughness, const float* metallic, const float* normals,
                                  const float* viewdirs, const float* incidents_shs, const float* direct_shs,
                                  const float* visibility_shs, int sample_num, const float* incident_dirs,
                                  const float* dL_dpbr, const float* dL_ddiffuse_light, float* dL_dbase_color,
                                  float* dL_droughness, float* dL_dmetallic, float* dL_dnormals, float* dL_dviewdirs,
                                  float* dL_dincidents_shs, float* dL_ddirect_shs, float* dL_dvisibility_shs)
{
    if (int e = re_check(P, Si, Sd, Sv, sample_num)) return e;
    if (P == 0) return R3DG_OK;
    return guarded([&]() -> int {
        hipStream_t stream = (hipStream_t)stream_;
        launch_re_backward(stream, P, Si, Sd, Sv, base_color, roughness, metallic, normals, viewdirs, incidents_shs,
                           direct_shs, visibility_shs, sample_num, incident_dirs, dL_dpbr, dL_ddiffuse_light,
                           dL_dbase_color, dL_droughness, dL_dmetallic, dL_dnormals, dL_dviewdirs, dL_dincidents_shs,
                           dL_ddirect_shs, dL_dvisibility_shs);
        check_launch(stream, false, "render_equation_backward");
        return R3DG_OK;
    });
}

}  // extern "C"
