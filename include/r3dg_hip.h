/*
 * r3dg_hip.h -- C ABI of libr3dg_hip.so, the MI355X (gfx950) implementation of the relightable-3DGS
 * hot path.  Plain pointers and sizes only; every pointer named d_* is DEVICE memory (HBM), everything
 * is fp32 / int32 unless stated.  All entry points enqueue work on `stream` (a hipStream_t passed as
 * void*; NULL = the null stream) and return 0 on success or a negative R3DG_E* code; the failing call's
 * message is available from r3dg_last_error().
 *
 * Each entry point replaces one function of the reference's pybind boundary (file:line under
 * NJU-3DV/Relightable3DGaussian):
 *   r3dg_rasterize_forward   <- CudaRasterizer::Rasterizer::forward   (cuda_rasterizer/rasterizer.h:31-66,
 *                               called from RasterizeGaussiansCUDA, rasterize_points.cu:36-141)
 *   r3dg_rasterize_backward  <- CudaRasterizer::Rasterizer::backward  (cuda_rasterizer/rasterizer.h:68-98,
 *                               called from RasterizeGaussiansBackwardCUDA, rasterize_points.cu:143-235)
 *   r3dg_mark_visible        <- CudaRasterizer::Rasterizer::markVisible (rasterizer.h:24-29, rasterize_points.cu:237-255)
 *   r3dg_shade_*             <- neilf.py:339-407 rendering_equation / GGX_specular (the LIVE stage-2 model)
 *   r3dg_render_equation_*   <- render_equation.h:7-46 (RenderEquationForwardCUDA / _complex / BackwardCUDA)
 *   r3dg_bvh_build           <- construct_bvh (bvh/include/construct.cuh, bvh/src/construct.cu:147-265)
 *   r3dg_bvh_trace_opacity   <- trace_bvh_opacity_cuda (bvh/include/trace.cuh:50-55, bvh/src/trace.cu:196-286)
 *   r3dg_knn_dist2           <- SimpleKNN::knn (submodules/simple-knn/simple_knn.cu:185-221)
 *   r3dg_densify_*           <- GaussianModel.add_densification_stats / densify_and_prune / prune / reset_opacity
 *                               (scene/gaussian_model.py:931-937, :893-915, :917-929, :563-566; train.py:158-175)
 */
#ifndef R3DG_HIP_H
#define R3DG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define R3DG_OK 0
#define R3DG_EINVAL (-1)   /* bad argument (shape / S limit / null pointer)  -> RuntimeError in the host mirror */
#define R3DG_EHIP (-2)     /* a HIP runtime call or kernel launch failed                                      */
#define R3DG_EALLOC (-3)   /* a resize callback returned NULL                                                 */

/* Resize callback, the C form of the reference's std::function<char*(size_t)> (rasterizer.h:32-34):
 * must return a DEVICE pointer to at least `bytes` bytes that stays valid until the matching backward. */
typedef void* (*r3dg_alloc_fn)(void* user, size_t bytes);

const char* r3dg_last_error(void);
/* Frees every scratch buffer the library holds (grow-only buffers per (device, stream): the tile backward's gradient records,
 * the shading kernels' records, the trace kernel's ray records; raw hipMalloc, outside any caching allocator).  Synchronises the
 * device.  Call it after a stream the library ran on has been destroyed, or to hand the memory back between phases; the next call
 * that needs a buffer allocates it again.  Not for use during stream capture (hipMalloc / hipFree). */
int r3dg_release_scratch(void);
int r3dg_version(void);

/* Limits (reference: forward F[33] forward.cu:312, backward 24 backward.cu:449). Ours: both 36. */
int r3dg_max_features_forward(void);
int r3dg_max_features_backward(void);

/* Scratch sizes (bytes) of the three opaque state buffers (rasterizer_impl.h:213-265 `required<T>`). */
size_t r3dg_geometry_state_bytes(int P);
size_t r3dg_image_state_bytes(int width, int height);
size_t r3dg_binning_state_bytes(int64_t num_rendered);
/* Byte offsets of named sub-arrays inside the state buffers, for tests/debugging only.
 * geometry: 0 depths f32[P], 1 clamped u8[3P], 2 radii i32[P], 3 means2D f32[2P], 4 cov3D f32[6P],
 *           5 conic_opacity f32[4P], 6 rgb f32[3P], 7 tiles_touched u32[P], 8 point_offsets u32[P]
 * image:    0 final_T f32[N], 1 n_contrib u32[N], 2 ranges u32[2T]
 * binning:  0 keys_unsorted u64[R], 1 keys u64[R], 2 vals_unsorted u32[R], 3 point_list u32[R] */
int r3dg_geometry_state_offsets(int P, size_t* offsets9);
/* byte offset of the uint64 instance count (num_rendered) of the last forward inside the geometry state */
size_t r3dg_geometry_state_total_offset(int P);
int r3dg_image_state_offsets(int width, int height, size_t* offsets3);
int r3dg_binning_state_offsets(int64_t num_rendered, size_t* offsets4);

/* Forward. Optional inputs (d_shs, d_colors_precomp, d_scales, d_rotations, d_cov3D_precomp) are NULL when
 * absent, exactly like the reference's nullptr convention (forward.cu:206,242).  Every image output and d_radii is
 * fully written (uninitialised memory is fine); only d_out_weights is accumulated and must be zero-filled by the
 * caller (the reference zero-fills everything, rasterize_points.cu:72-79).  `d_radii` may be NULL; so may d_out_weights
 * (the per-Gaussian blend weights, read by the densification statistics only: then they are not computed).
 * Returns num_rendered in *num_rendered_out.  One device->host sync (rasterizer_impl.cu:291). */
int r3dg_rasterize_forward(void* stream, r3dg_alloc_fn geometry_alloc, r3dg_alloc_fn binning_alloc,
                           r3dg_alloc_fn image_alloc, void* alloc_user, int P, int S, int D, int M,
                           const float* d_background, int width, int height, const float* d_means3D,
                           const float* d_shs, const float* d_colors_precomp, const float* d_features,
                           const float* d_opacities, const float* d_scales, float scale_modifier,
                           const float* d_rotations, const float* d_cov3D_precomp, const float* d_viewmatrix,
                           const float* d_projmatrix, const float* d_cam_pos, float tan_fovx, float tan_fovy,
                           float cx, float cy, int prefiltered, int compute_pseudo_normal, float* d_out_color,
                           float* d_out_opacity, float* d_out_depth, float* d_out_feature, float* d_out_normal,
                           float* d_out_surface_xyz, float* d_out_weights, int32_t* d_radii, int debug,
                           int* num_rendered_out);

/* ---- a rasterizer call described by structs ------------------------------------------------------------------------------------
 * r3dg_rasterize_forward_begin[_bounded] and r3dg_rasterize_backward_split take what the two positional entries (whose lists mirror
 * the reference's) spell out as three plain structs of int, float and pointer fields; the field names are those parameters' names.
 * The library copies a struct before the entry point returns, so a caller's struct may be a temporary (what its pointers name must
 * outlive the kernels, as ever).
 *
 * r3dg_raster_scene: what the forward and the backward of a frame both read -- P Gaussians, S feature channels, SH degree D with M
 * coefficients, the image size, the inputs and the camera.  Optional inputs are NULL when absent, as in r3dg_rasterize_forward.
 * d_opacities, cx and cy are read by the FORWARD only (the backward takes opacities from the geometry state and never needs the
 * principal point).  d_campos is the camera position under the backward's name for it (r3dg_rasterize_forward: d_cam_pos). */
typedef struct r3dg_raster_scene {
    int P, S, D, M, width, height;
    const float* d_background; const float* d_means3D; const float* d_shs; const float* d_colors_precomp; const float* d_features;
    const float* d_opacities; const float* d_scales;
    float scale_modifier;
    const float* d_rotations; const float* d_cov3D_precomp;
    const float* d_viewmatrix; const float* d_projmatrix; const float* d_campos;
    float tan_fovx, tan_fovy, cx, cy;
} r3dg_raster_scene;
/* r3dg_raster_outputs: the forward's own arguments, with r3dg_rasterize_forward's rules (d_out_weights zero-filled by the caller or
 * NULL, d_radii may be NULL, everything else fully written). */
typedef struct r3dg_raster_outputs {
    int prefiltered, compute_pseudo_normal, debug;
    float* d_out_color; float* d_out_opacity; float* d_out_depth; float* d_out_feature; float* d_out_normal;
    float* d_out_surface_xyz; float* d_out_weights;
    int32_t* d_radii;
} r3dg_raster_outputs;

/* The forward in two halves.  _begin takes the arguments of r3dg_rasterize_forward as structs, runs the projection and starts the
 * asynchronous read-back of num_rendered (an event is recorded on `stream`); _finish waits for that event only, sizes the
 * binning state, orders the instances and renders.  Kernels the caller enqueues on `stream` between the two calls run
 * while the host waits for the count -- `d_features` (and every other pointer) is only dereferenced by the device, so the
 * feature rows may be produced in between.  *ticket is NULL when P == 0; _finish(NULL) is a no-op.  Every ticket must be
 * finished exactly once.  r3dg_rasterize_forward == _begin immediately followed by _finish. */
int r3dg_rasterize_forward_begin(void* stream, r3dg_alloc_fn geometry_alloc, r3dg_alloc_fn binning_alloc,
                                 r3dg_alloc_fn image_alloc, void* alloc_user, const r3dg_raster_scene* scene,
                                 const r3dg_raster_outputs* outputs, void** ticket);
int r3dg_rasterize_forward_finish(void* ticket, int* num_rendered_out);
/* _finish with the instance ordering (key duplication, sort, tile ranges) on `ordering_stream` (NULL = the forward's
 * stream): it waits for the projection only and is joined before the tile kernel, so it can run concurrently with
 * whatever the caller queued on the forward's stream after _begin.  The binning state buffer is first touched on
 * `ordering_stream`. */
int r3dg_rasterize_forward_finish_on(void* ticket, void* ordering_stream, int* num_rendered_out);

/* The forward WITHOUT the host read-back of num_rendered (the reference's one synchronisation per forward,
 * rasterizer_impl.cu:291).  _begin_bounded queues the projection AND the instance ordering behind it at once on
 * `ordering_stream` (NULL = `stream`; otherwise ordered after everything queued on `stream` before the call), with the binning
 * state laid out for `capacity` instances (the value to pass as num_rendered to the backward, whose state layout it selects);
 * _finish_bounded makes `main_stream` wait for the ordering and renders there -- kernels the caller queues on `stream` after
 * _begin_ (the feature rows) run beside the whole front end when the two streams differ; the per-Gaussian outputs of the
 * projection (d_radii, the geometry state) are valid on `main_stream` after _finish_bounded.
 * A frame that needs MORE than `capacity` instances is dropped on the device: every tile list comes out empty (the
 * images are background only, n_contrib 0, all gradients of that frame zero) and *d_overflow_flag = 1.0f; otherwise the
 * flag is set to 0.0f (may be NULL); *d_overflow_count (may be NULL) is incremented for every dropped frame and never
 * reset by the library, so a caller that polls rarely still hears about it.  The true count stays readable in the geometry state
 * (r3dg_geometry_state_total_offset).  Needs the direct tile binning (the default) and at most 16384 tiles (a 2048x2048
 * image): its launches do not depend on the count.  r3dg_bounded_forward_supported(width, height) answers 1 when both hold
 * -- callers take the two-phase forward otherwise (_begin_bounded returns R3DG_EINVAL from _finish_bounded if asked anyway). */
int r3dg_bounded_forward_supported(int width, int height);
int r3dg_rasterize_forward_begin_bounded(void* stream, r3dg_alloc_fn geometry_alloc, r3dg_alloc_fn binning_alloc,
                                         r3dg_alloc_fn image_alloc, void* alloc_user, const r3dg_raster_scene* scene,
                                         const r3dg_raster_outputs* outputs, void* ordering_stream, long long capacity,
                                         float* d_overflow_flag, unsigned int* d_overflow_count, void** ticket);
int r3dg_rasterize_forward_finish_bounded(void* ticket, void* main_stream);

/* Backward.  d_dL_dpix_d == NULL: the depth image carries no gradient (the caller's promise; the tile kernel then takes its
 * instances without a depth slot).  Every output is FULLY WRITTEN (zeros for invisible Gaussians, for feature channels outside
 * `active_features` and when nothing was rendered) and may be uninitialised: d_dL_dmean2D [P,3] (z = depth side channel),
 * d_dL_dopacity, d_dL_dcolor, d_dL_dfeature [P,S], d_dL_dmean3D, d_dL_dcov3D and -- when SHs / scales+rotations are the active
 * inputs -- d_dL_dsh, d_dL_dscale, d_dL_drot (otherwise those three are left untouched; the reference zero-fills all ten,
 * rasterize_points.cu:179-188).  d_dL_dconic [P,4] is SCRATCH (it receives the second moments the tile pass accumulates, not the
 * reference's intermediate).  Rounds 1-4 accumulated the first five with atomics into caller-zeroed memory; since round 5 the tile
 * kernel adds into one 64-byte record per Gaussian (library scratch) and a scatter pass writes the arrays. */
int r3dg_rasterize_backward(void* stream, int P, int S, int D, int M, int R, const float* d_background, int width,
                            int height, const float* d_means3D, const float* d_shs, const float* d_features,
                            const float* d_colors_precomp, const float* d_scales, float scale_modifier,
                            const float* d_rotations, const float* d_cov3D_precomp, const float* d_viewmatrix,
                            const float* d_projmatrix, const float* d_campos, float tan_fovx, float tan_fovy,
                            const int32_t* d_radii, const void* d_geom_buffer, const void* d_binning_buffer,
                            const void* d_img_buffer, const float* d_dL_dpix, const float* d_dL_dpix_o,
                            const float* d_dL_dpix_d, const float* d_dL_dpix_f, float* d_dL_dmean2D,
                            float* d_dL_dconic, float* d_dL_dopacity, float* d_dL_dcolor, float* d_dL_dfeature,
                            float* d_dL_dmean3D, float* d_dL_dcov3D, float* d_dL_dsh, float* d_dL_dscale,
                            float* d_dL_drot, int backward_geometry, int debug);

/* r3dg_raster_backward: the backward's own arguments (r3dg_rasterize_backward_split, declared behind r3dg_adam_group below) -- R,
 * d_radii, the three state buffers and the four upstream gradients of r3dg_rasterize_backward, its ten outputs, and
 * active_features: a HOST array of n_active_features distinct channel indices (n_active_features < 0: all S), the caller's promise
 * that every OTHER channel of d_dL_dpix_f is zero everywhere; those channels are then not carried through the tile kernel at all
 * and the scatter pass WRITES ZEROS into their d_dL_dfeature columns (every output is fully written: no zero fill by the caller is
 * needed or relied upon).  Same results, less work: a loss normally reads a few of the S feature maps. */
typedef struct r3dg_raster_backward {
    int R;
    const int32_t* d_radii;
    const void* d_geom_buffer; const void* d_binning_buffer; const void* d_img_buffer;
    const float* d_dL_dpix; const float* d_dL_dpix_o; const float* d_dL_dpix_d; const float* d_dL_dpix_f;
    float* d_dL_dmean2D; float* d_dL_dconic; float* d_dL_dopacity; float* d_dL_dcolor; float* d_dL_dfeature;
    float* d_dL_dmean3D; float* d_dL_dcov3D; float* d_dL_dsh; float* d_dL_dscale; float* d_dL_drot;
    int backward_geometry, debug, n_active_features;
    const int* active_features;
} r3dg_raster_backward;

/* The backward for FROZEN GEOMETRY: only d_dL_dfeature [P,S] (ACCUMULATED with atomics: zero it first) from d_dL_dpix_f
 * [S,H,W].  The stage-2 schedules of script/run_syn4.sh:27-33 and run_dtu.sh set the learning rates of positions, normals, SH
 * colour, opacity, scaling and rotation to 0: every gradient r3dg_rasterize_backward produces except dL_dfeature
 * (= sum over pixels of alpha * T * dL_dpixel_f, backward.cu:566) is then multiplied by 0 in the optimizer, so neither the
 * alpha-gradient recursion of the tile kernel nor the per-Gaussian geometry backward (K12 + K13) needs to run.  Same state
 * buffers, same active_features contract as r3dg_rasterize_backward_split; values equal that call's d_dL_dfeature up to the
 * order of the float atomics. */
int r3dg_rasterize_backward_features(void* stream, int P, int S, int R, int width, int height, const void* d_geom_buffer,
                                     const void* d_binning_buffer, const void* d_img_buffer, const float* d_dL_dpix_f,
                                     float* d_dL_dfeature, int n_active_features, const int* active_features, int debug);

int r3dg_mark_visible(void* stream, int P, const float* d_means3D, const float* d_viewmatrix,
                      const float* d_projmatrix, uint8_t* d_present);

/* Fused per-Gaussian shading integral, LIVE model (gaussian_renderer/neilf.py:339-407): for each Gaussian the mean
 * over K cached samples of (albedo/pi + GGX) * (max(SH_local(d),0) + env(d)*vis) * area * max(n.d,0).
 *   base_color[P,3] roughness[P] normals[P,3] viewdirs[P,3] incidents[P,M,3] (M = 1,4,9,16 SH coefficients)
 *   env[He,We,3]: ACTIVATED lat-long environment texture (softplus(DirectLightMap.env) or EnvLight.envmap);
 *   env_transform: optional row-major 3x3 light rotation applied to the lookup direction (envmap.py:39-42) or NULL
 *   visibility[P,K] incident_dirs[P,K,3] incident_areas[P,K]  (GaussianModel.update_visibility caches)
 * out[P,19] = pbr(3) diffuse_light(3) specular(3) mean_k incident_lights(3) mean_k local(3) mean_k global(3) mean_k vis(1)
 * Backward: gradients of <pbr,dL_dpbr> + <diffuse_light,dL_ddiffuse_light>; dL_dbase_color[P,3], dL_droughness[P],
 * dL_dviewdirs[P,3], dL_dincidents[P,M,3] are overwritten, dL_denv[He,We,3] is ACCUMULATED (zero it first). */
int r3dg_shade_forward(void* stream, int P, int K, int M, const float* d_base_color, const float* d_roughness,
                       const float* d_normals, const float* d_viewdirs, const float* d_incidents, const float* d_env,
                       int He, int We, const float* d_env_transform, const float* d_visibility,
                       const float* d_incident_dirs, const float* d_incident_areas, float* d_out);
/* The same forward with two optional savings for callers that own the sample caches (fused iteration, relight renderer):
 *   d_taps [P*K*3] uint32: the lat-long lookup of every cached direction (texel corner + two bilinear weights, 12 bytes per
 *     sample), built ONCE per visibility update by r3dg_shade_build_taps for the SAME incident_dirs, env size and
 *     env_transform -- the directions are frozen between updates (gaussian_model.py:312-342), so acos/atan2 need not be
 *     re-evaluated per iteration; NULL = evaluate the lookup in the kernel;
 *   flags & R3DG_SHADE_TRAIN_OUTPUTS: write only pbr (out[:,0:3]), diffuse_light (out[:,3:6]) and the mean visibility (out[:,18]),
 *     the columns the training feature row reads (neilf.py:120-122); the other 12 columns are left untouched;
 *   d_incident_areas == NULL: every sample has the area `uniform_area` (fibonacci_sphere_sampling assigns 2*pi to all of
 *     them, graphics_utils.py:36) -- saves the 4 bytes per sample of the area cache. */
#define R3DG_SHADE_TRAIN_OUTPUTS 1
#define R3DG_SHADE_TAPS_ARE_RADIANCE 2
#define R3DG_SHADE_LEAVE_ROOM 4      /* the caller runs other kernels beside this one: occupy half of each CU */
#define R3DG_SHADE_ROTATED 8         /* r3dg_shade_frs_forward only: d_cprime already holds r3dg_shade_frs_rotate's result */
int r3dg_shade_forward_cached(void* stream, int P, int K, int M, const float* d_base_color, const float* d_roughness,
                              const float* d_normals, const float* d_viewdirs, const float* d_incidents,
                              const float* d_env, int He, int We, const float* d_env_transform,
                              const float* d_visibility, const float* d_incident_dirs, const float* d_incident_areas,
                              float uniform_area, const uint32_t* d_taps, int flags, float* d_out);
/* d_env_radiance == NULL: lookup records.  d_env_radiance = an env[He,We,3] that is NOT being trained (relighting under a fixed
 * HDR map, envmap.py:35-53): the records hold the bilinearly sampled RADIANCE of every cached direction instead -- pass them
 * with R3DG_SHADE_TAPS_ARE_RADIANCE and the shading kernel touches no texture at all. */
int r3dg_shade_build_taps(void* stream, int64_t num_samples, const float* d_incident_dirs, const float* d_env_transform,
                          int He, int We, const float* d_env_radiance, uint32_t* d_taps);
/* Relighting under a FIXED light with static Gaussians (relighting.py:114-170 with configs/teaser, configs/nerf_syn: only the
 * camera moves): the view-independent part of rendering_equation (neilf.py:339-371) as a cache.
 * r3dg_shade_build_transport: d_radiance_inout [P*K*3] holds the sampled radiance of every cached direction
 *   (r3dg_shade_build_taps with d_env_radiance) and is REWRITTEN IN PLACE with the sample's transport
 *   (max(SH_incident(d), 0) + radiance * visibility) * area * max(n . d, 0); d_consts [P*16] receives per Gaussian
 *   diffuse_light 3 | mean incident light 3 | mean local light 3 | mean global light 3 | mean visibility 1 | 3 unused.
 *   Rebuild whenever the light, its rotation, the incident-light coefficients, the normals or the visibility cache change.
 * r3dg_shade_forward_transport: the per-frame remainder -- the GGX lobe of every sample against the cached transport --
 *   writes the same 19 columns per Gaussian as r3dg_shade_forward.  Directions: d_incident_dirs [P,K,3] as cached, or NULL
 *   to regenerate them from the normal and d_zsamples [K,3], the Fibonacci set around +z (graphics_utils.py:9-37 before
 *   the rotation; sh_utils.py:36-68): 12 instead of 24 bytes per sample. */
int r3dg_shade_build_transport(void* stream, int P, int K, int M, const float* d_normals, const float* d_incidents,
                               const float* d_visibility, const float* d_incident_dirs, const float* d_incident_areas,
                               float uniform_area, float* d_radiance_inout, float* d_consts);
int r3dg_shade_forward_transport(void* stream, int P, int K, const float* d_base_color, const float* d_roughness,
                                 const float* d_normals, const float* d_viewdirs, const float* d_transport,
                                 const float* d_consts, const float* d_zsamples, const float* d_incident_dirs,
                                 float* d_out);
/* The same transport cache WITHOUT a stored direction: for callers whose samples are the fixed ray set -- d_k =
 * normalize(R(n) z_k), z_k = d_zsamples [K,3], R = rotation_between_z (the rays r3dg_bvh_trace_bundles generates, csrc/ray_set.hpp)
 * -- with the uniform area `uniform_area`.  One launch does what r3dg_shade_build_taps (with d_env_radiance) followed by
 * r3dg_shade_build_transport does for those directions: per sample the direction is regenerated from d_normals, rotated by
 * d_env_transform [3,3] (NULL = none), looked up in d_env [He,We,3] (lat-long, bilinear, zero padding) and turned into the
 * transport above, which goes to d_transport [P*K*3] (a fresh buffer, nothing is read from it); d_consts [P*16] as above.
 * Streams 4 B (visibility) in and 12 B out per sample where the two-kernel path moves 52 B.  M in {1, 4, 9, 16}, K > 0. */
int r3dg_shade_build_transport_rayset(void* stream, int P, int K, int M, const float* d_normals, const float* d_incidents,
                                      const float* d_visibility, const float* d_zsamples, float uniform_area,
                                      const float* d_env, int He, int We, const float* d_env_transform,
                                      float* d_transport, float* d_consts);
/* The same cache from BAKED visibility: d_visibility_sh [P*16] holds the visibility SH of every Gaussian (visibility_dc |
 * visibility_rest, what r3dg_visibility_sh_fit produces) and the visibility of sample k is clamp(0.5 + sum_i v_i Y_i(d_k), 0, 1)
 * (gaussian_renderer/neilf_composite.py:229-231 with bake=True), evaluated at the WORLD-frame direction d_k whatever
 * d_env_transform is.  No trace and no [P,K] visibility: 0 B in and 12 B out per sample.  The basis of the visibility is always
 * the full 16; M, the count of incident-light coefficients, is as above.
 * r3dg_visibility_sh_expand writes that visibility itself, d_visibility_out [P*K], for the consumers that take a [P,K] tensor
 * (r3dg_shade_build_split, r3dg_shade_forward_cached, r3dg_shade_build_transport). */
int r3dg_shade_build_transport_baked(void* stream, int P, int K, int M, const float* d_normals, const float* d_incidents,
                                     const float* d_visibility_sh, const float* d_zsamples, float uniform_area,
                                     const float* d_env, int He, int We, const float* d_env_transform,
                                     float* d_transport, float* d_consts);
int r3dg_visibility_sh_expand(void* stream, int P, int K, const float* d_normals, const float* d_zsamples,
                              const float* d_visibility_sh, float* d_visibility_out);
/* Relighting under a light that TURNS WITH EVERY FRAME (relighting.py:160-161 with configs/nerf_syn_light or configs/tnt
 * light_transform.json) and static Gaussians: the "split transport" cache holds what does NOT depend on the light --
 *   d_lt [K,P,4]: per sample (max(SH_incident(d), 0) * a, a) with a = area * max(n . d, 0);  d_vis_t [K/4,P,4]: the visibility
 *   (K % 4 == 0);
 *   d_consts [P,4]: mean local light, mean visibility
 * sample-major and in the order d_perm [P] lists the Gaussians (the caller sorts them by normal: all lanes of a wave then look up
 * neighbouring texels) -- and r3dg_shade_forward_split evaluates, per frame, the lat-long lookup of the rotated direction
 * (d_env_footprints: the map as 48-byte bilinear footprints, r3dg_shade_env_footprints into r3dg_shade_env_footprints_bytes(He, We)
 * bytes: a lookup is three 16-byte loads of one record instead of four gathers), the transport and the GGX lobe: the 19 columns of r3dg_shade_forward
 * for 16 incident-light coefficients, a uniform sample area and Fibonacci directions (d_incident_dirs, or NULL to regenerate them
 * from the normals and d_zsamples as the cache was generated). */
int r3dg_shade_build_split(void* stream, int P, int K, const int32_t* d_perm, const float* d_normals, const float* d_incidents,
                           const float* d_visibility, const float* d_incident_dirs, const float* d_zsamples,
                           float uniform_area, float* d_lt, float* d_vis_t, float* d_consts);
size_t r3dg_shade_env_footprints_bytes(int He, int We);
int r3dg_shade_env_footprints(void* stream, int He, int We, const float* d_env, float* d_env_footprints);
int r3dg_shade_forward_split(void* stream, int P, int K, const int32_t* d_perm, const float* d_base_color,
                             const float* d_roughness, const float* d_normals, const float* d_viewdirs, const float* d_lt,
                             const float* d_vis_t, const float* d_consts, const float* d_zsamples,
                             const float* d_env_transform, const float* d_env_footprints, int He, int We, float* d_out);
/* ---- the same integral over a FIXED RAY SET (csrc/shading_frs.hip) -----------------------------------------------------------
 * For callers whose cached directions are the Fibonacci set rotated to each Gaussian's normal, d_k = normalize(R(n) z_k) --
 * what GaussianModel.update_visibility produces (scene/gaussian_model.py:312-342 -> utils/graphics_utils.py:9-37,
 * rotation_between_z utils/sh_utils.py:36-68).  Then NOTHING per sample depends on a stored direction (SURVEY section 8f n2:
 * "store the frozen-normal snapshot, 12 B per Gaussian, instead of the [P,K,3] cache"):
 *   - the local incident light sum_i c_i Y_i(R z_k) equals sum_i c'_i Y_i(z_k) for the ROTATED coefficients c', and Y_i(z_k) is
 *     one K x 16 table for all Gaussians: both SH contractions run on the matrix cores against that constant table;
 *   - every dot product of d_k with a per-Gaussian vector w (the shading normal, the view vector) is z_k . (R^T w): one more
 *     matrix product per vector against the direction rows of the same table; the GGX half-vector terms follow from N.L, N.V
 *     and L.V alone;
 *   - the lat-long lookup of d_k is a constant between visibility updates: 8 bytes per sample (r3dg_shade_frs_build_taps).
 * What the kernels stream per sample: visibility (4 B) + the lookup record (8 B) -- round 3 read 28 B (direction 12, a 12-byte
 * record, visibility 4).  Same outputs and values (fp32 rounding) as r3dg_shade_forward_cached / r3dg_shade_backward_cached
 * with R3DG_SHADE_TRAIN_OUTPUTS and no light rotation; 16 incident-light coefficients, K % 4 == 0, a texture that fits LDS:
 * r3dg_shade_frs_supported.
 *   d_ray_normals [P,3]: the normals the ray set was GENERATED from (the snapshot update_visibility used, not the trained
 *     normal); d_zsamples [K,3]: the z set; d_tables: r3dg_shade_frs_build_tables(K, d_zsamples, r3dg_shade_frs_tables_bytes(K)
 *     bytes); d_taps [P,K,2] uint32: r3dg_shade_frs_build_taps for THIS texture size (rebuilt per visibility update);
 *   d_valid [P] bytes from r3dg_shade_frs_classify: 1 where R(n) is orthonormal to 2e-5 in fp32 -- normals within ~2.5 degrees of
 *     -z lose that to cancellation, their directions are not a rigid copy of the z set, and those Gaussians (d_invalid_list
 *     [n_invalid] int32 row indices, built by the caller from d_valid) are shaded inside the same call by wave-per-Gaussian
 *     kernels that regenerate their directions from the ray normal and evaluate the SH basis there;
 *   d_cprime [P,48]: scratch written by _forward (the rotated coefficients) and read by _backward of the same parameters;
 *   d_dcprime [P,48]: scratch of _backward.
 *   Sample areas: the fixed ray set has ONE area for every sample -- uniform_area, or 2*pi (what fibonacci_sphere_sampling assigns,
 *     utils/graphics_utils.py:36) when uniform_area == 0. */
int r3dg_shade_frs_supported(int K, int M, int He, int We);
size_t r3dg_shade_frs_tables_bytes(int K);
int r3dg_shade_frs_build_tables(void* stream, int K, const float* d_zsamples, float* d_tables);
int r3dg_shade_frs_classify(void* stream, int P, const float* d_ray_normals, uint8_t* d_valid);
/* d_taps [P,K,2]: per sample (x0 + 1) << 23 | mantissa(1 + wx1), (y0 + 1) << 23 | mantissa(1 + wy1) -- the texel corner and the
 * two bilinear weights (23-bit fixed point) of the lat-long lookup (direct_light_map.py:70-83) of d_k = normalize(R(n) z_k),
 * regenerated from the ray normal: no [P,K,3] direction array is read.  He, We <= 511. */
int r3dg_shade_frs_build_taps(void* stream, int P, int K, const float* d_ray_normals, const float* d_zsamples, int He, int We,
                              uint32_t* d_taps);
/* Stream plumbing for callers that spread one iteration over several streams of one device: `waiter` waits for everything queued
 * on `signaller` so far (hipEventRecord + hipStreamWaitEvent on a pooled event -- what the library's own entry points use between
 * the streams they are handed). */
int r3dg_stream_wait_stream(void* waiter, void* signaller);
/* Occupies `stream` (ONE wave, no memory traffic) for `microseconds` of the device's constant-rate wall clock.  Rehearsal tool:
 * fused_step prices an all-reduce it cannot run on a one-GPU box by queueing this behind each bucket's one-rank (identity)
 * collective, sized to the ring time of an assumed bus bandwidth (R3DG_DP_FAKE_COMM_GBS). */
int r3dg_spin(void* stream, float microseconds);
/* *h_pinned_dst = *d_src (8 bytes) behind everything queued on `stream`, written by a one-thread kernel straight into PINNED,
 * device-mapped host memory (hipHostMalloc / torch's pin_memory()) -- how a caller gets a count off the device without waiting
 * for it and without the runtime's blit path (an 8-byte hipMemcpyAsync to pinned memory runs as `__amd_rocclr_copyBuffer`, which
 * showed as 128 us on a hardware queue of the training iteration).  The host reads the slot after synchronising with the stream. */
int r3dg_store_u64_to_host(void* stream, const void* d_src, void* h_pinned_dst);
/* Measurement aid: a device-filling grid of VALU-only waves (iters x 16 fp32 FMAs per lane) that read the shader-clock counter and
 * the constant-rate wall clock on both sides.  d_out3[0] += shader cycles, [1] += wall ticks, [2] += waves (zeroed here);
 * shader clock under VALU load = d_out3[0] / d_out3[1] x *wall_clock_khz.  bench.py reports it beside the headline, so that a box
 * that ran at a lower clock says so (two boxes of the pool differed by 8 % on identical code in round 4).  d_sink: one float. */
int r3dg_clock_probe(void* stream, int iters, unsigned long long* d_out3, float* d_sink, int* wall_clock_khz);

/* The first step of r3dg_shade_frs_forward on its own: d_cprime [P,48] = the incident-light coefficients rotated into each
 * Gaussian's ray frame.  It depends on d_incidents and d_ray_normals only, so a caller can queue it (on another stream) as soon
 * as the coefficients are final and pass R3DG_SHADE_ROTATED to the forward. */
int r3dg_shade_frs_rotate(void* stream, int P, const float* d_incidents, const float* d_ray_normals, float* d_cprime);
int r3dg_shade_frs_forward(void* stream, int P, int K, const float* d_base_color, const float* d_roughness,
                           const float* d_normals, const float* d_viewdirs, const float* d_incidents, const float* d_env,
                           int He, int We, const float* d_visibility, float uniform_area, const uint32_t* d_taps,
                           const float* d_ray_normals, const float* d_zsamples, const float* d_tables,
                           const uint8_t* d_valid, const int32_t* d_invalid_list, int n_invalid, float* d_cprime, int flags,
                           float* d_out, void* listed_stream, float* d_feature_rows);
/*   listed_stream: NULL, or a second stream for the kernel on the listed Gaussians (ordered after everything queued on
 *   `stream` before the call; it then runs beside the rotation and the main kernel).  The caller joins listed_stream before anything
 *   reads d_out.
 *   d_feature_rows: NULL, or the rasterizer's [P,16] feature rows (neilf.py:115-122): the kernels then ALSO write pbr, diffuse
 *   light and mean visibility into columns 2..4, 12..14, 15 of each row -- with r3dg_stage2_activate(..., d_features) writing the
 *   other nine columns this replaces r3dg_stage2_pack_features (one launch and one pass over d_out less between the shading
 *   integral and the rasterizer; the light-smoothness sum then comes from r3dg_stage2_unpack_gradients). */
int r3dg_shade_frs_backward(void* stream, int P, int K, const float* d_base_color, const float* d_roughness,
                            const float* d_normals, const float* d_viewdirs, const float* d_incidents, const float* d_env,
                            int He, int We, const float* d_visibility, float uniform_area, const uint32_t* d_taps,
                            const float* d_ray_normals, const float* d_zsamples, const float* d_tables,
                            const uint8_t* d_valid, const int32_t* d_invalid_list, int n_invalid, const float* d_cprime,
                            float* d_dcprime, const float* d_dL_dpbr, const float* d_dL_ddiffuse_light,
                            float* d_dL_dbase_color, float* d_dL_droughness, float* d_dL_dviewdirs, float* d_dL_dincidents,
                            float* d_dL_denv, const float* d_block_absmax, int n_block_absmax, void* rotate_stream);
/* rotate_stream == R3DG_SHADE_NO_ROTATION_BACK: r3dg_shade_frs_backward leaves the coefficient gradient in the rotated frame
 * (d_dcprime) and does NOT write d_dL_dincidents for the Gaussians on the rotated path; the caller follows with
 * r3dg_shade_frs_incident_chain -- ONE pass per Gaussian that rotates the gradient back (writing d_dL_dincidents), applies the
 * Adam update of the incident-light group (the arithmetic of r3dg_adam_step for ONE group of [P,16,3] rows: columns 0..2 with
 * `lr`, the rest with `lr_tail`; `step` counts from 1; d_skip_flag as there) and rotates the NEW coefficients into the ray frames
 * (d_cprime, what r3dg_shade_frs_rotate would produce): 1536 instead of 2112 bytes per Gaussian and one launch instead of
 * three at the end of a whole training iteration (fused_step.py, "incident-light chain").
 * listed_rows_in_dcprime != 0: the world-frame gradient rows of the Gaussians OFF the rotated path (d_valid[g] == 0) are read from
 * their rows of d_dcprime instead of d_dL_dincidents -- for a caller that handed d_dcprime to r3dg_shade_frs_backward as
 * d_dL_dincidents too, so that ONE [P,48] buffer holds the whole coefficient gradient (rotated frame on the rotated path, world
 * frame off it) and can be summed over ranks as it is: the rotation is linear and the same on every rank (data-parallel
 * iterations, round 6: grad_scale = 1 / world).  The last argument is a set of R3DG_CHAIN_* bits; LISTED_ROWS_IN_DCPRIME is 1,
 * what callers passed for "true" before there were two.
 * R3DG_CHAIN_NO_GRADIENT_OUT: the world-frame gradient row is NOT written to d_dL_dincidents (192 of the pass's 1728 bytes per
 * Gaussian) -- for a caller whose gradient has no reader behind the update, e.g. a whole single-GPU iteration.  Parameters,
 * moments and d_cprime are bit for bit the same; d_dL_dincidents is then only READ, on the rows of the Gaussians off the
 * rotated path (unless those are in d_dcprime), and keeps whatever it held everywhere else. */
#define R3DG_SHADE_NO_ROTATION_BACK ((void*)(intptr_t)-1)
#define R3DG_CHAIN_LISTED_ROWS_IN_DCPRIME 1
#define R3DG_CHAIN_NO_GRADIENT_OUT 2
int r3dg_shade_frs_incident_chain(void* stream, int P, const float* d_ray_normals, const uint8_t* d_valid,
                                  const float* d_dcprime, float* d_dL_dincidents, float* d_incidents, float* d_exp_avg,
                                  float* d_exp_avg_sq, float* d_cprime, float lr, float lr_tail, float beta1, float beta2,
                                  float eps, int step, float grad_scale, const float* d_skip_flag, int chain_flags);
/*   Launch order on `stream`: the kernel on the listed Gaussians, then the main kernel (a caller that has other work
 *   running on another stream when it calls this gets the small launch beside that work).
 *   rotate_stream: NULL, or a second stream for the rotation of the coefficient gradient back to d_dL_dincidents (ordered after the
 *   main kernel by an event; it overlaps the caller's next launches on `stream`).  The caller joins rotate_stream before anything
 *   reads d_dL_dincidents. */

int r3dg_shade_backward(void* stream, int P, int K, int M, const float* d_base_color, const float* d_roughness,
                        const float* d_normals, const float* d_viewdirs, const float* d_incidents, const float* d_env,
                        int He, int We, const float* d_env_transform, const float* d_visibility,
                        const float* d_incident_dirs, const float* d_incident_areas, const float* d_dL_dpbr,
                        const float* d_dL_ddiffuse_light, float* d_dL_dbase_color, float* d_dL_droughness,
                        float* d_dL_dviewdirs, float* d_dL_dincidents, float* d_dL_denv);

/* r3dg_shade_backward with the cached lookup records of r3dg_shade_build_taps (lookup mode, NOT radiance: the texture's
 * gradient needs the texel indices); d_taps == NULL = r3dg_shade_backward.
 * d_block_absmax (may be NULL) / n_block_absmax: non-negative floats whose maximum is max(|dL_dpbr|, |dL_ddiffuse_light|)
 * over all elements, +inf if any element is not finite -- the scale of the texture gradient's fixed-point accumulation.
 * r3dg_stage2_unpack_gradients writes them as it produces the two gradients; NULL: reduced here by an extra pass. */
int r3dg_shade_backward_cached(void* stream, int P, int K, int M, const float* d_base_color, const float* d_roughness,
                               const float* d_normals, const float* d_viewdirs, const float* d_incidents,
                               const float* d_env, int He, int We, const float* d_env_transform,
                               const float* d_visibility, const float* d_incident_dirs, const float* d_incident_areas,
                               const uint32_t* d_taps, const float* d_dL_dpbr, const float* d_dL_ddiffuse_light,
                               float* d_dL_dbase_color, float* d_dL_droughness, float* d_dL_dviewdirs,
                               float* d_dL_dincidents, float* d_dL_denv, const float* d_block_absmax,
                               int n_block_absmax);

/* The reference's render_equation.{cu,h} contract model (render_equation.h:7-46): metallic BRDF with a spherical-
 * Gaussian D, SH environment light direct_shs[Sd,3] (+0.5), SH visibility visibility_shs[P,Sv] (+0.5, clamped), SH local
 * light incidents_shs[P,Si,3]; rays are the Fibonacci set rotated to the normal (no 10-degree floor), optionally with
 * a per-sample random angle rand_float[P,K] in [0,1) (is_training; NULL otherwise).  Backward: dL_dbase_color[P,3],
 * dL_droughness[P], dL_dmetallic[P], dL_dnormals[P,3], dL_dviewdirs[P,3], dL_dincidents_shs[P,Si,3],
 * dL_dvisibility_shs[P,Sv] are overwritten, dL_ddirect_shs[Sd,3] is ACCUMULATED (zero it first).  The backward keeps
 * the reference's quirks Q1-Q4 (see oracle/shading_oracle.c) and replaces its race on dL_ddirect_shs by the sum. */
int r3dg_render_equation_forward(void* stream, int P, int Si, int Sd, int Sv, const float* d_base_color,
                                 const float* d_roughness, const float* d_metallic, const float* d_normals,
                                 const float* d_viewdirs, const float* d_incidents_shs, const float* d_direct_shs,
                                 const float* d_visibility_shs, int sample_num, const float* d_rand_float,
                                 float* d_incident_dirs, float* d_pbr, float* d_diffuse_light);
int r3dg_render_equation_forward_complex(void* stream, int P, int Si, int Sd, int Sv, const float* d_base_color,
                                         const float* d_roughness, const float* d_metallic, const float* d_normals,
                                         const float* d_viewdirs, const float* d_incidents_shs,
                                         const float* d_direct_shs, const float* d_visibility_shs, int sample_num,
                                         float* d_incident_dirs, float* d_pbr, float* d_incident_lights,
                                         float* d_local_incident_lights, float* d_global_incident_lights,
                                         float* d_incident_visibility, float* d_diffuse_light,
                                         float* d_local_diffuse_light, float* d_accum, float* d_rgb_d, float* d_rgb_s);
int r3dg_render_equation_backward(void* stream, int P, int Si, int Sd, int Sv, const float* d_base_color,
                                  const float* d_roughness, const float* d_metallic, const float* d_normals,
                                  const float* d_viewdirs, const float* d_incidents_shs, const float* d_direct_shs,
                                  const float* d_visibility_shs, int sample_num, const float* d_incident_dirs,
                                  const float* d_dL_dpbr, const float* d_dL_ddiffuse_light, float* d_dL_dbase_color,
                                  float* d_dL_droughness, float* d_dL_dmetallic, float* d_dL_dnormals,
                                  float* d_dL_dviewdirs, float* d_dL_dincidents_shs, float* d_dL_ddirect_shs,
                                  float* d_dL_dvisibility_shs);

/* Scalar accumulators ("sum" arguments of r3dg_stage2_pack_features, r3dg_stage2_loss, r3dg_stage1_loss, r3dg_ssim_forward,
 * r3dg_stage2_env_backward): every quantity is R3DG_SUM_SLOTS consecutive floats and its value is the SUM of them -- each
 * workgroup adds its total to one slot (same-address float atomics serialise at ~35 ns each on MI355X; thousands of
 * workgroups on one word take longer than the kernels themselves).  `d_sums` arrays hold quantity q at
 * d_sums + q * R3DG_SUM_SLOTS.  Callers zero them before the first kernel of an iteration. */
#define R3DG_SUM_SLOTS 32

/* ---- Stage-2 iteration glue: the elementwise code around the hot ops, fused -------------------
 * All tensors fp32, device, contiguous.  Shapes: xyz/scaling/normal/base_color raw [P,3], rotation raw [P,4],
 * opacity/roughness raw [P]; viewmatrix = world_view_transform (16 floats, row-vector convention, scene/cameras.py:62),
 * campos[3]; features [P,16]; shade_out [P,19] (r3dg_shade_forward).
 * r3dg_stage2_activate: GaussianModel.get_scaling/get_rotation/get_opacity/get_normal/get_base_color/get_roughness
 *   (scene/gaussian_model.py:183-232; exp, F.normalize, sigmoid, 0.03+0.77s, 0.09+0.9s) and
 *   viewdirs = normalize(campos - xyz) (gaussian_renderer/neilf.py:74-76).  base_raw == NULL skips the stage-2 outputs.
 *   d_features (may be NULL; needs d_viewmatrix and the stage-2 inputs): the columns of the feature row that do not depend on
 *   the shading integral are written here -- depth, depth^2 (0, 1), normal (5..7), base colour (8..10), roughness (11).
 * r3dg_stage2_pack_features: the S=16 feature row of neilf.py:115-122 = depth, depth^2, pbr, normal, base_color,
 *   roughness, diffuse_light, mean visibility; *light_l1_sum (may be NULL) += sum_p sum_c |diffuse_c - mean_c diffuse|
 *   (light-smoothness term, neilf.py:286-292).
 * r3dg_stage2_unpack_gradients: dL_dfeatures[P,16] -> the shading op's upstream gradients dL_dpbr[P,3] and
 *   dL_ddiffuse_light[P,3], the latter including light_weight * d(sum_c |diffuse_c - mean|)/d diffuse;
 *   d_block_absmax (may be NULL): [ceil(P/256)] floats, max |.| of the rows written by each block (+inf: not finite),
 *   for r3dg_shade_backward_cached.  d_light_l1_sum (may be NULL): += sum_p sum_c |diffuse_c - mean_c diffuse|, the term's
 *   value, for callers that did not run r3dg_stage2_pack_features (which adds the same sum).
 * r3dg_stage2_activate_backward: chain rule of every activation above; combines the rasterizer's dL_dscales, dL_drot,
 *   dL_dopacity, dL_dmeans3D, dL_dfeatures and the shading op's dL_dbase_color, dL_droughness, dL_dviewdirs into the
 *   raw-parameter gradients (all seven outputs fully written).  d_g_xyz == NULL = frozen geometry (run_syn4.sh / run_dtu.sh:
 *   learning rate 0 on everything but the PBR groups): only d_g_base / d_g_rough are written, from d_dL_dfeatures and the
 *   shading op's two gradients; the geometry inputs and outputs are not touched and may be NULL.
 * r3dg_stage2_loss: image-space terms of calculate_loss (neilf.py:212-318) and their gradients in one pass:
 *   sums[0] += sum |image - gt|, sums[1] += sum |srgb(pbr_img) - gt|, sums[2] += sum m^2 (normal_render - pseudo_normal)^2
 *   (m = d_image_mask [HW], the view's object mask of neilf.py:258-264; NULL = all ones)
 *   with feat = feature / max(opacity,1e-5) * (n_contrib > 0), pbr_img = feat[2:5]*opacity + (1-opacity)*bg;
 *   dL_dimage[3,HW], dL_dopacity[HW], dL_dfeature[16,HW] are fully written for weights w_* per element;
 *   d_extra_dL_dimage / d_extra_dL_dsrgb (may be NULL): gradients of further terms w.r.t. the image and the sRGB PBR
 *   image (the SSIM terms), added before the chain rule.  sparse_feature_gradients != 0: only the maps that carry a loss
 *   term are written (channels 2-4, and 5-7 when w_normal != 0; the others are left untouched and, with w_normal == 0,
 *   the normal maps are not read and sums[2] is not accumulated) -- for a rasterizer backward restricted to those
 *   channels (active_features). */
int r3dg_stage2_activate(void* stream, int P, const float* d_xyz, const float* d_scaling_raw,
                         const float* d_rotation_raw, const float* d_opacity_raw, const float* d_normal_raw,
                         const float* d_base_raw, const float* d_rough_raw, const float* d_campos, float* d_scales,
                         float* d_rotations, float* d_opacity, float* d_normal, float* d_base_color,
                         float* d_roughness, float* d_viewdirs, const float* d_viewmatrix, float* d_features);
int r3dg_stage2_pack_features(void* stream, int P, const float* d_xyz, const float* d_viewmatrix, const float* d_normal,
                              const float* d_base_color, const float* d_roughness, const float* d_shade_out,
                              float* d_features, float* d_light_l1_sum);
int r3dg_stage2_unpack_gradients(void* stream, int P, const float* d_dL_dfeatures, const float* d_shade_out,
                                 float light_weight, float* d_dL_dpbr, float* d_dL_ddiffuse_light,
                                 float* d_block_absmax, float* d_light_l1_sum);
int r3dg_stage2_activate_backward(void* stream, int P, const float* d_xyz, const float* d_scaling_raw,
                                  const float* d_rotation_raw, const float* d_opacity_raw, const float* d_normal_raw,
                                  const float* d_base_raw, const float* d_rough_raw, const float* d_viewmatrix,
                                  const float* d_campos, const float* d_dL_dfeatures, const float* d_dL_dbase_color,
                                  const float* d_dL_droughness, const float* d_dL_dviewdirs, const float* d_dL_dscales,
                                  const float* d_dL_drotations, const float* d_dL_dopacity, const float* d_dL_dmeans3D,
                                  float* d_g_xyz, float* d_g_scaling, float* d_g_rotation, float* d_g_opacity,
                                  float* d_g_normal, float* d_g_base, float* d_g_rough);
int r3dg_stage2_loss(void* stream, int width, int height, const float* d_image, const float* d_opacity,
                     const float* d_feature, const float* d_pseudo_normal, const int32_t* d_n_contrib,
                     const float* d_gt, const float* d_background, const float* d_image_mask, float w_l1, float w_pbr,
                     float w_normal, const float* d_extra_dL_dimage, const float* d_extra_dL_dsrgb, float* d_dL_dimage,
                     float* d_dL_dopacity, float* d_dL_dfeature, float* d_sums,
                     int sparse_feature_gradients);
/* The three edge-aware smoothness terms of the Synthetic4Relight / DTU objective (neilf.py:275-292 with
 * script/run_syn4.sh:34-36 / run_dtu.sh:36-38; first_order_edge_aware_loss, utils/loss_utils.py:104-105 = kornia 0.6.12's
 * Sobel / 8 with replicate padding):
 *   w_base_color sum_{c,d} |G_d (base_color_c m)| exp(-|G_d gt_c|) + w_roughness sum_{c,d} |G_d (roughness m)| exp(-|G_d gt_c|)
 *   + w_light sum_{c,d} |G_d (diffuse_c m)| exp(-|G_d normal_c|)          (the guide of the light term is the RENDERED normal
 *   and carries a gradient), with X = feature_X / max(opacity, 1e-5) * (n_contrib > 0) on the S=16 training feature image --
 *   base_color and diffuse additionally through rgb_to_srgb with its clip to [0,1] (they are results["base_color"] /
 *   results["diffuse"], neilf.py:153-155; utils/graphics_utils.py:207-213), roughness and normal as rendered -- and
 *   m = d_image_mask [HW] (NULL = all ones).  The weights carry the 1 / (3 H W) of the reference's means; a zero weight
 *   switches its term off.
 * _forward: sums3[0..2] (R3DG_SUM_SLOTS floats each) += the three UNWEIGHTED sums; d_scratch [30 * H * W] floats receives
 *   what _backward needs.  _backward (after r3dg_stage2_loss, same images): d_dL_dopacity is ADDED to; of d_dL_dfeature
 *   [16,HW] the maps 8..10 / 11 / 12..14 of the active terms are written, and with the light term the normal maps 5..7 are
 *   written (accumulate_normal == 0) or added to (!= 0: r3dg_stage2_loss wrote them, w_normal != 0). */
int r3dg_stage2_smooth_forward(void* stream, int width, int height, const float* d_opacity, const float* d_feature,
                               const int32_t* d_n_contrib, const float* d_gt, const float* d_image_mask,
                               float w_base_color, float w_roughness, float w_light, float* d_scratch, float* d_sums3);
int r3dg_stage2_smooth_backward(void* stream, int width, int height, const float* d_opacity, const float* d_feature,
                                const int32_t* d_n_contrib, const float* d_image_mask, const float* d_scratch,
                                float w_base_color, float w_roughness, float w_light, int accumulate_normal,
                                float* d_dL_dopacity, float* d_dL_dfeature);
/* _forward + _backward as ONE kernel that streams the image through registers (lane = column, the wave walks down 60-column
 * strips; neighbours by DPP lane shifts; the divided maps, the stencil outputs and the adjoint inputs never exist in HBM or
 * LDS: no d_scratch): same arithmetic bit for bit, same outputs (d_sums3 += the three unweighted sums,
 * d_dL_dopacity added to, d_dL_dfeature maps written / added to as described above). */
int r3dg_stage2_smooth_fused(void* stream, int width, int height, const float* d_opacity, const float* d_feature,
                             const int32_t* d_n_contrib, const float* d_gt, const float* d_image_mask, float w_base_color,
                             float w_roughness, float w_light, int accumulate_normal, float* d_dL_dopacity,
                             float* d_dL_dfeature, float* d_sums3);
/* sRGB-mapped PBR image [3,HW] exactly as r3dg_stage2_loss forms it (input of the SSIM term on the PBR image). */
int r3dg_stage2_pbr_srgb(void* stream, int width, int height, const float* d_opacity, const float* d_feature,
                         const int32_t* d_n_contrib, const float* d_background, float* d_srgb);

/* Launches folded into their neighbours (round 5; each was 5-20 us alone on the iteration's critical stream):
 * r3dg_stage2_activate_with: r3dg_stage2_activate + two SIDE JOBS that ride as extra workgroups of the same launch:
 *   d_env[0..n_env) = softplus(d_env_raw[..]) (DirectLightMap.get_env, scene/direct_light_map.py:18-23; beta 1, threshold 20 as
 *   torch.nn.functional.softplus) and d_zero[0..n_zero) = 0 (the iteration's loss sums).  n_env == 0 / n_zero == 0: that job is
 *   skipped.
 * r3dg_stage2_activate_backward_with: r3dg_stage2_activate_backward + r3dg_stage2_env_backward (same arguments, same results)
 *   in one launch; He * We == 0: no texture job.
 * r3dg_stage2_normals_srgb: the rasterizer forward's surface-point + pseudo-normal pass (forward.cu:398-491; what
 *   r3dg_rasterize_forward computes when compute_pseudo_normal != 0 -- call the forward with 0 and this afterwards) and
 *   r3dg_stage2_pbr_srgb as one per-pixel kernel.  d_pseudo_normal, d_surface_xyz [3,HW] and d_srgb [3,HW] are fully written;
 *   tan_fovx/tan_fovy/cx/cy as passed to the forward. */
int r3dg_stage2_activate_with(void* stream, int P, const float* d_xyz, const float* d_scaling_raw,
                              const float* d_rotation_raw, const float* d_opacity_raw, const float* d_normal_raw,
                              const float* d_base_raw, const float* d_rough_raw, const float* d_campos, float* d_scales,
                              float* d_rotations, float* d_opacity, float* d_normal, float* d_base_color,
                              float* d_roughness, float* d_viewdirs, const float* d_viewmatrix, float* d_features,
                              int n_env, const float* d_env_raw, float* d_env, float* d_zero, int n_zero);
int r3dg_stage2_activate_backward_with(void* stream, int P, const float* d_xyz, const float* d_scaling_raw,
                                       const float* d_rotation_raw, const float* d_opacity_raw, const float* d_normal_raw,
                                       const float* d_base_raw, const float* d_rough_raw, const float* d_viewmatrix,
                                       const float* d_campos, const float* d_dL_dfeatures, const float* d_dL_dbase_color,
                                       const float* d_dL_droughness, const float* d_dL_dviewdirs, const float* d_dL_dscales,
                                       const float* d_dL_drot, const float* d_dL_dopacity, const float* d_dL_dmeans3D,
                                       float* d_g_xyz, float* d_g_scaling, float* d_g_rotation, float* d_g_opacity,
                                       float* d_g_normal, float* d_g_base, float* d_g_rough, int He, int We,
                                       const float* d_env_raw, const float* d_env, float* d_dL_denv, float w_tv,
                                       float* d_g_env_raw, float* d_tv_sum, int consume);
int r3dg_stage2_normals_srgb(void* stream, int width, int height, const float* d_viewmatrix, float tan_fovx, float tan_fovy,
                             float cx, float cy, const float* d_opacity, const float* d_depth, float* d_pseudo_normal,
                             float* d_surface_xyz, const float* d_feature, const int32_t* d_n_contrib,
                             const float* d_background, float* d_srgb);
/* The image-space tail of a stage-2 iteration in ONE launch: r3dg_stage2_normals_srgb, r3dg_ssim_forward_pair,
 * r3dg_ssim_backward_pair (scales scale_image / scale_pbr) and r3dg_stage2_loss with sparse_feature_gradients != 0 and the two
 * SSIM gradients as its extras -- same inputs, same outputs, same sums (d_sums[0..2], d_ssim_sum_image, d_ssim_sum_pbr), the
 * same per-pixel arithmetic -- without their intermediates: the sRGB PBR image, the SSIM partials and the SSIM gradients are
 * never stored.  d_pseudo_normal / d_surface_xyz [3,HW] are fully written; d_dL_dimage [3,HW], d_dL_dopacity [HW] and of
 * d_dL_dfeature [16,HW] the maps 2-4 (5-7 too when w_normal != 0) are written, the other maps are left untouched; with
 * w_normal == 0 the normal maps and d_image_mask are not read and d_sums[2] is not accumulated.  d_image_mask may be NULL.
 * r3dg_stage2_image_tail_supported: 1 where the kernel applies (callers fall back to the four calls elsewhere). */
int r3dg_stage2_image_tail_supported(int width, int height);
int r3dg_stage2_image_tail(void* stream, int width, int height, const float* d_viewmatrix, float tan_fovx, float tan_fovy,
                           float cx, float cy, const float* d_image, const float* d_opacity, const float* d_depth,
                           const float* d_feature, const int32_t* d_n_contrib, const float* d_gt, const float* d_background,
                           const float* d_image_mask, float w_l1, float w_pbr, float w_normal, float scale_image,
                           float scale_pbr, float* d_pseudo_normal, float* d_surface_xyz, float* d_dL_dimage,
                           float* d_dL_dopacity, float* d_dL_dfeature, float* d_sums, float* d_ssim_sum_image,
                           float* d_ssim_sum_pbr);

/* SSIM (utils/loss_utils.py:20-63: 11x11 Gaussian window, sigma 1.5, zero padding) of x against y, both [C,H,W].
 * _forward: *d_sum += sum of the SSIM map (divide by C*H*W for the reference's mean); d_partials [C,3,H,W] receives the
 * per-pixel partial derivatives the backward needs.  _backward: d_grad_x [C,H,W] = scale * d(sum SSIM)/dx (overwritten);
 * scale = -lambda_dssim / (C*H*W) for the loss term lambda_dssim * (1 - ssim). */
int r3dg_ssim_forward(void* stream, int width, int height, int channels, const float* d_x, const float* d_y,
                      float* d_partials, float* d_sum);
int r3dg_ssim_backward(void* stream, int width, int height, int channels, const float* d_x, const float* d_y,
                       const float* d_partials, float scale, float* d_grad_x);
/* The same for TWO images against one target in one launch each (the SH image and the sRGB PBR image of a stage-2
 * iteration, neilf.py:225-239): image 1 is optional (d_x1 NULL = the single-image call). */
int r3dg_ssim_forward_pair(void* stream, int width, int height, int channels, const float* d_x0, const float* d_x1,
                           const float* d_y, float* d_partials0, float* d_partials1, float* d_sum0, float* d_sum1);
int r3dg_ssim_backward_pair(void* stream, int width, int height, int channels, const float* d_x0, const float* d_x1,
                            const float* d_y, const float* d_partials0, const float* d_partials1, float scale0,
                            float scale1, float* d_grad_x0, float* d_grad_x1);

/* Stage-1 counterparts (plain 3DGS + normals, gaussian_renderer/render.py:15-130; r3dg_stage2_activate with
 * d_base_raw == NULL provides the activations): features [P,5] = normal(3), depth, depth^2.
 * r3dg_stage1_loss = the image-space terms of calculate_loss (gaussian_renderer/render.py:137-223) that script/run_nerf.sh:7-14
 * enables, values AND gradients in one call, with [normal, depth, depth2] = feature / max(opacity,1e-5) * (n_contrib > 0):
 *   w_l1 sum|image-gt| + w_mask_entropy sum -(m log o + (1-m) log(1-o)), o = clamp(opacity,1e-6,1-1e-6)      (:156-160)
 *   + w_normal sum (m normal - m pseudo_normal)^2                                                              (:162-167)
 *   + w_normal_smooth sum_{c,d} |G_d normal_c| exp(-|G_d gt_c|), G = 3x3 Sobel / 8, replicate padding (kornia 0.6.12
 *     spatial_gradient, utils/loss_utils.py:104-105)                                                           (:169-173)
 *   + w_depth_var sum sqrt(max(depth2 - depth^2, 1e-6))                                                        (:199-205)
 * d_image_mask [HW] may be NULL (all ones); d_edge_scratch [6*HW] floats is required when w_normal_smooth != 0;
 * d_extra_dL_dimage (may be NULL) is added to dL_dimage (the SSIM gradient).  The weights carry the 1/count of the
 * reference's means.  sums[0] += L1 sum, [1] += normal sum, [2] += entropy sum, [4] += edge-aware sum, [5] += sqrt-variance
 * sum (slot 3 is left to r3dg_ssim_forward); dL_dfeature is [5,HW]. */
int r3dg_stage1_pack_features(void* stream, int P, const float* d_xyz, const float* d_viewmatrix, const float* d_normal,
                              float* d_features);
int r3dg_stage1_loss(void* stream, int width, int height, const float* d_image, const float* d_opacity,
                     const float* d_feature, const float* d_pseudo_normal, const int32_t* d_n_contrib, const float* d_gt,
                     const float* d_image_mask, float w_l1, float w_mask_entropy, float w_normal, float w_normal_smooth,
                     float w_depth_var, const float* d_extra_dL_dimage, float* d_edge_scratch, float* d_dL_dimage,
                     float* d_dL_dopacity, float* d_dL_dfeature, float* d_sums);
int r3dg_stage1_activate_backward(void* stream, int P, const float* d_xyz, const float* d_scaling_raw,
                                  const float* d_rotation_raw, const float* d_opacity_raw, const float* d_normal_raw,
                                  const float* d_viewmatrix, const float* d_dL_dfeatures, const float* d_dL_dscales,
                                  const float* d_dL_drotations, const float* d_dL_dopacity, const float* d_dL_dmeans3D,
                                  float* d_g_xyz, float* d_g_scaling, float* d_g_rotation, float* d_g_opacity,
                                  float* d_g_normal);

/* Loss terms of the reference's OptimizationParams that no run script switches on (csrc/supervision.hip): the MVS depth / normal
 * supervision of stage 2 and the depth-smoothness and per-Gaussian terms of stage 1.  All maps [C,H,W] fp32; throughout
 * X = feature_X / max(opacity, 1e-5) * (n_contrib > 0) with the quotient rule and clamp convention of r3dg_stage2_loss's normal
 * term.  Each call ADDS to gradient buffers the existing kernels wrote and runs behind them; a zero weight switches its term
 * off, and with every weight zero the call returns without a launch.
 * r3dg_supervision_count: *d_count (one uint32, WRITTEN) = number of pixels with (image_mask != 0) == (gt_depth > 0), the
 *   ~sur_mask of neilf.py:243-247; d_gt_depth [HW], d_image_mask [HW] (NULL = all ones).  Integer adds only: the same bits on
 *   every run.  Depends on the view alone, not on the render.
 * r3dg_stage2_supervision: the two image-space terms of neilf.py:241-249 and :266-273 on the S=16 training feature image:
 *     w_depth / count * sum_sel |depth - gt_depth|          depth = map 0, sel as counted above, count = *d_count
 *   + w_normal_mvs * sum_c (normal_c dm - mvs_normal_c dm)^2   normal = maps 5..7, dm = (gt_depth > 0); the weight carries the
 *                                                              1 / (3 H W) of F.mse_loss
 *   sign(0) = 0 as in PyTorch's L1 backward.  count == 0: the depth term is zero in value and gradient (PyTorch returns NaN, the
 *   mean over nothing: the one deliberate difference).  d_mvs_normal [3,HW] (may be NULL when w_normal_mvs == 0), d_count (may
 *   be NULL when w_depth == 0).  d_dL_dopacity [HW] is ADDED to; of d_dL_dfeature [16,HW] map 0 is WRITTEN (w_depth != 0) and
 *   maps 5..7 (w_normal_mvs != 0) are written (accumulate_normal == 0) or added to (!= 0: an earlier kernel wrote them), as
 *   r3dg_stage2_smooth_fused does; d_sums2[0] += sum_sel |depth - gt_depth|, d_sums2[1] += the squared-difference sum (two
 *   quantities of R3DG_SUM_SLOTS floats, unweighted).
 * r3dg_stage1_depth_smooth: lambda_depth_smooth * first_order_edge_aware_loss(depth, gt) (render.py:175-179), depth = map 3 of
 *   the S=5 image, Sobel / 8 with replicate padding as the normal-smoothness term of r3dg_stage1_loss; the weight carries the
 *   1 / (3 H W).  Call after r3dg_stage1_loss: map 3 of d_dL_dfeature [5,HW] and d_dL_dopacity are ADDED to; d_edge_scratch
 *   [2*HW] floats; *d_sum (R3DG_SUM_SLOTS floats) += the unweighted sum.
 * r3dg_stage1_gaussian_terms: the per-Gaussian terms of render.py:181-197 and :215-219, each weight carrying the 1 / P:
 *     w_point_entropy sum_p w_p (-o log(o + 1e-10) - (1 - o) log(1 - o + 1e-10))
 *   + w_orientation   sum_p min(w_p, 1) max(n_p . d_p, 0),  d = normalize(xyz - campos)   (the caller gates it on the iteration)
 *   + w_scaling       sum_p sum_axis |s - mean_axis s|                                    (the caller applies the schedule)
 *   d_weights [P] = the rasterizer's blend weights (a constant), d_opacity [P], d_normal [P,3], d_scales [P,3]: ACTIVATED values.
 *   Call between the rasterizer backward and r3dg_stage1_activate_backward; ADDED to: d_dL_dopacity [P], d_dL_dscales [P,3],
 *   d_dL_dmeans3D [P,3] (orientation, through d) and columns 0..2 of d_dL_dfeatures [P,5] (orientation: the feature row's normal
 *   columns are the activated normal).  d_sums3[0..2] += the three unweighted sums (R3DG_SUM_SLOTS floats each; one add per
 *   wave).  Buffers of a term whose weight is zero may be NULL. */
int r3dg_supervision_count(void* stream, int width, int height, const float* d_gt_depth, const float* d_image_mask,
                           uint32_t* d_count);
int r3dg_stage2_supervision(void* stream, int width, int height, const float* d_opacity, const float* d_feature,
                            const int32_t* d_n_contrib, const float* d_gt_depth, const float* d_mvs_normal,
                            const float* d_image_mask, const uint32_t* d_count, float w_depth, float w_normal_mvs,
                            int accumulate_normal, float* d_dL_dopacity, float* d_dL_dfeature, float* d_sums2);
int r3dg_stage1_depth_smooth(void* stream, int width, int height, const float* d_opacity, const float* d_feature,
                             const int32_t* d_n_contrib, const float* d_gt, float w_depth_smooth, float* d_edge_scratch,
                             float* d_dL_dopacity, float* d_dL_dfeature, float* d_sum);
int r3dg_stage1_gaussian_terms(void* stream, int P, const float* d_weights, const float* d_opacity, const float* d_normal,
                               const float* d_scales, const float* d_xyz, const float* d_campos, float w_point_entropy,
                               float w_orientation, float w_scaling, float* d_dL_dopacity, float* d_dL_dfeatures,
                               float* d_dL_dscales, float* d_dL_dmeans3D, float* d_sums3);

/* Learnable environment texture (DirectLightMap, scene/direct_light_map.py:18-27): env = softplus(raw), [He,We,3].
 * g_raw = (dL_denv + w_tv * dTV(env)/denv) * softplus'(raw) with TV = mean (d/dh)^2 + mean (d/dw)^2 (tv_loss, utils/loss_utils.py:113-117: the env-smoothness term,
 * neilf.py:294-300); *tv_sum (may be NULL) += TV(env).  consume != 0: dL_denv is zeroed after it was read, so the
 * buffer can be handed to the next r3dg_shade_backward (which accumulates into it) without a fill. */
int r3dg_stage2_env_backward(void* stream, int He, int We, const float* d_raw, const float* d_env, float* d_dL_denv,
                             float w_tv, float* d_g_raw, float* d_tv_sum, int consume);

/* Adam over up to R3DG_ADAM_MAX_GROUPS parameter groups in ONE launch (torch.optim.Adam semantics, no weight decay /
 * amsgrad; GaussianModel.training_setup + step, scene/gaussian_model.py:465-497).  Elements whose index modulo `period`
 * is >= `split` use lr_tail (period 0: one rate) -- e.g. a [P,16,3] SH tensor with period 48, split 3 carries the
 * features_dc / features_rest rates.  `step` is the 1-based step count for the bias corrections; every gradient is
 * multiplied by `grad_scale` first (1/world_size after a sum all-reduce, 1 otherwise).  d_skip_flag (may be NULL): when the
 * float it points to is non-zero on the device the launch updates nothing (the overflow flag of a bounded forward). */
#define R3DG_ADAM_MAX_GROUPS 16
typedef struct r3dg_adam_group {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    uint64_t n;
    float lr, lr_tail;
    uint32_t period, split;
} r3dg_adam_group;
int r3dg_adam_step(void* stream, int n_groups, const r3dg_adam_group* groups, float beta1, float beta2, float eps,
                   int step, float grad_scale, const float* d_skip_flag);

/* ---- the backward, split over two streams; optionally with the SH group's Adam in it and the gradient records read in place ----
 * r3dg_rasterize_backward_split(stream, geometry_stream, scene, call, NULL, ..., NULL, NULL, NULL) is r3dg_rasterize_backward with
 * the per-Gaussian geometry backward (K12+K13) launched on `geometry_stream`, ordered after the tile kernel by an event, so work that
 * only needs the tile pass's FINAL outputs can follow on `stream` concurrently.  geometry_stream == stream is exactly
 * r3dg_rasterize_backward.
 *   final on `stream` (behind the tile kernel + its scatter pass):  d_dL_dfeature, d_dL_dopacity, d_dL_dcolor;
 *   valid ONLY AFTER JOINING geometry_stream:  d_dL_dmean3D, d_dL_dcov3D, d_dL_dsh, d_dL_dscale, d_dL_drot -- AND d_dL_dmean2D
 *     and d_dL_dconic: since round 5 the tile pass leaves RAW MOMENTS in those two (S_x, S_y / the second moments) and the
 *     per-Gaussian geometry kernel turns them into the viewspace gradient IN PLACE (rasterizer_preprocess_bwd.hip).  A consumer on
 *     `stream` that has not joined (e.g. densification statistics reading dL_dmeans2D) would read raw moments or race with that
 *     rewrite.  r3dg_stream_wait_stream(stream, geometry_stream) is the join.
 * Scratch: the tile pass adds into one gradient record per Gaussian, P x (16 or, with all S = 16 channels live, 32) floats of
 * LIBRARY scratch per (device, stream) that ever ran a backward -- 64 / 128 bytes per Gaussian (2M Gaussians: 128 / 256 MB),
 * grown geometrically and kept until r3dg_release_scratch().
 *
 * sh_adam != NULL (whole single-GPU training iterations; NULL: d_dL_dsh is written and the six arguments behind sh_adam are not
 * read): the geometry kernel applies the Adam step of the SH colour group ITSELF.  `sh_adam` describes the group -- param ==
 * d_shs ([P,M,3], n = 3 M P), both moments, lr / lr_tail / period / split as for r3dg_adam_step; its `grad` is not read -- and
 * step, betas, eps, grad_scale and d_skip_flag mean what they mean there.  The gradient rows, which that kernel holds in on-chip
 * memory, are consumed where they are: d_dL_dsh is NOT written (it may be NULL) and no r3dg_adam_step launch reads it and the
 * parameter row again -- per Gaussian 3 x 12 M bytes less through device memory and one launch less.  Parameters and moments come
 * out bit for bit as from the call with sh_adam == NULL followed by r3dg_adam_step on the one group (the same update statements,
 * compiled with the same flags); Gaussians outside the view take part with a zero gradient, as there; every other output is what
 * that call writes, also when *d_skip_flag != 0 (then parameters and moments are left untouched).  d_shs and the moments are final
 * only after joining geometry_stream.  Needs SH input (d_colors_precomp == NULL), 16-byte aligned arrays and
 * r3dg_rasterize_backward_sh_adam_supported(M) == 1 (M a multiple of 4 up to 16 while R3DG_OPT_STAGE_SH_ROWS is on);
 * R3DG_EINVAL otherwise -- there is no fallback.
 *
 * d_records_out != NULL (NULL: the three launches above, and layout_out and supported_out must be NULL too): the tile backward's
 * gradient records are read in place.  The classic call runs three launches: the tile kernel adds into one record per Gaussian, a
 * scatter pass copies the records into five arrays (and zeroes them), the geometry kernel reads three of the arrays.  In a whole
 * stage-2 iteration the other readers of the arrays -- r3dg_stage2_unpack_gradients and r3dg_stage2_activate_backward_with -- run
 * one thread per Gaussian too, so each of the three can read its Gaussian's record row itself and the scatter pass (at 300k
 * Gaussians 71 MB through device memory, alone on the critical path) is not needed.  The three outputs are reset first; then
 *   *supported_out = 1: the tile kernel has filled the records of `stream`, the geometry kernel has read them in place on
 *   geometry_stream, *d_records_out is the first of P rows and layout_out (R3DG_GRAD_RECORD_LAYOUT_INTS ints) describes them.  The
 *   four arrays only the scatter pass writes -- d_dL_dconic, d_dL_dopacity, d_dL_dcolor, d_dL_dfeature -- are neither read nor
 *   required; d_dL_dmean2D [P,3], an output of the op (required when P > 0), is written in full by the geometry kernel (valid
 *   after joining geometry_stream); every other output is bit for bit what the classic call writes.  The caller then OWES the rows
 *   their zeroing: r3dg_stage2_activate_backward_with_records on `stream` (behind the join with geometry_stream) or
 *   r3dg_gradient_records_scatter.  A backward on the same stream that finds the debt unpaid clears the whole buffer first, so an
 *   abandoned fill costs time, not correctness.
 *   *supported_out = 0 with R3DG_OK: nothing was enqueued -- P == 0, or the instance this call selects has no 16-float records (more
 *   than 7 active feature channels, or a depth gradient with more than 6); call again with d_records_out == NULL.
 *
 * A LAYOUT is R3DG_GRAD_RECORD_LAYOUT_INTS host ints that say which channel of a record holds what: the record width in floats |
 * colour r g b | S_x, S_y, depth side channel | S_xx, S_xy, S_yy, opacity | the channel of each of the 36 possible feature columns.
 * A channel of -1 means "not carried": the value is +0.f (the depth side channel of an instance without a depth gradient, a
 * feature column outside active_features).
 * r3dg_gradient_records_scatter: the scatter pass alone -- P rows of `layout` -> the five arrays of the classic call (every element
 *   written, as there), zeros -> the rows.  d_records may be a copy of the rows in the caller's memory.
 * r3dg_stage2_unpack_gradients_records, r3dg_stage2_activate_backward_with_records: those two calls with the rows (16-float
 *   records over S = 16 feature columns) in place of d_dL_dfeatures, and of d_dL_dopacity; same arithmetic, same results.  The
 *   second is the LAST reader: each thread writes its row back as zeros behind its loads.  Frozen geometry (d_g_xyz == NULL) has
 *   no records: R3DG_EINVAL. */
#define R3DG_GRAD_RECORD_LAYOUT_INTS 47
int r3dg_rasterize_backward_sh_adam_supported(int M);
int r3dg_rasterize_backward_split(void* stream, void* geometry_stream, const r3dg_raster_scene* scene,
                                  const r3dg_raster_backward* call, const r3dg_adam_group* sh_adam, float beta1, float beta2,
                                  float eps, int step, float grad_scale, const float* d_skip_flag, void** d_records_out,
                                  int* layout_out, int* supported_out);
int r3dg_gradient_records_scatter(void* stream, int P, int S, float* d_records, const int* layout, float* d_dL_dmean2D,
                                  float* d_dL_dconic, float* d_dL_dopacity, float* d_dL_dcolor, float* d_dL_dfeature);
int r3dg_stage2_unpack_gradients_records(void* stream, int P, const float* d_records, const int* layout,
                                         const float* d_shade_out, float light_weight, float* d_dL_dpbr,
                                         float* d_dL_ddiffuse_light, float* d_block_absmax, float* d_light_l1_sum);
int r3dg_stage2_activate_backward_with_records(void* stream, int P, const float* d_xyz, const float* d_scaling_raw,
                                               const float* d_rotation_raw, const float* d_opacity_raw,
                                               const float* d_normal_raw, const float* d_base_raw, const float* d_rough_raw,
                                               const float* d_viewmatrix, const float* d_campos, float* d_records,
                                               const int* layout, const float* d_dL_dbase_color,
                                               const float* d_dL_droughness, const float* d_dL_dviewdirs,
                                               const float* d_dL_dscales, const float* d_dL_drot, const float* d_dL_dmeans3D,
                                               float* d_g_xyz, float* d_g_scaling, float* d_g_rotation, float* d_g_opacity,
                                               float* d_g_normal, float* d_g_base, float* d_g_rough, int He, int We,
                                               const float* d_env_raw, const float* d_env, float* d_dL_denv, float w_tv,
                                               float* d_g_env_raw, float* d_tv_sum, int consume);

/* ---- relight / eval frame glue (relighting.py:114-170 -> gaussian_renderer/neilf.py:74-209 with is_training=False) -----
 * r3dg_relight_pack_features: the S=28 eval feature row (neilf.py:124-130) from the activated parameters and the 19
 *   outputs of r3dg_shade_forward: depth, depth^2, pbr3, normal3, base_color3, roughness, diffuse3, specular3, incident /
 *   local / global light means (3 each), mean visibility.  d_features [P,28] must be 16-byte aligned.
 * r3dg_relight_compose: per pixel the camera ray in world space (Camera.get_world_directions, scene/cameras.py:79-91;
 *   d_viewmatrix = world_view_transform, whose upper-left 3x3 is the camera-to-world rotation), the lat-long lookup of the
 *   HDR environment map d_envmap [He,We,3] (EnvLight.direct_light, scene/envmap.py:35-53; d_light_transform = row-major
 *   3x3 rotation applied as dirs @ T^T, or NULL) and the composites of neilf.py:203-207 -- any output may be NULL:
 *     d_pbr_env = srgb(pbr * opacity + (1 - opacity) * env), d_render_env = image + (1 - opacity) * srgb(env),
 *     d_env_only = srgb(env), all [3,H,W].  d_feature is the rasterizer's [S>=5,H,W] feature image (pbr in channels 2..4,
 *   un-normalised: it is divided by max(opacity, 1e-5) and masked by n_contrib > 0 here, neilf.py:146-147). */
int r3dg_relight_pack_features(void* stream, int P, const float* d_xyz, const float* d_viewmatrix, const float* d_normal,
                               const float* d_base_color, const float* d_roughness, const float* d_shade_out,
                               float* d_features);
int r3dg_relight_compose(void* stream, int width, int height, float focal_x, float focal_y, float cx, float cy,
                         const float* d_viewmatrix, const float* d_light_transform, const float* d_envmap, int He, int We,
                         const float* d_image, const float* d_opacity, const float* d_feature,
                         const int32_t* d_n_contrib, float* d_pbr_env, float* d_render_env, float* d_env_only);

/* ---- evaluation of held-out views (eval_nvs.py:49-82, eval_relighting_syn4.py:140-224; evaluate.py) ---------------------
 * r3dg_relight_capture: the capture maps of an eval frame (neilf.py:146-182, what --capture_list and the evaluation scripts
 *   read) from the rasterizer's raw S=28 feature image d_feature [28,H,W] (channel layout: r3dg_relight_pack_features),
 *   d_opacity [H,W] and d_n_contrib [H,W] in one pass: x = feature / max(opacity, 1e-5) * (n_contrib > 0);
 *     d_base_color, d_diffuse, d_specular, d_lights, d_local_lights, d_global_lights [3,H,W] = rgb_to_srgb(x) with its clip,
 *     d_normal [3,H,W], d_roughness, d_visibility [1,H,W] = x, d_depth_var [1,H,W] = depth2 - depth^2,
 *     d_pbr [3,H,W] = srgb(pbr * opacity + (1 - opacity) * background).
 *   Any output may be NULL (its channels are then not read).  d_background [3] is required by d_pbr and by d_mask; d_mask
 *   [H,W] (may be NULL): every map but d_depth_var is composited as map * mask + (1 - mask) * background
 *   (eval_relighting_syn4.py:161-167; one-channel maps take background[0], the normal is composited as rendered).
 * r3dg_eval_image_metrics: PSNR and SSIM of d_pred against d_gt, both [C,H,W] with 1 <= C <= 3.  With d_mask [H,W] both
 *   images are first composited as x * mask + fill * (1 - mask) (eval_relighting_syn4.py:161-186) while they are loaded --
 *   d_fill (may be NULL = 0) is a colour [C] (fill_is_image == 0) or an image [C,H,W] (!= 0, the env_only fill of :169,186).
 *   d_tile_sums: scratch, 2 * C * ceil(W/32) * ceil(H/32) doubles (one (squared error, SSIM sum) pair per workgroup of the
 *   SSIM tiling; added up in a fixed order by one workgroup: no float atomics, two runs give the same bits).  d_row
 *   (R3DG_EVAL_ROW doubles, one row of the caller's metrics table) receives [0..2] the per-channel mean squared error,
 *   [3] the sum of the SSIM map, [4] psnr = mean_c 20 log10(1 / sqrt(mse_c)) (utils/image_utils.py:24-29),
 *   [5] ssim = [3] / (C H W) (utils/loss_utils.py:39-63), [6] C.
 * r3dg_eval_median_ratio: the albedo scale of eval_relighting_syn4.py:201 -- per channel the LOWER median (index (n-1)/2 of
 *   the sorted values, as torch.median) of d_gt / clamp(d_pred, 1e-6, 1) over the n pixels with d_mask > 0 (NULL = all);
 *   images [3,H,W] with non-negative d_gt.  8-bit radix select on the float bit patterns, four passes, the digit picked on
 *   the device.  d_state: scratch, R3DG_EVAL_MEDIAN_STATE_WORDS uint32.  d_row (R3DG_EVAL_ROW doubles) receives [0..2] the
 *   medians and [3] n; n == 0 gives NaN medians and a count of 0.
 * None of the three synchronises or reads anything back; images of 2^31 pixels and more are rejected. */
#define R3DG_EVAL_ROW 8
#define R3DG_EVAL_MEDIAN_STATE_WORDS 1024
int r3dg_relight_capture(void* stream, int width, int height, const float* d_feature, const float* d_opacity,
                         const int32_t* d_n_contrib, const float* d_background, const float* d_mask, float* d_pbr,
                         float* d_base_color, float* d_roughness, float* d_normal, float* d_visibility, float* d_diffuse,
                         float* d_specular, float* d_lights, float* d_local_lights, float* d_global_lights,
                         float* d_depth_var);
int r3dg_eval_image_metrics(void* stream, int width, int height, int channels, const float* d_pred, const float* d_gt,
                            const float* d_mask, const float* d_fill, int fill_is_image, double* d_tile_sums,
                            double* d_row);
int r3dg_eval_median_ratio(void* stream, int width, int height, const float* d_pred, const float* d_gt,
                           const float* d_mask, uint32_t* d_state, double* d_row);

/* ---- scene assembly: PLY records <-> parameter groups, objects into a composite (relighting.py:28-52 scene_composition;
 *      scene/gaussian_model.py:507-665 save_ply / load_ply; ply.py, compose.py) ------------------------------------------------
 * A RECORD is one row of a reference PLY body: R3DG_SCENE_COLUMNS (130) floats in the order of construct_list_of_attributes
 *   (x y z, nx ny nz, f_dc_0..2, f_rest_0..44, opacity, scale_0..2, rot_0..3 -- the R3DG_SCENE_STAGE1_COLUMNS (62) a stage-1
 *   file ends with -- then base_color_0..2, roughness, incidents_dc_0..2, incidents_rest_0..44, visibility_dc_0,
 *   visibility_rest_0..14); *_rest columns are channel-major (f_rest_{c*15+i} is coefficient i+1 of channel c).
 * The GROUPS are the R3DG_SCENE_GROUPS (13) parameter tensors of a model, coefficient-major, in the order
 *   xyz [P,3], normal [P,3], features_dc [P,1,3], features_rest [P,15,3], opacity [P,1], scaling [P,3], rotation [P,4],
 *   base_color [P,3], roughness [P,1], incidents_dc [P,1,3], incidents_rest [P,15,3], visibility_dc [P,1,1],
 *   visibility_rest [P,15,1].  A group table is a HOST array of 13 device pointers in that order (`dst_groups`, `src_groups`).
 * r3dg_scene_place_records: rows [0,P) of d_records [P,A] (A floats per row, 62 <= A <= R3DG_SCENE_MAX_COLUMNS; 4-byte aligned
 *   is enough) are read through d_column_map (int32 [130]: the file column of every canonical slot, -1 = absent, read as 0) and
 *   written to rows [row_offset, row_offset + P) of the 13 destination tensors (all required), one launch: 64-row tiles staged
 *   through LDS, every access to device memory with consecutive lanes on consecutive floats.
 *   d_placement (may be NULL: a pure copy) is R3DG_SCENE_PLACEMENT_FLOATS floats describing the object's similarity transform
 *   T as relight.transform_object defines it: [0..11] the upper three rows of T, row-major 3x4; [12..14] the per-axis scale
 *   (row norms of T[:3,:3]); [15..23] R = T[:3,:3] / scale, row-major; [24..27] R's quaternion (w,x,y,z); [28..36], [37..61],
 *   [62..110] the band 1, 2, 3 SH rotation matrices, row-major (read only with R3DG_SCENE_ROTATE_SH).  Per row:
 *   xyz = T (x,1); scaling = log(exp(s) * scale); normal = R n; rotation = quaternion * rotation.
 *   flags: R3DG_SCENE_ZERO_INCIDENTS writes zeros to the placed rows of incidents_dc / incidents_rest (relighting.py:49-50);
 *   R3DG_SCENE_ROTATE_SH (needs d_placement) multiplies bands 1..3 of the colour, incident-light (unless zeroed) and visibility
 *   SH by the three matrices, c'_l = M_l c_l; without it coefficients are copied unchanged, as the reference does.
 * r3dg_scene_place_groups: the same with the 13 tensors of an in-memory model (P rows each) as the source; the six PBR
 *   entries of src_groups may ALL be NULL (a stage-1 model: read as 0).
 * r3dg_scene_pack_records: the inverse of the unpack -- src_groups (P rows) -> d_records [P,columns], columns 62 (the first
 *   seven groups are read) or 130.
 * Rows outside the placed range are not touched; nothing synchronises; no atomics. */
#define R3DG_SCENE_COLUMNS 130
#define R3DG_SCENE_STAGE1_COLUMNS 62
#define R3DG_SCENE_GROUPS 13
#define R3DG_SCENE_MAX_COLUMNS 250
#define R3DG_SCENE_PLACEMENT_FLOATS 111
#define R3DG_SCENE_ZERO_INCIDENTS 1
#define R3DG_SCENE_ROTATE_SH 2
int r3dg_scene_place_records(void* stream, int P, int A, const float* d_records, const int32_t* d_column_map,
                             const float* d_placement, int flags, long long row_offset, void** dst_groups);
int r3dg_scene_place_groups(void* stream, int P, void** src_groups, const float* d_placement, int flags,
                            long long row_offset, void** dst_groups);
int r3dg_scene_pack_records(void* stream, int P, int columns, void** src_groups, float* d_records);

/* r3dg_relight_quantize: a frame for an 8-bit image file, d_image [C,H,W] float -> d_bytes [H,W,C] uint8 (1 <= C <= 4) as
 *   torchvision's save_image quantises: clamp(x * 255 + 0.5, 0, 255) truncated, the product and the sum rounded separately.
 *   NaN quantises to 0.  The driver copies d_bytes asynchronously into its ring of pinned host buffers. */
int r3dg_relight_quantize(void* stream, int width, int height, int channels, const float* d_image, uint8_t* d_bytes);

/* r3dg_training_sheet: the contact sheet train.py:276-317 (save_training_vis) writes while a run trains, d_bytes
 *   [out_height,out_width,3] uint8, from the RAW outputs of one eval frame in one launch: d_render, d_gt, d_pseudo_normal [3,H,W],
 *   d_opacity [H,W], d_n_contrib [H,W], the rasterizer's un-normalised feature image d_feature [S,H,W].  layout 0: S = 5, channels
 *   normal3, depth, depth2 (render.py:91,111), 7 panels; layout 1: the S = 28 eval row of r3dg_relight_pack_features, 16 panels,
 *   with d_background [3] and the ACTIVATED environment texture d_env [env_rows,2 env_rows,3] (both read by layout 1 only and may
 *   be NULL for layout 0; every other pointer is required).  Per output byte, in this order: (1) the source of the nearest-
 *   neighbour resample of the grid to out_height x out_width, torch's rule src = min((int)floorf(dst * scale), in - 1), scale =
 *   (float)in / out; (2) the cell of torchvision's make_grid(nrow=4, padding=2, pad_value=0): panel k at y = (k / 4) * (H + 2)
 *   + 2, x = (k % 4) * (W + 2) + 2 of a grid of rows * (H + 2) + 2 by 4 * (W + 2) + 2, padding and cell 7 of the stage-1 grid 0;
 *   (3) that panel at that pixel, with x = feature / max(opacity, 1e-5) * (n_contrib > 0) as in r3dg_relight_capture:
 *     0 render, 1 gt, 2 visualize_depth(depth) (utils/image_utils.py:6-21 with its defaults: t = clip((-log(depth + eps) -
 *     c_far) / (c_near - c_far), 0, 1) in float32, NaN -> 0, bin min((int)(t * 256), 255) of matplotlib's `turbo` table),
 *     3 min((depth2 - depth^2) / 0.001, 1), 4 opacity, 5 normal * 0.5 + 0.5, 6 pseudo_normal * 0.5 + 0.5, 7 srgb(base_color),
 *     8 roughness, 9 visibility, 10 srgb(diffuse), 11 srgb(specular), 12 srgb(global_lights), 13 srgb(pbr * opacity + (1 -
 *     opacity) * background), 14 / 15 the left / right half of srgb(F.interpolate(env, (H, 2W))), nearest by the same rule;
 *   one-channel panels fill all three channels; srgb is rgb_to_srgb with its clip; (4) r3dg_relight_quantize's quantisation.
 *   The caller picks the size (training_vis.sheet_size: the reference's `scale = grid_h / 800`); any size of at least 1 x 1 is
 *   served.  d_bytes must be 4-byte aligned: a lane stores four consecutive bytes as one word (the last lane its own bytes
 *   only), the floats are read with 4-byte accesses at any 4-byte alignment, nothing outside the arrays is touched.  Nothing
 *   synchronises; no atomics.  layout outside {0, 1}, a NULL required pointer, and frames, sheets or grid sides of 2^31
 *   pixels and more are rejected. */
int r3dg_training_sheet(void* stream, int width, int height, int layout, const float* d_render, const float* d_gt,
                        const float* d_opacity, const int32_t* d_n_contrib, const float* d_feature,
                        const float* d_pseudo_normal, const float* d_background, const float* d_env, int env_rows,
                        int out_width, int out_height, uint8_t* d_bytes);

/* r3dg_png_encode: the zlib stream of the PNG file of d_bytes [H,W,C] uint8 (8 bits deep, colour type 0 / 4 / 2 / 6 for C = 1 / 2 /
 *   3 / 4, no interlace) -- the scanline filter, the deflate stream and the Adler-32 -- in three launches.  The host is left with the
 *   chunk framing and its CRC-32 (png_device.wrap).  The stream is cut so that a row segment is an independent unit of work:
 *   FILTER, per row, bpp = C: None, Sub, Up, Average (floor((a + b) / 2)), Paeth (standard predictor, tie order a, b, c); row 0
 *     sees a zero row above; the score of a candidate is sum |int8(byte)| over the row, the lowest wins, a tie goes to the lowest
 *     type.  The filtered stream is H rows of row_bytes = 1 + W * C bytes: the type, then the row.  The filter reads the pixel row
 *     above also across a segment boundary.
 *   SEGMENTS: rows_per_segment = max(1, min(H, 16384 / row_bytes)) rows; the last one may be shorter; at most 65535 raw bytes.
 *   PARSE: the segment's bytes, type bytes included, in maximal runs of equal bytes.  A run of n emits one literal, then rest =
 *     n - 1: while rest >= 261 or rest == 258 a match (258, distance 1); then rest of 259 / 260: a match of rest - 3 and one of 3;
 *     rest >= 3: a match of rest; else `rest` literals.  Distance 1 is the only distance.
 *   CODE: one dynamic-Huffman table for all segments, handed over as data.  d_code_table uint32[286]: bits 0..15 the canonical
 *     code of a literal/length symbol, bit-reversed for LSB-first packing, bits 16..20 its length (1..15).  d_block_header: the
 *     constant bits of a non-final BTYPE = 10 block header (BFINAL = 0, BTYPE, HLIT = 29, HDIST = 0, HCLEN, the code-length code,
 *     the 286 + 1 lengths), header_bits of them, LSB-first in ceil(header_bits / 8) bytes.  The one distance code has length 1 and
 *     code 0: a match is its length code, the extra bits, one 0 bit.  The caller vouches for the table (png_device.CodeTable.
 *     validate: lengths in 1..15, Kraft sum 1, a complete code-length code); the kernel reads it as it is.
 *   A CODED SEGMENT: the block header, the tokens, symbol 256, then an empty stored block (bits 000, zero bits to the byte
 *     boundary, 00 00 FF FF).  When that exceeds raw + 5 bytes the segment is ONE stored block instead: 00, LEN, ~LEN, the raw
 *     bytes.  The choice is made from the scanned bit total before anything is written.
 *   STREAM: 78 01, the segments, 03 00 (a final empty fixed block), Adler-32 of the filtered stream, big-endian; so
 *     *d_zlib_bytes <= 2 + sum(raw_seg + 5) + 6 = r3dg_png_zlib_bound.
 *   d_scratch: r3dg_png_scratch_bytes bytes at least, 16-byte aligned (a fixed slot per segment, its byte count and Adler pair
 *   (sum b, sum (n - i) b) mod 65521, the stream offsets); d_zlib: zlib_capacity >= the bound, any alignment, only the first
 *   *d_zlib_bytes bytes are written; d_bytes any alignment (byte loads); d_code_table and d_zlib_bytes 4-byte aligned.
 *   No global atomics, nothing synchronises, nothing outside the arrays is touched.  Rejected, with nothing enqueued: channels
 *   outside 1..4, row_bytes > 65535, header_bits outside 17..2048, a capacity or scratch below its size, a misaligned scratch, a
 *   NULL pointer, 2^31 pixels and more, a bound of 2^31 bytes and more (the length word is an int32).  The two size queries
 *   return R3DG_EINVAL (negative) for a shape the encoder rejects. */
long long r3dg_png_zlib_bound(int width, int height, int channels);
long long r3dg_png_scratch_bytes(int width, int height, int channels);
int r3dg_png_encode(void* stream, int width, int height, int channels, const uint8_t* d_bytes, const uint32_t* d_code_table,
                    const uint8_t* d_block_header, int header_bits, uint8_t* d_scratch, long long scratch_bytes,
                    uint8_t* d_zlib, long long zlib_capacity, int32_t* d_zlib_bytes);

/* r3dg_view_unpack: one ground-truth view of the device view store, d_pixels [H,W,C] uint8 as the image file holds them (C = 4:
 *   RGBA, C = 3: RGB) -> d_image [3,H,W] float composited onto d_background (3 floats on the device) and d_mask [1,H,W] float (the
 *   alpha channel; ones for C = 3; NULL: not wanted), bit for bit what the reference's reader makes of the file
 *   (scene/utils.py:47-48, dataset_readers.py:246-249, camera_utils.py:35,56, cameras.py:34): u = byte / 255 and a = alpha / 255 in
 *   float64, x = u * a + bg * (1 - a) in float64 with every operation rounded on its own, x rounded to float32 and clamped to
 *   [0,1]; mask = (float)a.  One launch, flat over the H*W pixels (a lane = 4 consecutive pixels: one 16-byte load, one 16-byte
 *   store per plane); pointers that are not 16-byte aligned (4-byte for RGB pixels) take narrower accesses; nothing outside the
 *   three arrays is read or written.  Nothing synchronises; no atomics.  Same size limits as r3dg_relight_quantize. */
int r3dg_view_unpack(void* stream, int width, int height, int channels, const uint8_t* d_pixels, const float* d_background,
                     float* d_image, float* d_mask);

/* r3dg_view_unpack_masked: the same for a view whose mask is a file of its own (the NeILF layout: scene/utils.py:52-57,
 *   dataset_readers.py:358-364): d_pixels [H,W,3] uint8 and d_mask_bytes [H,W] uint8 (the mask file as 8-bit grey) -> d_image
 *   [3,H,W] and d_mask [1,H,W] (NULL: not wanted).  m = (byte > 0) ? 1 : 0 (`mask[mask > 0.5] = 1` on the float of the byte),
 *   image = (float)((byte / 255 in float64) * m) clamped to [0,1], mask = m.  No background: the reader composites none for this
 *   layout.  One launch, a lane = 4 consecutive pixels (12 bytes of pixels and 4 mask bytes in, one 16-byte store per plane);
 *   misaligned pointers and the last lane take narrower accesses of their own bytes only.  Nothing synchronises; no atomics. */
int r3dg_view_unpack_masked(void* stream, int width, int height, const uint8_t* d_pixels, const uint8_t* d_mask_bytes,
                            float* d_image, float* d_mask);

/* r3dg_view_resize: a stored view at another resolution, as the reference's loadCam makes it (utils/camera_utils.py:13-58,
 *   scene/cameras.py:34): d_pixels [H,W,C] uint8 (C = 4: RGBA over d_background; C = 3: RGB, d_background not read) and
 *   d_mask_bytes [H,W] uint8 (C = 3 only; NULL: no mask file) -> d_image [3,out_height,out_width] and d_mask
 *   [1,out_height,out_width] (NULL: not wanted; all ones for RGB without a mask file).  Order: the composite of r3dg_view_unpack /
 *   r3dg_view_unpack_masked at full size rounded to float32, the separable antialiased bilinear filter of
 *   torch.nn.functional.interpolate(mode="bilinear", align_corners=False, antialias=True) with float64 weights and float32 sums,
 *   clamp to [0,1]; the mask by nearest neighbour from the full-size float mask, src = min(floor(dst * float32(in / out)), in - 1).
 *   1 <= in / out <= R3DG_VIEW_RESIZE_MAX_SCALE on both axes (no upscaling; the tap count is bounded); d_pixels and d_mask_bytes
 *   16-byte aligned; no byte outside the arrays is read.  One launch (64 x 8 output pixels per workgroup, both passes through
 *   LDS).  Nothing synchronises; no atomics.  Same size limits as r3dg_relight_quantize. */
#define R3DG_VIEW_RESIZE_MAX_SCALE 16
int r3dg_view_resize(void* stream, int width, int height, int channels, const uint8_t* d_pixels, const uint8_t* d_mask_bytes,
                     const float* d_background, int out_width, int out_height, float* d_image, float* d_mask);

/* r3dg_exr_unpack_chunks: the chunks of one OpenEXR scanline view (NONE / ZIPS / ZIP compression, HALF or FLOAT samples) after the
 *   host's zlib inflate -> the planar view d_planes [kept,height,width] in the file's own sample type (bytes_per_sample = 2: half
 *   bit patterns, 4: float bit patterns), never converted: bit for bit what exr.decode_reference makes of the file, NaN payloads
 *   and denormals included.  d_inflated: `inflated_bytes` bytes, every chunk at a 16-byte-aligned offset; d_chunk_table
 *   [chunks,4] int32 per chunk: byte offset into d_inflated, first row, row count, stored-raw flag (non-zero: the chunk was not
 *   compressed and carries no predictor and no byte split; every chunk of an uncompressed file).  A chunk holds `row count` rows
 *   of `file_channels` planes of `width` little-endian samples; d_kept_channels [kept] int32: the file-channel index of each
 *   output plane.  The device undoes the predictor (t[i] = t[i-1] + d[i] - 128 mod 256 over the whole chunk), the split (raw[2j]
 *   = t[j], raw[2j+1] = t[half+j]) and the row / channel planarisation, by a two-pass tile-sum scan: d_tile_sums (scratch, at
 *   least chunks * 2 * ceil(max_chunk_rows * width * file_channels * bytes_per_sample / 2 / R3DG_EXR_TILE) uint32,
 *   `tile_sums_count` of them offered) takes the byte sums of every tile in the first launch, the second scans, interleaves and
 *   stores.  max_chunk_rows: 16 for ZIP, 1 for ZIPS / NONE; a table row with more rows, with rows outside [0, height), with an
 *   offset off the 16-byte grid or with bytes outside d_inflated is SKIPPED (nothing is read or written for it); rows no chunk
 *   covers keep what d_planes held.  Two launches; nothing synchronises; no atomics. */
#define R3DG_EXR_TILE 4096
#define R3DG_EXR_MAX_KEPT 8
#define R3DG_EXR_MAX_TILES 32768
int r3dg_exr_unpack_chunks(void* stream, int width, int height, int file_channels, int bytes_per_sample, int chunks,
                           int max_chunk_rows, const uint8_t* d_inflated, long long inflated_bytes, const int32_t* d_chunk_table,
                           int kept, const int32_t* d_kept_channels, uint32_t* d_tile_sums, long long tile_sums_count,
                           void* d_planes);

/* r3dg_view_unpack_hdr: one resident HDR view of the device view store, d_view [3,H,W] planar R, G, B (is_half != 0: half, else
 *   float: what r3dg_exr_unpack_chunks wrote), d_mask_bytes [H,W] uint8 (the view's mask file as 8-bit grey; NULL: no mask file),
 *   d_background 3 floats -> d_image [3,H,W] float and d_mask [1,H,W] float (NULL: not wanted), as the reference's
 *   Synthetic4Relight reader makes them (scene/utils.py:40-46, dataset_readers.py:551-555, cameras.py:34): y = x > 0.0031308 ?
 *   pow(x, 1/2.4) * 1.055 - 0.055 : 12.92 * x in float32 with the constants rounded to float32 and every operation rounded on its
 *   own, m = byte > 0, image = m ? clamp(y, 0, 1) : background, mask = m.  Without d_mask_bytes the image alone and an all-ones
 *   mask.  A NaN sample stays NaN.  One launch, a lane = one pixel; nothing synchronises; no atomics.  Same size limits as
 *   r3dg_relight_quantize. */
int r3dg_view_unpack_hdr(void* stream, int width, int height, int is_half, const void* d_view, const uint8_t* d_mask_bytes,
                         const float* d_background, float* d_image, float* d_mask);

/* ---- densification bookkeeping -------------------------------------------------------------------
 * r3dg_densify_accumulate: GaussianModel.add_densification_stats (scene/gaussian_model.py:931-937) + the max-radii
 *   update of train.py:164-165, one pass.  The visibility filter is radii > 0 (render.py / neilf.py `visibility_filter`).
 *   d_viewspace_grad [P,3] is the gradient slot of the screen-space dummy (dL_dmeans2D); d_normal_grad [P,3] is the
 *   gradient of the raw normal parameter (NULL: the normal statistic is left alone); d_weights [P] are the rasterizer's
 *   per-Gaussian blend weights.  All five statistics are [P] floats updated in place.  d_skip_flag (may be NULL): a
 *   non-zero float on the device turns the call into a no-op (the overflow flag of a bounded forward). */
int r3dg_densify_accumulate(void* stream, int P, const float* d_viewspace_grad, const float* d_normal_grad,
                            const int32_t* d_radii, const float* d_weights, float* d_xyz_gradient_accum,
                            float* d_normal_gradient_accum, float* d_denom, float* d_weights_accum,
                            float* d_max_radii2D,
                            const float* d_skip_flag);

/* Thresholds of one densify_and_prune (mode 0, gaussian_model.py:893-915) or prune (mode 1, :917-929) call.  The
 * products the reference forms in Python doubles are passed already rounded to fp32:
 *   dense_size = percent_dense * scene_extent (:855, :804), world_size_limit = 0.1 * extent (:909),
 *   split_divisor = 0.8 * n_split (:814).  max_screen_size 0 = None (no screen / world size tests). */
typedef struct r3dg_densify_config {
    int32_t mode;
    int32_t n_split;
    float grad_threshold, grad_normal_threshold, min_opacity, weights_threshold;
    float dense_size, world_size_limit, split_divisor, max_screen_size;
} r3dg_densify_config;

/* r3dg_densify_plan: every decision of the call as ONE row map.  d_src_row / d_kind need max(2, n_split) * P entries;
 *   on return entries [0, d_counts[0]) hold, in the reference's output order (surviving originals, surviving clones,
 *   n_split blocks of surviving split children), the source row and its kind: -1 original (Adam moments travel with
 *   it), -2 clone (moments 0), k >= 0 split child that uses row k of the caller's standard-normal table
 *   [n_split * d_counts[3], 3] (row b * d_counts[3] + rank of the parent among ALL split Gaussians -- the row
 *   torch.normal would have filled, so the random stream is consumed exactly as in the reference).
 *   d_counts int32[8]: [0] rows out, [1] surviving originals, [2] surviving clones, [3] split Gaussians,
 *   [4] split Gaussians whose children survive.  d_temp: r3dg_densify_temp_bytes(P).  Statistics are [P] floats. */
size_t r3dg_densify_temp_bytes(int P);
int r3dg_densify_plan(void* stream, int P, const r3dg_densify_config* config, const float* d_scaling_raw,
                      const float* d_opacity_raw, const float* d_xyz_gradient_accum,
                      const float* d_normal_gradient_accum, const float* d_denom, const float* d_weights_accum,
                      const float* d_max_radii2D, int32_t* d_src_row, int32_t* d_kind, int32_t* d_counts, void* d_temp);

/* r3dg_densify_gather: builds every output tensor from the row map in ONE launch (the reference runs cat + cat +
 *   mask + mask over each parameter and both Adam moments: cat_tensors_to_optimizer :721-744, _prune_optimizer :681-698).
 *   Groups are [rows, row_floats] fp32; exp_avg pointers may be NULL (no optimizer state).  Split children: the
 *   ROLE_XYZ group receives R(q) (exp(scaling) * z) + xyz, the ROLE_SCALING group log(exp(scaling) / split_divisor)
 *   (densify_and_split :806-814); d_xyz / d_scaling_raw / d_rotation_raw are the SOURCE tensors of those formulas. */
#define R3DG_DENSIFY_MAX_GROUPS 24
#define R3DG_DENSIFY_ROLE_COPY 0
#define R3DG_DENSIFY_ROLE_XYZ 1
#define R3DG_DENSIFY_ROLE_SCALING 2
typedef struct r3dg_densify_group {
    const float* src_param;
    const float* src_exp_avg;
    const float* src_exp_avg_sq;
    float* dst_param;
    float* dst_exp_avg;
    float* dst_exp_avg_sq;
    uint32_t row_floats, role;
} r3dg_densify_group;
int r3dg_densify_gather(void* stream, int rows_out, const int32_t* d_src_row, const int32_t* d_kind, int n_groups,
                        const r3dg_densify_group* groups, const float* d_xyz, const float* d_scaling_raw,
                        const float* d_rotation_raw, const float* d_normal_table, float split_divisor);

/* GaussianModel.reset_opacity (:563-566): raw opacity <- inverse_sigmoid(min(sigmoid(raw), 0.01)) and zeroed Adam
 * moments (replace_tensor_to_optimizer :667-679; moment pointers may be NULL). */
int r3dg_reset_opacity(void* stream, int P, float* d_opacity_raw, float* d_exp_avg, float* d_exp_avg_sq);

/* distCUDA2 (submodules/simple-knn/spatial.cu:14-26 -> SimpleKNN::knn, simple_knn.cu:185-221): d_mean_dist2[i] = mean of
 * the squared distances from point i to its 3 nearest neighbours (FLT_MAX terms when P < 4, like the reference). */
size_t r3dg_knn_temp_bytes(int P);
int r3dg_knn_dist2(void* stream, int P, const float* d_points, float* d_mean_dist2, void* d_temp);

/* LBVH over per-Gaussian leaf boxes + visibility trace (reference bvh/include/bvh.h:5-18).
 * r3dg_bvh_build: d_nodes int32[2P-1,5] = (parent,left,right,object_id,leaf_count) and d_aabbs float[2P-1,6] =
 *   (lower xyz, upper xyz) arrive initialised as bvh/__init__.py:31-57 prepares them (nodes -1, counts 0 internal /
 *   1 leaf, leaf boxes in rows P-1..) and are completed IN PLACE; d_morton int64[P] receives the 64-bit codes.
 * r3dg_bvh_trace_opacity: one ray per (rays_o, rays_d) row; covs3D is the 6-vector INVERSE covariance
 *   (GaussianModel.get_inverse_covariance); outputs must be pre-set by the caller to 0 / 1 (bvh.cu:101-102);
 *   *d_stack_overflow (zeroed by the caller) counts rays that needed more than the 64-entry traversal stack;
 *   num_gaussians = P of the tree (rows of d_means3D): lets the library repack the tree into one 64-byte record per node for
 *   the walk (<= 0: unknown, the arrays are walked as they are).  Rays are traced in blocks of 256 consecutive rows; callers
 *   that can should order them so that consecutive rays start near each other (train_step.update_visibility does). */
size_t r3dg_bvh_build_temp_bytes(int P);
int r3dg_bvh_build(void* stream, int P, int32_t* d_nodes, float* d_aabbs, int64_t* d_morton, void* d_temp);
int r3dg_bvh_trace_opacity(void* stream, int64_t num_rays, int num_gaussians, const int32_t* d_nodes, const float* d_aabbs,
                           const float* d_rays_o, const float* d_rays_d, const float* d_means3D,
                           const float* d_covs3D, const float* d_opacities, const float* d_normals,
                           int32_t* d_num_contributes, float* d_rendered_opacity, int32_t* d_stack_overflow);

/* The same trace for callers that keep a tracer around (bvh.RayTracer; update_visibility traces the ray bundles in chunks
 * against ONE tree): the 64-byte traversal records r3dg_bvh_trace_opacity rebuilds on every call are packed ONCE into a buffer
 * the caller owns -- r3dg_bvh_trace_records_bytes(P) bytes, valid while the tree and the four per-Gaussian arrays are
 * unchanged -- and traced any number of times.  The buffer also holds the per-XCD ray-queue heads of a trace in flight: one
 * trace at a time per buffer (tracers on different streams use their own buffers; r3dg_bvh_trace_opacity keeps one private
 * scratch per device and stream).  Results are bit-identical to r3dg_bvh_trace_opacity. */
size_t r3dg_bvh_trace_records_bytes(int num_gaussians);
int r3dg_bvh_pack_traversal(void* stream, int num_gaussians, const int32_t* d_nodes, const float* d_aabbs,
                            const float* d_means3D, const float* d_covs3D, const float* d_opacities,
                            const float* d_normals, void* d_records);
int r3dg_bvh_trace_opacity_packed(void* stream, int64_t num_rays, int num_gaussians, void* d_records, const float* d_rays_o,
                                  const float* d_rays_d, int32_t* d_num_contributes, float* d_rendered_opacity,
                                  int32_t* d_stack_overflow);

/* A visibility update without host-side tensor work (train_step.update_visibility_device; GaussianModel.update_visibility,
 * scene/gaussian_model.py:312-342, is what it restates).
 * r3dg_bvh_prepare_leaves: one launch for everything r3dg_bvh_build and the trace need from the activated Gaussians
 *   (d_scales [P,3] activated, d_rotations [P,4] raw or normalised, d_means3D [P,3]): d_nodes int32[2P-1,5] and d_aabbs
 *   float[2P-1,6] initialised as bvh/__init__.py:29-57 prepares them (nodes -1, counts 0 internal / 1 leaf, internal boxes
 *   +-100000, the 3-sigma oriented box of the eight signed corners in the leaf rows P-1..) -- BIT-IDENTICAL to the PyTorch
 *   operations of that file, so the tree built from them is the same tree -- and d_covs3D_inv float[P,6], the inverse
 *   covariance 6-vector of GaussianModel.get_inverse_covariance (same formula, fp32 rounding of its own).
 * r3dg_bvh_trace_bundles: the trace of r3dg_bvh_trace_opacity_packed over rays the kernel generates itself: for every Morton
 *   leaf slot i in [leaf_lo, leaf_hi) (row P-1+i of d_nodes: object id g) and every k < K the ray with direction
 *   d = normalize(rotation_between_z(normal_g) z_k) (utils/sh_utils.py:36-68, graphics_utils.py:9-37; d_zsamples [K,3] = the
 *   Fibonacci set around +z; mean and normal of g are read from d_records, what r3dg_bvh_pack_traversal wrote) and origin
 *   mean_g + d * origin_offset (RayTracer.trace_visibility: 0.05).  The transmittance goes to d_visibility[g*K + k], the hit
 *   count to d_num_contributes[g*K + k] (NULL: not wanted), d to d_dirs_out[g,k,:] (NULL: not wanted; [P,K,3]) -- the caller's
 *   row order; rows of leaves outside [leaf_lo, leaf_hi) are untouched, so ranks or calls that split the slots fill one buffer.
 *   Each result is bit-identical to r3dg_bvh_trace_opacity_packed given that origin and direction.  *d_stack_overflow as above;
 *   num_gaussians * K must fit an int; one trace at a time per d_records.  P == 0 or an empty range: nothing is launched. */
int r3dg_bvh_prepare_leaves(void* stream, int P, const float* d_means3D, const float* d_scales, const float* d_rotations,
                            int32_t* d_nodes, float* d_aabbs, float* d_covs3D_inv);
int r3dg_bvh_trace_bundles(void* stream, int num_gaussians, int K, void* d_records, const int32_t* d_nodes,
                           const float* d_zsamples, int leaf_lo, int leaf_hi, float origin_offset, float* d_visibility,
                           int32_t* d_num_contributes, float* d_dirs_out, int32_t* d_stack_overflow);

/* Baking traced visibility into the per-Gaussian SH coefficients (visibility_bake.VisibilityBaker;
 * GaussianModel.finetune_visibility, scene/gaussian_model.py:275-310, is what it restates -- with the prediction taken from the live
 * coefficients, which the reference's loop reads from a copy made before it starts, :289).  T iterations are two launches:
 * r3dg_bvh_trace_hemisphere: the trace of r3dg_bvh_trace_opacity_packed over the T random hemisphere rays of every Gaussian: for
 *   every Morton leaf slot i in [leaf_lo, leaf_hi) (object id g) and every t < T the ray with direction d = z / max(|z|, 1e-12),
 *   z = d_raw_dirs[t,g,:] (F.normalize of the caller's draw), negated when d . normal_g < 0 (strict; mean and normal of g are read
 *   from d_records), and origin mean_g + d * origin_offset.  The transmittance goes to d_visibility[t*P + g], d to
 *   d_dirs_out[(t*P + g)*3 ..], the hit count to d_num_contributes[t*P + g] (NULL: not wanted): iteration-major, what the fit reads
 *   coalesced; rows of leaves outside [leaf_lo, leaf_hi) are untouched.  Each result is bit-identical to
 *   r3dg_bvh_trace_opacity_packed given that origin and direction.  P * T must fit an int; one trace at a time per d_records;
 *   P == 0, T == 0 or an empty range: nothing is launched.
 * r3dg_visibility_sh_fit: T Adam steps of every Gaussian's 16 coefficients in one launch, one thread per Gaussian with the 48 state
 *   values in registers.  Iteration t: Y = the degree-3 SH basis (utils/sh_utils.py:71-128) at d_dirs[t,g,:], x = sum c Y + 0.5,
 *   vhat = clamp(x, 0, 1), gradient sign(vhat - v) [0 <= x <= 1] Y / P of mean |v - vhat| (sign(0) = 0, the clamp's mask inclusive
 *   at both ends), then torch.optim.Adam's default single-tensor step number steps_done + t + 1 (bias corrections in double).
 *   d_coeffs / d_exp_avg / d_exp_avg_sq [P,16] (16-byte aligned) are updated in place.  The same inputs give the same bits, and T
 *   iterations split into several calls (steps_done advanced by the caller) give the bits of one call.  d_loss_partials (NULL: not
 *   wanted), [r3dg_visibility_sh_fit_loss_rows(P), T]: per-workgroup sums of |v - vhat| per iteration; the loss of iteration t is
 *   the sum of column t, added by the caller in a fixed order, divided by P (no float atomics). */
int r3dg_bvh_trace_hemisphere(void* stream, int num_gaussians, int T, void* d_records, const int32_t* d_nodes,
                              const float* d_raw_dirs, int leaf_lo, int leaf_hi, float origin_offset, float* d_visibility,
                              float* d_dirs_out, int32_t* d_num_contributes, int32_t* d_stack_overflow);
int r3dg_visibility_sh_fit(void* stream, int P, int T, int64_t steps_done, const float* d_dirs, const float* d_visibility,
                           float lr, float beta1, float beta2, float eps, float* d_coeffs, float* d_exp_avg,
                           float* d_exp_avg_sq, float* d_loss_partials);
int r3dg_visibility_sh_fit_loss_rows(int P);
/* Measurement ("report rays/s and node-visits/s"): with R3DG_OPT_TRACE_COUNT_VISITS = 1 the phased trace counts
 * its node steps (one slab test of both children of a node, trace.cu:228-246) and leaf steps (one Gaussian evaluated,
 * :247-276); r3dg_bvh_trace_visits synchronises `stream` and returns the two sums of the LAST trace over `d_records` in
 * node_and_leaf_steps[0..1] (host memory).  Results of the trace itself are unchanged. */
int r3dg_bvh_trace_visits(void* stream, int num_gaussians, const void* d_records, uint64_t* node_and_leaf_steps);

/* trace_bvh (bvh/include/bvh.h:8-12, bvh/src/trace.cu:8-192; no caller in the reference's Python): per-ray hit lists.
 *   r3dg_bvh_trace_count: num_contributes[r] = number of leaves in the <=4-leaf subtrees ray r reaches (trace.cu:21-58);
 *   (caller: inclusive scan of the counts into int64 offsets, allocation of the n = last offset entries)
 *   r3dg_bvh_trace_fill: the entries of every ray in traversal order: key = ray << 32 | bits(t), point id (-1 = rejected,
 *     t = 1e6), position = o + t d, ray id (trace.cu:88-166);
 *   (caller: stable sort by key -- r3dg_sort_pairs -- and the gather of point_list / position_list, trace.cu:171-175). */
int r3dg_bvh_trace_count(void* stream, int64_t num_rays, const int32_t* d_nodes, const float* d_aabbs,
                         const float* d_rays_o, const float* d_rays_d, int32_t* d_num_contributes,
                         int32_t* d_stack_overflow);
int r3dg_bvh_trace_fill(void* stream, int64_t num_rays, const int32_t* d_nodes, const float* d_aabbs,
                        const float* d_rays_o, const float* d_rays_d, const float* d_means3D,
                        const int32_t* d_num_contributes, const int64_t* d_offsets_inclusive, uint64_t* d_keys,
                        int32_t* d_point_list, float* d_position_list, int32_t* d_ray_id_list);

/* Stable ascending radix sort of (u64 key, u32 value) pairs on key bits [0,end_bit) -- the semantics of
 * cub::DeviceRadixSort::SortPairs as used at rasterizer_impl.cu:313-318. Exposed for tests/benchmarks.
 * d_temp must hold r3dg_sort_temp_bytes(n) bytes. Inputs are clobbered (used as ping-pong space). */
size_t r3dg_sort_temp_bytes(int64_t n);
int r3dg_sort_pairs(void* stream, int64_t n, uint64_t* d_keys_in, uint32_t* d_vals_in, uint64_t* d_keys_out,
                    uint32_t* d_vals_out, int end_bit, void* d_temp);

/* Tuning / experiment knobs (NOT part of the drop-in surface; defaults are the measured best, results never depend on them
 * beyond the order of float atomics).  r3dg_set_option returns R3DG_EINVAL for an unknown option or a value out of range. */
enum r3dg_option {
    R3DG_OPT_TILE_ORDER = 0,            /* block -> tile map: 1 longest tile list first (default), 0 natural order */
    R3DG_OPT_CULL,                      /* 1 = conservative per-block cull of the staged entries in the tile kernels (default), 0 = every
                                         * entry is evaluated; identical results */
    R3DG_OPT_TILE_BINNING,              /* instance ordering: 2 = direct tile binning + per-tile sort (default), 1 = radix partition by
                                         * tile + per-tile sort, 0 = the reference's one global radix sort; identical lists either way */
    R3DG_OPT_BINNING_BLOCK_K,           /* direct binning: Gaussians per workgroup / 1024 (1..4, default 2) */
    R3DG_OPT_STAGE_SH_ROWS,             /* per-Gaussian kernels move SH / dL_dsh rows through LDS (1, default) or walk them in HBM (0) */
    R3DG_OPT_SHADE_FWD_BLOCKS_PER_CU,   /* persistent workgroups per CU of the general shading forward; 0 = as many as fit (default) */
    R3DG_OPT_TRACE_FORMULATION,         /* visibility trace: 1 = packed records, phase-separated persistent waves (default),
                                         * 0 = one fixed ray per thread over the reference's tables */
    R3DG_OPT_TRACE_REFILL,              /* idle lanes at which a persistent trace wave refills (default 16) */
    R3DG_OPT_TRACE_NODE_WEIGHT,         /* vote weights of the phased trace */
    R3DG_OPT_TRACE_LEAF_WEIGHT,
    R3DG_OPT_RESERVE_CUS,               /* CUs the persistent kernels (shading, trace, long-tile sort) leave free for a collective running
                                         * beside them (default 0; the data-parallel iteration sets it) */
    R3DG_OPT_TRACE_COUNT_VISITS,        /* 1 = the phased trace counts node and leaf steps (measurement: r3dg_bvh_trace_visits); default 0 */
    R3DG_OPT_BWD_LEAN,                  /* 1 (default) = the tile backward takes its lean instances (no depth slot) when the caller passed no
                                         * depth gradient; 0 = never (A/B and parity tests: same gradients up to rounding order) */
    R3DG_OPT_COUNT
};
int r3dg_set_option(int option, int value);       /* the PROCESS default */
int r3dg_get_option(int option, int* value);      /* what a launch issued by the calling thread would see right now */
/* Option contexts -- settings that belong to an OBJECT (a training step, a renderer, a tracer), not to the process.  A context
 * overrides the process defaults for the options set on it; r3dg_context_make_current installs it for the CALLING THREAD (every
 * entry point of this library launches on its caller's thread and reads its knobs at launch time), NULL removes it; *previous
 * (may be NULL) receives the context that was current, so calls nest.  Two objects with different settings in one process, or two
 * threads, never see each other's values -- r3dg_set_option alone is process-global mutable state. */
void* r3dg_context_create(void);
void r3dg_context_destroy(void* ctx);
int r3dg_context_set_option(void* ctx, int option, int value);
int r3dg_context_make_current(void* ctx, void** previous);
/* r3dg_selftest_transpose_reduce: one wave reduces d_in[64][N] -> d_out[64] (+ channel / owner maps) with the transposing
 * DPP / permlane reduction (dpp != 0) or the __shfl_xor one. */
int r3dg_selftest_transpose_reduce(void* stream, int N, int dpp, const float* d_in, float* d_out, int* d_chan,
                                   int* d_owner);

/* Per-stage kernel timing with HIP events recorded on the launch stream (used by bench.py for the roofline
 * numbers).  Stages: see r3dg_profile_stage_name(0..r3dg_profile_num_stages()-1). */
int r3dg_profile_enable(int on);
int r3dg_profile_pause(int paused);   /* suspend (1) / resume (0) recording without clearing */
int r3dg_profile_num_stages(void);
const char* r3dg_profile_stage_name(int stage);
int r3dg_profile_read(double* ms_out, int* count_out);

#ifdef __cplusplus
}
#endif
#endif /* R3DG_HIP_H */
