// Launchers of the relight frame's two opt-in caches: the transport cache under a fixed light (shading_transport.hpp; its
// builder from the ray set alone has a unit of its own, shading_relight_rayset.hip) and the split transport cache under a light
// that turns with every frame (shading_split.hpp).
#include "shading_host.hpp"
#include "shading_transport.hpp"
#include "shading_split.hpp"

namespace r3dg {

void launch_shade_build_split(hipStream_t s, int P, int K, const int* perm, const float* normals, const float* incidents,
                              const float* visibility, const float* dirs, const float* zsamples, float uniform_area, float* lt,
                              float* vis_t, float* consts)
{
    if (P == 0) return;
    shade_build_split_kernel<<<(P + 255) / 256, 256, 0, s>>>(P, K, perm, normals, incidents, visibility, dirs, zsamples,
                                                           frs_area(uniform_area), reinterpret_cast<float4*>(lt), vis_t, consts);
    check_launch(s, false, "shade_build_split_kernel");
}

void launch_shade_forward_split(hipStream_t s, int P, int K, const int* perm, const float* base_color, const float* roughness,
                                const float* normals, const float* viewdirs, const float* lt, const float* vis_t,
                                const float* consts, const float* zsamples, const float* tr, const float* env_fp, int He, int We,
                                float* out)
{
    if (P == 0) return;
    // sample range split into parts (shading_split.hpp): ~12+ waves per SIMD in the launch, parts a multiple of 4 samples long
    const int waves = (P + 63) / 64;
    int parts = (12 * 4 * persistent_cus() + waves - 1) / waves;
    parts = parts < 1 ? 1 : (parts > 8 ? 8 : parts);
    int Kp = ((K + parts - 1) / parts + 3) & ~3;
    parts = (K + Kp - 1) / Kp;
    float4* partial = reinterpret_cast<float4*>(stream_scratch(s, 1, (size_t)parts * P * 3 * sizeof(float4)));
    const dim3 grid((P + 255) / 256, parts);
    shade_forward_split_kernel<<<grid, 256, 0, s>>>(P, K, Kp, perm, base_color, roughness, normals, viewdirs,
                                                   reinterpret_cast<const float4*>(lt), vis_t, zsamples, tr,
                                                   reinterpret_cast<const float4*>(env_fp), He, We, partial);
    shade_split_combine_kernel<<<(P + 255) / 256, 256, 0, s>>>(P, K, parts, perm, base_color, partial, consts, out);
    check_launch(s, false, "shade_forward_split_kernel");
}

void launch_shade_env_footprints(hipStream_t s, int He, int We, const float* env, float* fp)
{
    const int n = (He + 1) * (We + 1);
    shade_env_footprints_kernel<<<(n + 255) / 256, 256, 0, s>>>(He, We, env, reinterpret_cast<float4*>(fp));
    check_launch(s, false, "shade_env_footprints_kernel");
}

void launch_shade_build_transport(hipStream_t s, int P, int K, int M, const float* normals, const float* incidents,
                                  const float* visibility, const float* dirs, const float* areas, float uniform_area,
                                  float* radiance_to_transport, float* consts)
{
    if (P == 0) return;
    shade_build_transport_kernel<<<(P + TR_WAVES - 1) / TR_WAVES, 64 * TR_WAVES, 0, s>>>(
        P, K, M, normals, incidents, visibility, dirs, areas, uniform_area, radiance_to_transport, consts);
    check_launch(s, false, "shade_build_transport_kernel");
}

void launch_shade_forward_transport(hipStream_t s, int P, int K, const float* base_color, const float* roughness,
                                    const float* normals, const float* viewdirs, const float* transport, const float* consts,
                                    const float* zsamples, const float* dirs, float* out)
{
    if (P == 0) return;
    shade_forward_transport_kernel<<<(P + TR_WAVES - 1) / TR_WAVES, 64 * TR_WAVES, 0, s>>>(
        P, K, base_color, roughness, normals, viewdirs, transport, consts, zsamples, dirs, out);
    check_launch(s, false, "shade_forward_transport_kernel");
}

}  // namespace r3dg
