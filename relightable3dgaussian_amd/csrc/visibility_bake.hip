// Baking traced visibility into the 16 SH coefficients every stage-2 Gaussian carries (visibility_dc / visibility_rest), for gfx950.
// Reference semantics: GaussianModel.finetune_visibility, scene/gaussian_model.py:275-310 -- per iteration one random ray per
// Gaussian in the hemisphere of its normal, traced; eval_sh (utils/sh_utils.py:71-128) + 0.5 clamped to [0,1]; F.l1_loss against
// the traced value; one torch.optim.Adam step -- with the prediction taken from the LIVE coefficients (the reference's loop reads a
// copy made before the loop, :289, and so never sees its own updates).
//
// The trace does not depend on the coefficients and a Gaussian's fit only on its own rays (the one cross-Gaussian quantity is the
// constant 1/P of the mean), so T iterations are ONE trace launch (bvh_trace.hip, HemisphereRays: directions and transmittances
// iteration-major, [T,P,3] and [T,P]) and ONE launch of the kernel below: a thread per Gaussian keeps the 16 coefficients and
// their 32 Adam moments in registers through the T steps.  Nothing crosses lanes in the state path, so the same inputs give the
// same bits, and T split into chunks gives the same bits as T at once (the state travels through memory exactly; the bias
// corrections are a function of the step number alone).
#include "launchers.hpp"
#include "shading_math.hpp"

namespace r3dg {

constexpr int FIT_LOSS_BATCH = 32;        // iterations whose per-wave loss sums wait in LDS for one barrier

// b^n by squaring, in double: the same value for the same n however the iterations are chunked
__device__ __forceinline__ double power_of(double b, long long n)
{
    double r = 1.0;
    while (n > 0) {
        if (n & 1) r *= b;
        b *= b;
        n >>= 1;
    }
    return r;
}

// One thread per Gaussian, 256-thread workgroups.  dirs [T,P,3], vis [T,P]; coeffs / exp_avg / exp_avg_sq [P,16], loaded once,
// stored once.  Every state array is indexed by unrolled constants only (a dynamic index would put it into scratch: the static
// test of tests/test_visibility_bake_cpu.py).  Per iteration, with Y the degree-3 basis at the ray's direction:
//   x = sum c Y + 0.5, vhat = clamp(x, 0, 1), g = sign(vhat - v) [0 <= x <= 1] Y / P     (l1_loss's mean, clamp's inclusive mask)
//   torch.optim.Adam, single-tensor form: exp_avg.lerp_(g, 1 - b1); exp_avg_sq = b2 exp_avg_sq + (1 - b2) g g;
//   denom = sqrt(exp_avg_sq) / sqrt(1 - b2^n) + eps; c -= (lr / (1 - b1^n)) exp_avg / denom, n = steps_done + t + 1, the bias
//   corrections in double.
// loss (optional, [gridDim.x, T]): the workgroup's sum of |v - vhat| per iteration; the caller adds the rows in a fixed order.
// Lanes past P run on a copy of the last Gaussian (the barriers of the loss need every lane), add nothing and store nothing.
__global__ void __launch_bounds__(256)
visibility_sh_fit_kernel(int P, int T, long long steps_done, const float* __restrict__ dirs, const float* __restrict__ vis,
                         double lr, double beta1, double beta2, float eps, float* __restrict__ coeffs,
                         float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq, float* __restrict__ loss)
{
    __shared__ float s_part[FIT_LOSS_BATCH][4];
    const int gid = blockIdx.x * 256 + threadIdx.x;
    const bool live = gid < P;
    const int row = live ? gid : P - 1;
    const float b1 = (float)beta1, b2 = (float)beta2;
    const float w1 = 1.f - b1, w2 = 1.f - b2;                 // (exact in float: the weights sum to the bias corrections)
    const float inv_P = 1.f / (float)P;
    float c[16], m[16], v[16];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const float4 a = reinterpret_cast<const float4*>(coeffs + 16 * (size_t)row)[q];
        const float4 b = reinterpret_cast<const float4*>(exp_avg + 16 * (size_t)row)[q];
        const float4 d = reinterpret_cast<const float4*>(exp_avg_sq + 16 * (size_t)row)[q];
        c[4 * q] = a.x; c[4 * q + 1] = a.y; c[4 * q + 2] = a.z; c[4 * q + 3] = a.w;
        m[4 * q] = b.x; m[4 * q + 1] = b.y; m[4 * q + 2] = b.z; m[4 * q + 3] = b.w;
        v[4 * q] = d.x; v[4 * q + 1] = d.y; v[4 * q + 2] = d.z; v[4 * q + 3] = d.w;
    }
    // the next iteration's four inputs are in flight while this one is computed
    float nx = dirs[3 * (size_t)row], ny = dirs[3 * (size_t)row + 1], nz = dirs[3 * (size_t)row + 2], nv = vis[row];
    for (int t0 = 0; t0 < T; t0 += FIT_LOSS_BATCH) {
        const int tn = min(FIT_LOSS_BATCH, T - t0);
        for (int u = 0; u < tn; u++) {
            const int t = t0 + u;
            const float dx = nx, dy = ny, dz = nz, vt = nv;
            if (t + 1 < T) {
                const size_t r = (size_t)(t + 1) * P + row;
                nx = dirs[3 * r]; ny = dirs[3 * r + 1]; nz = dirs[3 * r + 2]; nv = vis[r];
            }
            float Y[16];
            sh_basis16(dx, dy, dz, 16, Y);
            float s = c[0] * Y[0];
#pragma unroll
            for (int k = 1; k < 16; k++) s += c[k] * Y[k];
            const float x = s + 0.5f;
            const float vhat = fminf(fmaxf(x, 0.f), 1.f);
            const float diff = vhat - vt;
            const float sgn = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);
            const float gs = (x >= 0.f && x <= 1.f) ? sgn * inv_P : 0.f;
            const long long n = steps_done + t + 1;
            const double bc1 = 1.0 - power_of(beta1, n), bc2 = 1.0 - power_of(beta2, n);
            const float step = (float)(lr / bc1), bc2_sqrt = (float)sqrt(bc2);
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const float g = gs * Y[k];
                m[k] = m[k] + w1 * (g - m[k]);
                v[k] = b2 * v[k] + (w2 * g) * g;
                const float denom = sqrtf(v[k]) / bc2_sqrt + eps;
                c[k] = c[k] - (step * m[k]) / denom;
            }
            if (loss != nullptr) {
                const float a = wave_sum(live ? fabsf(vt - vhat) : 0.f);
                if ((threadIdx.x & 63) == 0) s_part[u][threadIdx.x >> 6] = a;
            }
        }
        if (loss != nullptr) {
            __syncthreads();
            if ((int)threadIdx.x < tn)
                loss[(size_t)blockIdx.x * T + t0 + threadIdx.x] =
                    ((s_part[threadIdx.x][0] + s_part[threadIdx.x][1]) + s_part[threadIdx.x][2]) + s_part[threadIdx.x][3];
            __syncthreads();
        }
    }
    if (!live) return;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        reinterpret_cast<float4*>(coeffs + 16 * (size_t)row)[q] = make_float4(c[4 * q], c[4 * q + 1], c[4 * q + 2], c[4 * q + 3]);
        reinterpret_cast<float4*>(exp_avg + 16 * (size_t)row)[q] = make_float4(m[4 * q], m[4 * q + 1], m[4 * q + 2], m[4 * q + 3]);
        reinterpret_cast<float4*>(exp_avg_sq + 16 * (size_t)row)[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
    }
}

// rows of the loss partials: one per workgroup
int visibility_sh_fit_loss_rows(int P) { return P > 0 ? (P + 255) / 256 : 0; }

void visibility_sh_fit(hipStream_t s, int P, int T, long long steps_done, const float* dirs, const float* visibility, float lr,
                       float beta1, float beta2, float eps, float* coeffs, float* exp_avg, float* exp_avg_sq, float* loss_partials)
{
    if (P <= 0 || T <= 0) return;
    visibility_sh_fit_kernel<<<(P + 255) / 256, 256, 0, s>>>(P, T, steps_done, dirs, visibility, (double)lr, (double)beta1,
                                                             (double)beta2, eps, coeffs, exp_avg, exp_avg_sq, loss_partials);
}

}  // namespace r3dg
