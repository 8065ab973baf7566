// Known-region sampling (replacement conditioning, RePaint: Lugmayr et al. 2022): after the step that consumed timestep
// j = t[b], the part of the sampler's state that the caller knows is put back at the step's noise level,
//     x = m (a[j] known + s[j] eps) + (1 - m) x,     a = sqrt(alphas_cumprod_prev), s = sqrt(1 - alphas_cumprod_prev)
// with m a (B, T, H, W) mask in [0, 1] broadcast over the channels, and - for resampling - a state is taken one level
// back up,  x = sqrt(1 - beta[j]) x + sqrt(beta[j]) eps.  HBM-bound streaming kernels shaped like p_sample_rng_kernel
// (diffusion_ops.hip): one batch row per blockIdx.y, t and the table entries read once per thread, a grid-stride walk over
// quads of four consecutive elements with 16-byte accesses and one Philox call per quad.  No LDS, no atomics.
//
// Noise streams.  All in-kernel noise of a chain is normal4_stream of philox_normal.h under ONE key, the chain's seed, and
// the counter (quad, batch row, j, stream word).  The blend draws with stream word NOISE_STREAM_BLEND = 1, the re-noise
// with NOISE_STREAM_RENOISE = 2, the update kernels with 0: the fourth counter word differs, so the three never see the
// same Philox input.  The repeats of a resampled timestep differ by the KEY: the host steps the seed between replays
// (GaussianDiffusion._known_region_steps).
#include "common_hip.h"
#include "philox_normal.h"

namespace {

// FRESH: eps drawn here (and stored to noise_out if given); else read from `eps`.  VEC_MASK: H*W % 4 == 0, the four
// elements of a quad share a mask row and their mask values are one 16-byte load.
template <bool FRESH, bool VEC_MASK>
__global__ __launch_bounds__(256) void known_blend_kernel(float* __restrict__ x, const float* __restrict__ known,
                                                          const float* __restrict__ mask, const float* __restrict__ eps,
                                                          float* __restrict__ noise_out, const int64_t* __restrict__ t,
                                                          const float* __restrict__ t_a, const float* __restrict__ t_s,
                                                          const int64_t* __restrict__ seed, int T, int C, int HW) {
    const int b = blockIdx.y;
    const int64_t tb = t[b];
    const float a = t_a[tb], s = t_s[tb];
    const unsigned long long key = FRESH ? (unsigned long long)seed[0] : 0ull;
    const unsigned k0 = (unsigned)key, k1 = (unsigned)(key >> 32);
    const int CHW = C * HW, inner = T * CHW;
    const size_t base = (size_t)b * inner;
    const float* mrow = mask + (size_t)b * T * HW;
    const int nq = inner >> 2;
    for (int qd = blockIdx.x * blockDim.x + threadIdx.x; qd < nq; qd += gridDim.x * blockDim.x) {
        const int i = 4 * qd;
        f32x4 m;
        if (VEC_MASK) {
            const int tt = i / CHW, hw = (i - tt * CHW) % HW;
            m = ld4(mrow + tt * HW + hw);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int tt = (i + e) / CHW, hw = (i + e - tt * CHW) % HW;
                m[e] = mrow[tt * HW + hw];
            }
        }
        const f32x4 z = FRESH ? normal4_stream((unsigned)qd, (unsigned)b, (unsigned)tb, NOISE_STREAM_BLEND, k0, k1)
                              : ld4(eps + base + i);
        const f32x4 xv = ld4(x + base + i), kv = ld4(known + base + i);
        f32x4 r;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float v = a * kv[e] + s * z[e];
            // m == 0 and m == 1 are selects, not arithmetic: an untouched element keeps its bits (-0 included)
            r[e] = m[e] == 0.f ? xv[e] : m[e] == 1.f ? v : m[e] * v + (1.f - m[e]) * xv[e];
        }
        st4(x + base + i, r);
        if (FRESH && noise_out) st4(noise_out + base + i, z);
    }
}

__global__ __launch_bounds__(256) void renoise_kernel(float* __restrict__ x, float* __restrict__ noise_out,
                                                      const int64_t* __restrict__ t, const float* __restrict__ t_c,
                                                      const float* __restrict__ t_d, const int64_t* __restrict__ seed,
                                                      int inner) {
    const int b = blockIdx.y;
    const int64_t tb = t[b];
    const float c = t_c[tb], d = t_d[tb];
    const unsigned long long key = (unsigned long long)seed[0];
    const unsigned k0 = (unsigned)key, k1 = (unsigned)(key >> 32);
    const size_t base = (size_t)b * inner;
    const int nq = inner >> 2;
    for (int qd = blockIdx.x * blockDim.x + threadIdx.x; qd < nq; qd += gridDim.x * blockDim.x) {
        const f32x4 z = normal4_stream((unsigned)qd, (unsigned)b, (unsigned)tb, NOISE_STREAM_RENOISE, k0, k1);
        st4(x + base + 4 * qd, c * ld4(x + base + 4 * qd) + d * z);
        if (noise_out) st4(noise_out + base + 4 * qd, z);
    }
}

// B rides in gridDim.y: the entries refuse B > 65535 (LFVDM_E_SHAPE) before they launch.  As in the update kernels, t[b] is
// trusted to index the tables: the sampler's clock never leaves [0, num_timesteps).
constexpr int MAX_ROWS = 65535;

dim3 quad_grid(int inner, int B) {
    int gx = ((inner >> 2) + 255) / 256;
    if (gx > 1024) gx = 1024;
    return dim3(gx, B);
}

}  // namespace

extern "C" int lfvdm_known_blend(float* x, const float* known, const float* mask, const float* eps, float* noise_out,
                                 const int64_t* t, const float* sqrt_acp_prev, const float* sqrt_1macp_prev,
                                 const int64_t* seed, int B, int T, int C, int HW, void* stream) {
    if (!x || !known || !mask || !t || !sqrt_acp_prev || !sqrt_1macp_prev || (!eps && !seed)) return LFVDM_E_SHAPE;
    if (B <= 0 || B > MAX_ROWS || T <= 0 || C <= 0 || HW <= 0) return LFVDM_E_SHAPE;
    const long inner = (long)T * C * HW;
    if ((inner & 3) || inner >= (1L << 31)) return LFVDM_E_SHAPE;
    const dim3 grid = quad_grid((int)inner, B);
    hipStream_t st = (hipStream_t)stream;
#define LFVDM_BLEND(FRESH, VEC)                                                                                              \
    hipLaunchKernelGGL((known_blend_kernel<FRESH, VEC>), grid, dim3(256), 0, st, x, known, mask, eps, noise_out, t, sqrt_acp_prev, \
                       sqrt_1macp_prev, seed, T, C, HW)
    if (eps) {
        if (HW & 3) LFVDM_BLEND(false, false); else LFVDM_BLEND(false, true);
    } else {
        if (HW & 3) LFVDM_BLEND(true, false); else LFVDM_BLEND(true, true);
    }
#undef LFVDM_BLEND
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}

extern "C" int lfvdm_renoise(float* x, float* noise_out, const int64_t* t, const float* sqrt_1mbeta, const float* sqrt_beta,
                             const int64_t* seed, int B, int inner, void* stream) {
    if (!x || !t || !sqrt_1mbeta || !sqrt_beta || !seed) return LFVDM_E_SHAPE;
    if (B <= 0 || B > MAX_ROWS || inner <= 0 || (inner & 3)) return LFVDM_E_SHAPE;
    hipLaunchKernelGGL(renoise_kernel, quad_grid(inner, B), dim3(256), 0, (hipStream_t)stream, x, noise_out, t, sqrt_1mbeta,
                       sqrt_beta, seed, inner);
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}
