// Elementwise Gaussian-diffusion step math (gaussian_diffusion.py:200-218, 290-346, 369-401,
// 787-788).  HBM-bound streaming kernels: float4 accesses, one table gather per batch row.
#include "common_hip.h"
#include "philox_normal.h"

namespace {

__global__ __launch_bounds__(256) void q_sample_kernel(const float* __restrict__ x0, const float* __restrict__ noise,
                                                       const int64_t* __restrict__ t, const float* __restrict__ sa,
                                                       const float* __restrict__ sb, float* __restrict__ out, int inner) {
    const int b = blockIdx.y;
    const float ca = sa[t[b]], cb = sb[t[b]];
    const size_t base = (size_t)b * inner;
    for (int i = (blockIdx.x * blockDim.x + threadIdx.x) * 4; i < inner; i += gridDim.x * blockDim.x * 4) {
        if (i + 3 < inner) {
            st4(out + base + i, ca * ld4(x0 + base + i) + cb * ld4(noise + base + i));
        } else {
            for (int j = i; j < inner; ++j) out[base + j] = ca * x0[base + j] + cb * noise[base + j];
        }
    }
}

// The x_{t-1} update (include/lfvdm_hip.h) is three kernels - given noise, noise drawn in the kernel, fused with the output
// convolution - over two COMPILE-TIME choices.  The update rule:
//   RULE_ANCESTRAL  mean = c1[t] p0 + c2[t] x, sigma = exp(0.5 logvar[t])                          (:369-401)
//   RULE_DDIM       the same form with the folded DDIM coefficients k1[t], k2[t] in the c1 / c2 slots and sigma[t] itself
//                   in the logvar slot (ddim_sample / ddim_reverse_sample, :524-610; folded on the host in float64, see
//                   GaussianDiffusion.ddim_coefficients)
//   RULE_DDIM_DET   eta = 0 and the reverse step: no sigma table, no noise read, no Philox rounds, no noise store
//   RULE_DPMPP2M    DPM-Solver++(2M) (Lu et al. 2022, Algorithm 2): the deterministic DDIM mean of k1[t], k2[t], then
//                   mean += k3[t] (p0 - hist) where k3[t] != 0; hist = the x0-hat of the step before.  No noise either
//                   (multistep_mean below).
//                   Only the given-noise kernel and the fused one are instantiated with it (lfvdm_update_ms_x0,
//                   lfvdm_conv_out_update_ms_x0; GaussianDiffusion.dpm_solver_coefficients folds k3 in float64)
enum { RULE_ANCESTRAL = 0, RULE_DDIM = 1, RULE_DDIM_DET = 2, RULE_DPMPP2M = 3 };
constexpr bool rule_draws(int rule) { return rule == RULE_ANCESTRAL || rule == RULE_DDIM; }

// What the network's output IS (ModelMeanType, :305-326):
//   MEAN_EPS  the noise: p0 = sqrt_recip_acp[t] x - sqrt_recipm1_acp[t] eps      (_predict_xstart_from_eps, :341-346)
//   MEAN_X0   x0-hat itself (predict_xstart=True): p0 = the output; the two tables are neither loaded nor multiplied and
//             their pointers may be null
// Everything behind p0 - clamp, c1 p0 + c2 x, the noise (same key, counter and stream), the stores - is shared text.
enum { MEAN_EPS = 0, MEAN_X0 = 1 };

template <int MEAN>
__device__ __forceinline__ float mean_x0hat(float r, float rm1, float xv, float out) {
    return MEAN == MEAN_X0 ? out : r * xv - rm1 * out;
}

template <int RULE>
__device__ __forceinline__ float rule_sigma(const float* __restrict__ t_logvar, int64_t tb) {
    if (RULE == RULE_ANCESTRAL) return tb != 0 ? expf(0.5f * t_logvar[tb]) : 0.f;      // [t != 0] exp(0.5 log_variance), :396-400
    if (RULE == RULE_DDIM) return tb != 0 ? t_logvar[tb] : 0.f;
    return 0.f;
}

// The coefficients of batch row b's step, gathered once per thread from the five tables at tb = t[b].  No __restrict__ on
// the tables here: what the compiler may assume about them is what the calling kernel's own parameters say.
struct StepCoef { float r, rm1, c1, c2, sigma; };

template <int RULE, int MEAN>
__device__ __forceinline__ StepCoef step_coef(int64_t tb, const float* t_recip, const float* t_recipm1, const float* t_c1,
                                              const float* t_c2, const float* t_logvar) {
    return {MEAN == MEAN_EPS ? t_recip[tb] : 0.f, MEAN == MEAN_EPS ? t_recipm1[tb] : 0.f, t_c1[tb], t_c2[tb],
            rule_sigma<RULE>(t_logvar, tb)};
}

// p0 = the (clamped) x0-hat; returns the mean c1 p0 + c2 x (q_posterior_mean_variance, :228-231).  The noise is NOT applied
// here: the given-noise kernel adds it only where t != 0 and must not read its buffer at t = 0, the other two always add.
template <int MEAN>
__device__ __forceinline__ float step_mean(const StepCoef& k, float xv, float out, int clip, float& p0) {
    p0 = mean_x0hat<MEAN>(k.r, k.rm1, xv, out);
    if (clip) p0 = fminf(fmaxf(p0, -1.f), 1.f);
    return k.c1 * p0 + k.c2 * xv;
}

// RULE_DPMPP2M: step_mean with its roundings SPELLED OUT, then the second-order term.  step_mean leaves the compiler free
// to fuse either product of c1 p0 + c2 x (and of r x - rm1 out) into an fma, and it decides per instantiation: written
// with step_mean, the multistep cells came out as packed multiplies plus an add, one rounding away from the deterministic
// DDIM cells.  The intrinsics below are what p_sample_kernel<RULE_DDIM_DET> compiles to - p0 = fma(r, x, -(rm1 out)),
// mean = fma(c2, x, c1 p0) - in BOTH multistep kernels, so a row whose k3 is 0 (the first step of a chain and the last two)
// has the bits of lfvdm_update_x0's deterministic DDIM rule and never reads hist, and the fused launch has the bits of the
// stand-alone one.  (conv_out_psample_kernel<.., RULE_DDIM_DET, MEAN_X0> happens to fuse the OTHER product, c1 p0: against
// that one cell a k3 = 0 row can differ in the last bit.)  tests/test_dpm_solver_gpu.py holds all of this.
template <int MEAN>
__device__ __forceinline__ float multistep_mean(const StepCoef& k, float k3, float xv, float out, int clip, const float* hist,
                                                size_t at, float& p0) {
    p0 = MEAN == MEAN_X0 ? out : __fmaf_rn(k.r, xv, -__fmul_rn(k.rm1, out));
    if (clip) p0 = fminf(fmaxf(p0, -1.f), 1.f);
    float mean = __fmaf_rn(k.c2, xv, __fmul_rn(k.c1, p0));
    if (k3 != 0.f) mean = __fmaf_rn(k3, __fsub_rn(p0, hist[at]), mean);
    return mean;
}

// pred is written through a __restrict__ pointer except under RULE_DPMPP2M, whose hist may BE pred (each thread reads its
// element of hist before it writes that element of pred)
template <int RULE> struct PredOut { typedef float* __restrict__ ptr; };
template <> struct PredOut<RULE_DPMPP2M> { typedef float* ptr; };

// x and sample may alias (the sampler updates its state in place): no __restrict__ on them.
template <int RULE, int MEAN>
__global__ __launch_bounds__(256) void p_sample_kernel(const float* x, const float* __restrict__ eps,
                                                       const float* __restrict__ noise, const int64_t* __restrict__ t,
                                                       const float* __restrict__ t_recip, const float* __restrict__ t_recipm1,
                                                       const float* __restrict__ t_c1, const float* __restrict__ t_c2,
                                                       const float* __restrict__ t_logvar, int clip,
                                                       float* sample, typename PredOut<RULE>::ptr pred,
                                                       float* __restrict__ mean_out, int inner, const float* hist,
                                                       const float* __restrict__ t_k3) {
    const int b = blockIdx.y;
    const int64_t tb = t[b];
    const StepCoef k = step_coef<RULE, MEAN>(tb, t_recip, t_recipm1, t_c1, t_c2, t_logvar);
    const float k3 = RULE == RULE_DPMPP2M ? t_k3[tb] : 0.f;
    const size_t base = (size_t)b * inner;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < inner; i += gridDim.x * blockDim.x) {
        float p0;
        const float mean = RULE == RULE_DPMPP2M ? multistep_mean<MEAN>(k, k3, x[base + i], eps[base + i], clip, hist, base + i, p0)
                                                : step_mean<MEAN>(k, x[base + i], eps[base + i], clip, p0);
        float sv = mean;
        if (rule_draws(RULE) && tb != 0) sv += k.sigma * noise[base + i];
        sample[base + i] = sv;
        if (pred) pred[base + i] = p0;
        if (mean_out) mean_out[base + i] = mean;
    }
}

// ---- the same update with the Gaussian noise drawn in the kernel (one launch less per sampling step): normal4 of
// philox_normal.h, counter = (quad index within the row, batch row, timestep, NOISE_STREAM_UPDATE).
template <int RULE, int MEAN>
__global__ __launch_bounds__(256) void p_sample_rng_kernel(const float* x, const float* __restrict__ eps,
                                                           float* __restrict__ noise_out, const int64_t* __restrict__ t,
                                                           const float* __restrict__ t_recip, const float* __restrict__ t_recipm1,
                                                           const float* __restrict__ t_c1, const float* __restrict__ t_c2,
                                                           const float* __restrict__ t_logvar, int clip, float* sample,
                                                           float* __restrict__ pred, float* __restrict__ mean_out, int inner,
                                                           const int64_t* __restrict__ seed) {
    const int b = blockIdx.y;
    const int64_t tb = t[b];
    const StepCoef k = step_coef<RULE, MEAN>(tb, t_recip, t_recipm1, t_c1, t_c2, t_logvar);
    const unsigned long long key = RULE != RULE_DDIM_DET ? (unsigned long long)seed[0] : 0ull;
    const unsigned k0 = (unsigned)key, k1 = (unsigned)(key >> 32);
    const size_t base = (size_t)b * inner;
    const int nq = (inner + 3) >> 2;
    for (int qd = blockIdx.x * blockDim.x + threadIdx.x; qd < nq; qd += gridDim.x * blockDim.x) {
        f32x4 z = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (RULE != RULE_DDIM_DET) z = normal4((unsigned)qd, (unsigned)b, (unsigned)tb, k0, k1);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = 4 * qd + e;
            if (i < inner) {
                float p0;
                const float mean = step_mean<MEAN>(k, x[base + i], eps[base + i], clip, p0);
                sample[base + i] = RULE != RULE_DDIM_DET ? mean + k.sigma * z[e] : mean;
                if (RULE != RULE_DDIM_DET && noise_out) noise_out[base + i] = z[e];
                if (pred) pred[base + i] = p0;
                if (mean_out) mean_out[base + i] = mean;
            }
        }
    }
}

// ---- The U-Net's output convolution and the update in ONE launch (the last two launches of a replayed sampling step:
// a 64 -> 4 convolution run as an implicit GEMM with 28 of its 32 filter columns padding, 10.4 us, and the update,
// 5.2 us).  eps = conv3x3(act) + bias with act = SiLU(GN(h)) as channels-last rows (reference unet.py:399-403,462-464),
// then exactly p_sample_rng_kernel's arithmetic and noise on it.  Direct convolution: SIXTEEN lanes share an output pixel
// and split its input channels (each lane CPL float4 of every tap: a pixel's 256-byte channel rows are read contiguously),
// partial sums combined with four butterfly steps inside the 16-lane row; a wave = four consecutive x positions = one
// noise quad of each output channel, so the lanes (pixel j, channel co < CO) finish with the update of their own element.
// The packed filters [CO][9][C] (lfvdm_pack_conv_weight) sit in LDS; the four pixels of a wave read the same addresses.
struct HeadUpdate {
    const float *act, *Wp, *bias, *x, *noise_in;
    float *eps_out, *noise_out, *sample, *pred, *mean_out;
    const int64_t *t, *seed;
    const float *t_recip, *t_recipm1, *t_c1, *t_c2, *t_logvar;
    int N, T, H, W, C, clip;
    const float *hist, *t_k3;      // RULE_DPMPP2M only
};

template <int CO, int CPL, int RULE, int MEAN>
__global__ __launch_bounds__(256) void conv_out_psample_kernel(const HeadUpdate p) {
    extern __shared__ __attribute__((aligned(16))) float wl[];      // [CO * 9][C]
    const int tid = threadIdx.x;
    const int C = p.C;
    {   // filters -> LDS, all loads in flight before the first store (C = 64 CPL: the trip count is a constant)
        constexpr int NW4 = CO * 9 * 16 * CPL, NIT = (NW4 + 255) / 256;
        f32x4 wv[NIT];
#pragma unroll
        for (int u = 0; u < NIT; ++u) {
            const int i = tid + 256 * u;
            wv[u] = i < NW4 ? ld4(p.Wp + 4 * (size_t)i) : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < NIT; ++u) {
            const int i = tid + 256 * u;
            if (i < NW4) st4(wl + 4 * i, wv[u]);
        }
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
    const int WQ = p.W >> 2;
    const long quad = (long)blockIdx.x * 4 + wave;
    if (quad >= (long)p.N * p.H * WQ) return;                       // whole wave, after the only barrier
    const int n = (int)(quad / (p.H * WQ));
    const int rem = (int)(quad - (long)n * p.H * WQ);
    const int y = rem / WQ, xq = rem - y * WQ;
    const int j = lane >> 4, cl = lane & 15;
    const int x = 4 * xq + j;
    float acc[CO];
#pragma unroll
    for (int co = 0; co < CO; ++co) acc[co] = 0.f;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const int iy = y + tap / 3 - 1, ix = x + tap % 3 - 1;
        const bool inb = iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
        const float* a = p.act + ((size_t)(n * p.H + (inb ? iy : y)) * p.W + (inb ? ix : x)) * C;
#pragma unroll
        for (int u = 0; u < CPL; ++u) {
            const int c = (cl + 16 * u) * 4;
            f32x4 a4 = ld4(a + c);
            if (!inb) a4 = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int co = 0; co < CO; ++co) {
                const f32x4 w4 = ld4(wl + (co * 9 + tap) * C + c);
                acc[co] += (a4.x * w4.x + a4.y * w4.y) + (a4.z * w4.z + a4.w * w4.w);
            }
        }
    }
#pragma unroll
    for (int co = 0; co < CO; ++co)
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) acc[co] += __shfl_xor(acc[co], o, 64);
    if (cl >= CO) return;
    float e = acc[0];
#pragma unroll
    for (int co = 1; co < CO; ++co) e = cl == co ? acc[co] : e;
    const int co = cl;
    e += p.bias[co];
    const int b = n / p.T, tt = n - b * p.T;
    const int inner = p.T * CO * p.H * p.W;
    const int i = ((tt * CO + co) * p.H + y) * p.W + x;             // element of the (T, C, H, W) frame stack
    const size_t at = (size_t)b * inner + i;
    const int64_t tb = p.t[b];
    const StepCoef k = step_coef<RULE, MEAN>(tb, p.t_recip, p.t_recipm1, p.t_c1, p.t_c2, p.t_logvar);
    float z = 0.f;
    if (!rule_draws(RULE)) {
    } else if (p.noise_in) {
        z = p.noise_in[at];
    } else {
        const unsigned long long key = (unsigned long long)p.seed[0];
        const f32x4 z4 = normal4((unsigned)(i >> 2), (unsigned)b, (unsigned)tb, (unsigned)key, (unsigned)(key >> 32));
        z = j == 0 ? z4.x : j == 1 ? z4.y : j == 2 ? z4.z : z4.w;  // x = 4 * xq + j and W % 4 == 0: i & 3 == j
    }
    float p0;
    const float mean = RULE == RULE_DPMPP2M ? multistep_mean<MEAN>(k, p.t_k3[tb], p.x[at], e, p.clip, p.hist, at, p0)
                                            : step_mean<MEAN>(k, p.x[at], e, p.clip, p0);
    p.sample[at] = rule_draws(RULE) ? mean + k.sigma * z : mean;
    if (p.eps_out) p.eps_out[at] = e;
    if (rule_draws(RULE) && p.noise_out) p.noise_out[at] = z;
    if (p.pred) p.pred[at] = p0;
    if (p.mean_out) p.mean_out[at] = mean;
}

// out[b] = (1/inner_total) * sum_{t, i} (a - b)^2 * mask[b, t]; one workgroup of 1024 threads per batch row, float4 loads
// (fixed summation order: deterministic).  The first version walked the row with 256 scalar-loading threads: 24 us for
// 82 k elements, twice per training step.
__global__ __launch_bounds__(1024) void masked_mse_kernel(const float* __restrict__ a, const float* __restrict__ bb,
                                                          const float* __restrict__ mask, float* __restrict__ out, int T,
                                                          int frame_inner) {
    const int b = blockIdx.x;
    const size_t base = (size_t)b * T * frame_inner;
    float acc = 0.f;
    if ((frame_inner & 3) == 0) {
        const int q = frame_inner >> 2, total = T * q;
        for (int e = threadIdx.x; e < total; e += 1024) {
            const int t = e / q;
            const float mk = mask ? mask[b * T + t] : 1.f;
            const f32x4 d = ld4(a + base + (size_t)e * 4) - ld4(bb + base + (size_t)e * 4);
            acc += ((d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w)) * mk;
        }
    } else {
        for (int t = 0; t < T; ++t) {
            const float mk = mask ? mask[b * T + t] : 1.f;
            for (int i = threadIdx.x; i < frame_inner; i += 1024) {
                const float d = a[base + (size_t)t * frame_inner + i] - bb[base + (size_t)t * frame_inner + i];
                acc += d * d * mk;
            }
        }
    }
    __shared__ float red[16];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int w = 0; w < 16; ++w) t += red[w];
        out[b] = t / (float)((size_t)T * frame_inner);
    }
}

// its backward: dpred = -2 (target - pred) * mask[b, t] * g[b] / inner   (closed form, one launch)
__global__ __launch_bounds__(256) void masked_mse_bwd_kernel(const float* __restrict__ target, const float* __restrict__ pred,
                                                             const float* __restrict__ mask, const float* __restrict__ g,
                                                             float* __restrict__ dpred, int T, int frame_inner) {
    const int b = blockIdx.y;
    const size_t base = (size_t)b * T * frame_inner;
    const float sc = -2.0f * g[b] / (float)((size_t)T * frame_inner);
    const long total = (long)T * frame_inner;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const float mk = mask ? mask[b * T + (int)(i / frame_inner)] : 1.f;
        dpred[base + i] = (target[base + i] - pred[base + i]) * (sc * mk);
    }
}

}  // namespace

extern "C" int lfvdm_masked_mse_bwd(const float* target, const float* pred, const float* mask, const float* g, float* dpred,
                                    int B, int T, int frame_inner, void* stream) {
    if (B <= 0 || T <= 0 || frame_inner <= 0 || !target || !pred || !g || !dpred) return LFVDM_E_SHAPE;
    long gx = ((long)T * frame_inner + 255) / 256;
    if (gx > 1024) gx = 1024;
    hipLaunchKernelGGL(masked_mse_bwd_kernel, dim3((unsigned)gx, B), dim3(256), 0, (hipStream_t)stream, target, pred, mask, g, dpred,
                       T, frame_inner);
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}

extern "C" int lfvdm_q_sample(const float* x0, const float* noise, const int64_t* t, const float* sqrt_acp,
                              const float* sqrt_1macp, float* out, int B, int inner, void* stream) {
    if (B <= 0 || inner <= 0) return LFVDM_E_SHAPE;
    int gx = (inner / 4 + 255) / 256;
    if (gx > 1024) gx = 1024;
    if (gx < 1) gx = 1;
    hipLaunchKernelGGL(q_sample_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, x0, noise, t, sqrt_acp, sqrt_1macp, out, inner);
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}

namespace {
// one thread per batch element: t <- max(t - 1, 0); model_t <- table[t]
__global__ void sampler_tick_kernel(int64_t* __restrict__ t, const float* __restrict__ table, float* __restrict__ model_t, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int64_t v = t[b] - 1;
    v = v < 0 ? 0 : v;
    t[b] = v;
    model_t[b] = table[v];
}

// tick + fetch in ONE workgroup: the rows of the per-timestep table that belong to the new t replace the per-step
// embedding launches (the table is built once per chain with the very same kernels, _engine.Plan.build_time_tables)
__global__ __launch_bounds__(1024) void sampler_tick_fetch_kernel(int64_t* __restrict__ t, const float* __restrict__ table,
                                                                  float* __restrict__ model_t, int B,
                                                                  const float* __restrict__ rows_all, int rows_ld,
                                                                  float* __restrict__ rows, int row_floats) {
    __shared__ int64_t tnew[64];
    if ((int)threadIdx.x < B) {
        int64_t v = t[threadIdx.x] - 1;
        v = v < 0 ? 0 : v;
        t[threadIdx.x] = v;
        model_t[threadIdx.x] = table[v];
        tnew[threadIdx.x] = v;
    }
    __syncthreads();
    const int q4 = row_floats >> 2;
    for (int e = threadIdx.x; e < B * q4; e += 1024) {
        const int b = e / q4, i = e - b * q4;
        const float* src = rows_all + ((size_t)tnew[b] * B + b) * rows_ld;      // both buffers have rows of rows_ld floats,
        st4(rows + (size_t)b * rows_ld + 4 * i, ld4(src + 4 * i));              // of which the first row_floats are fetched
    }
}

}  // namespace

extern "C" int lfvdm_sampler_tick_fetch(int64_t* t, const float* model_timestep_table, float* model_t, int B,
                                        const float* rows_all, int rows_ld, float* rows, int row_floats, void* stream) {
    if (B <= 0 || B > 64 || !t || !model_timestep_table || !model_t || !rows_all || !rows) return LFVDM_E_SHAPE;
    if (row_floats <= 0 || (row_floats & 3) || (rows_ld & 3) || rows_ld < row_floats) return LFVDM_E_SHAPE;
    hipLaunchKernelGGL(sampler_tick_fetch_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, t, model_timestep_table, model_t, B,
                       rows_all, rows_ld, rows, row_floats);
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}

extern "C" int lfvdm_sampler_tick(int64_t* t, const float* model_timestep_table, float* model_t, int B, void* stream) {
    if (B <= 0 || !t || !model_timestep_table || !model_t) return LFVDM_E_SHAPE;
    hipLaunchKernelGGL(sampler_tick_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, t, model_timestep_table,
                       model_t, B);
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}

extern "C" int lfvdm_conv_out_psample_ok(int N, int H, int W, int C, int Cout) {
    if (N <= 0 || H <= 0 || W <= 0 || W % 4 || (Cout != 3 && Cout != 4)) return LFVDM_E_UNSUPPORTED;
    if (C != 64 && C != 128 && C != 256) return LFVDM_E_UNSUPPORTED;
    if ((long)N * H * W * C >= (1L << 31) / 4) return LFVDM_E_UNSUPPORTED;
    return LFVDM_OK;
}

// ---- the three update entries: validate once (update_cell), then launch the cell's instantiation (on_grid)
namespace {
template <int RULE, int MEAN>
int launch_update(const float* x, const float* eps, const float* noise, const int64_t* t, const float* recip, const float* recipm1,
                  const float* c1, const float* c2, const float* sg, int clip, float* sample, float* pred, float* mean_out, int B,
                  int inner, void* stream, const float* hist = nullptr, const float* k3 = nullptr) {
    int gx = (inner + 255) / 256;
    if (gx > 1024) gx = 1024;
    hipLaunchKernelGGL((p_sample_kernel<RULE, MEAN>), dim3(gx, B), dim3(256), 0, (hipStream_t)stream, x, eps, noise, t, recip, recipm1, c1,
                       c2, sg, clip, sample, pred, mean_out, inner, hist, k3);
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}

template <int RULE, int MEAN>
int launch_update_rng(const float* x, const float* eps, float* noise_out, const int64_t* t, const float* recip,
                      const float* recipm1, const float* c1, const float* c2, const float* sg, int clip, float* sample, float* pred,
                      float* mean_out, int B, int inner, const int64_t* seed, void* stream) {
    int gx = ((inner + 3) / 4 + 255) / 256;
    if (gx > 1024) gx = 1024;
    hipLaunchKernelGGL((p_sample_rng_kernel<RULE, MEAN>), dim3(gx, B), dim3(256), 0, (hipStream_t)stream, x, eps, noise_out, t, recip,
                       recipm1, c1, c2, sg, clip, sample, pred, mean_out, inner, seed);
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}

template <int RULE, int MEAN>
int launch_head(const HeadUpdate& p, int Cout, void* stream) {
    if (int rc = lfvdm_conv_out_psample_ok(p.N, p.H, p.W, p.C, Cout)) return rc;
    const long quads = (long)p.N * p.H * (p.W / 4);
    const dim3 grid((unsigned)((quads + 3) / 4));
    const size_t lds = (size_t)Cout * 9 * p.C * sizeof(float);
    hipStream_t s = (hipStream_t)stream;
    const int C = p.C;
#define LFVDM_HEAD(CO, CPL) hipLaunchKernelGGL((conv_out_psample_kernel<CO, CPL, RULE, MEAN>), grid, dim3(256), lds, s, p)
    if (Cout == 4) {
        if (C == 64) LFVDM_HEAD(4, 1); else if (C == 128) LFVDM_HEAD(4, 2); else LFVDM_HEAD(4, 4);
    } else {
        if (C == 64) LFVDM_HEAD(3, 1); else if (C == 128) LFVDM_HEAD(3, 2); else LFVDM_HEAD(3, 4);
    }
#undef LFVDM_HEAD
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}

// -> RULE_* of the template grid, or -1: DDIM without a sigma table is the deterministic rule
int grid_rule(int rule, const float* sg) {
    if (rule == LFVDM_RULE_ANCESTRAL) return sg ? RULE_ANCESTRAL : -1;
    if (rule == LFVDM_RULE_DDIM) return sg ? RULE_DDIM : RULE_DDIM_DET;
    return -1;
}
bool mean_ok(int mean_type, const float* recip, const float* recipm1) {
    if (mean_type == LFVDM_MEAN_X0) return true;
    return mean_type == LFVDM_MEAN_EPS && recip && recipm1;
}
// Everything the three entries check alike -> the cell's RULE_*, or -1.  have_noise: the entry's own source of z (a noise
// buffer or a seed), required in every cell but the deterministic one.
int update_cell(int rule, int mean_type, const float* x, const float* model_out, const int64_t* t, const float* recip,
                const float* recipm1, const float* c1, const float* c2, const float* sg, const float* sample, int B, int inner,
                bool have_noise) {
    const int R = grid_rule(rule, sg);
    if (R < 0 || !mean_ok(mean_type, recip, recipm1)) return -1;
    if (B <= 0 || inner <= 0 || !x || !model_out || !t || !c1 || !c2 || !sample) return -1;
    return R == RULE_DDIM_DET || have_noise ? R : -1;
}

template <int V> struct Const { static constexpr int value = V; };
// f(Const<RULE>, Const<MEAN>) on the cell of the 3 x 2 template grid
template <class F>
int on_grid(int R, int mean_type, F f) {
    const bool x0 = mean_type == LFVDM_MEAN_X0;
    switch (R) {
        case RULE_ANCESTRAL: return x0 ? f(Const<RULE_ANCESTRAL>(), Const<MEAN_X0>()) : f(Const<RULE_ANCESTRAL>(), Const<MEAN_EPS>());
        case RULE_DDIM: return x0 ? f(Const<RULE_DDIM>(), Const<MEAN_X0>()) : f(Const<RULE_DDIM>(), Const<MEAN_EPS>());
        case RULE_DDIM_DET: return x0 ? f(Const<RULE_DDIM_DET>(), Const<MEAN_X0>()) : f(Const<RULE_DDIM_DET>(), Const<MEAN_EPS>());
    }
    return LFVDM_E_SHAPE;
}
}  // namespace

extern "C" int lfvdm_update_x0(const float* x, const float* model_out, const float* noise, const int64_t* t,
                               const float* sqrt_recip_acp, const float* sqrt_recipm1_acp, const float* c1, const float* c2,
                               const float* sg, int rule, int mean_type, int clip, float* sample, float* pred_xstart,
                               float* mean_out, int B, int inner, void* stream) {
    const int R = update_cell(rule, mean_type, x, model_out, t, sqrt_recip_acp, sqrt_recipm1_acp, c1, c2, sg, sample, B, inner,
                              noise != nullptr);
    if (R < 0) return LFVDM_E_SHAPE;
    return on_grid(R, mean_type, [&](auto r, auto m) {
        return launch_update<decltype(r)::value, decltype(m)::value>(
            x, model_out, decltype(r)::value == RULE_DDIM_DET ? nullptr : noise, t, sqrt_recip_acp, sqrt_recipm1_acp, c1, c2, sg,
            clip, sample, pred_xstart, mean_out, B, inner, stream);
    });
}

extern "C" int lfvdm_update_rng_x0(const float* x, const float* model_out, float* noise_out, const int64_t* t,
                                   const float* sqrt_recip_acp, const float* sqrt_recipm1_acp, const float* c1, const float* c2,
                                   const float* sg, int rule, int mean_type, int clip, float* sample, float* pred_xstart,
                                   float* mean_out, int B, int inner, const int64_t* seed, void* stream) {
    const int R = update_cell(rule, mean_type, x, model_out, t, sqrt_recip_acp, sqrt_recipm1_acp, c1, c2, sg, sample, B, inner,
                              seed != nullptr);
    if (R < 0) return LFVDM_E_SHAPE;
    return on_grid(R, mean_type, [&](auto r, auto m) {
        constexpr bool det = decltype(r)::value == RULE_DDIM_DET;
        return launch_update_rng<decltype(r)::value, decltype(m)::value>(
            x, model_out, det ? nullptr : noise_out, t, sqrt_recip_acp, sqrt_recipm1_acp, c1, c2, sg, clip, sample, pred_xstart,
            mean_out, B, inner, det ? nullptr : seed, stream);
    });
}

// model_out of the fused launch is the convolution's result: act / Wp / bias stand in for it
extern "C" int lfvdm_conv_out_update_x0(const float* act, const float* Wp, const float* bias, float* out, const float* x,
                                        const float* noise_in, float* noise_out, const int64_t* t, const float* sqrt_recip_acp,
                                        const float* sqrt_recipm1_acp, const float* c1, const float* c2, const float* sg,
                                        int rule, int mean_type, int clip, float* sample, float* pred_xstart, float* mean_out,
                                        int B, int T, int H, int W, int C, int Cout, const int64_t* seed, void* stream) {
    const int R = update_cell(rule, mean_type, x, act, t, sqrt_recip_acp, sqrt_recipm1_acp, c1, c2, sg, sample, B, T,
                              noise_in || seed);
    if (R < 0 || !Wp || !bias) return LFVDM_E_SHAPE;
    const bool det = R == RULE_DDIM_DET;
    const HeadUpdate p = {act, Wp, bias, x, det ? nullptr : noise_in, out, det ? nullptr : noise_out, sample, pred_xstart, mean_out,
                          t, det ? nullptr : seed, sqrt_recip_acp, sqrt_recipm1_acp, c1, c2, sg, B * T, T, H, W, C, clip,
                          nullptr, nullptr};
    return on_grid(R, mean_type, [&](auto r, auto m) { return launch_head<decltype(r)::value, decltype(m)::value>(p, Cout, stream); });
}

// ---- the multistep entries: one rule (RULE_DPMPP2M; without a history, the deterministic DDIM cell itself), two mean types
namespace {
bool multistep_ok(int mean_type, const float* x, const float* model_out, const int64_t* t, const float* recip,
                  const float* recipm1, const float* k1, const float* k2, const float* k3, const float* sample, int B, int inner) {
    if (!mean_ok(mean_type, recip, recipm1)) return false;
    return B > 0 && inner > 0 && x && model_out && t && k1 && k2 && k3 && sample;
}
// f(Const<RULE>, Const<MEAN>) on RULE_DPMPP2M, or on RULE_DDIM_DET where there is no history
template <class F>
int on_multistep(bool have_hist, int mean_type, F f) {
    const bool x0 = mean_type == LFVDM_MEAN_X0;
    if (have_hist) return x0 ? f(Const<RULE_DPMPP2M>(), Const<MEAN_X0>()) : f(Const<RULE_DPMPP2M>(), Const<MEAN_EPS>());
    return x0 ? f(Const<RULE_DDIM_DET>(), Const<MEAN_X0>()) : f(Const<RULE_DDIM_DET>(), Const<MEAN_EPS>());
}
}  // namespace

extern "C" int lfvdm_update_ms_x0(const float* x, const float* model_out, const float* hist, const int64_t* t,
                                  const float* sqrt_recip_acp, const float* sqrt_recipm1_acp, const float* k1, const float* k2,
                                  const float* k3, int mean_type, int clip, float* sample, float* pred_xstart, int B, int inner,
                                  void* stream) {
    if (!multistep_ok(mean_type, x, model_out, t, sqrt_recip_acp, sqrt_recipm1_acp, k1, k2, k3, sample, B, inner))
        return LFVDM_E_SHAPE;
    return on_multistep(hist != nullptr, mean_type, [&](auto r, auto m) {
        return launch_update<decltype(r)::value, decltype(m)::value>(x, model_out, nullptr, t, sqrt_recip_acp, sqrt_recipm1_acp, k1,
                                                                     k2, nullptr, clip, sample, pred_xstart, nullptr, B, inner,
                                                                     stream, hist, k3);
    });
}

extern "C" int lfvdm_conv_out_update_ms_x0(const float* act, const float* Wp, const float* bias, float* out, const float* x,
                                           const float* hist, const int64_t* t, const float* sqrt_recip_acp,
                                           const float* sqrt_recipm1_acp, const float* k1, const float* k2, const float* k3,
                                           int mean_type, int clip, float* sample, float* pred_xstart, int B, int T, int H, int W,
                                           int C, int Cout, void* stream) {
    if (!multistep_ok(mean_type, x, act, t, sqrt_recip_acp, sqrt_recipm1_acp, k1, k2, k3, sample, B, T) || !Wp || !bias)
        return LFVDM_E_SHAPE;
    const HeadUpdate p = {act, Wp, bias, x, nullptr, out, nullptr, sample, pred_xstart, nullptr, t, nullptr, sqrt_recip_acp,
                          sqrt_recipm1_acp, k1, k2, nullptr, B * T, T, H, W, C, clip, hist, k3};
    return on_multistep(hist != nullptr, mean_type,
                        [&](auto r, auto m) { return launch_head<decltype(r)::value, decltype(m)::value>(p, Cout, stream); });
}

extern "C" int lfvdm_masked_mse(const float* a, const float* b, const float* mask, float* out, int B, int T,
                                int frame_inner, void* stream) {
    if (B <= 0 || T <= 0 || frame_inner <= 0) return LFVDM_E_SHAPE;
    hipLaunchKernelGGL(masked_mse_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, a, b, mask, out, T, frame_inner);
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}
