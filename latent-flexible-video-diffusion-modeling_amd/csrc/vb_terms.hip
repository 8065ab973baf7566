// One term of the variational bound per batch row, in bits per dimension (gaussian_diffusion.py:687-720 with
// losses.py:12-77), and its closed-form gradient with respect to the network's output.  Fixed sigma only.
//
//   x0-hat      = MEAN_EPS: sqrt_recip[t] x_t - sqrt_recipm1[t] out   |  MEAN_X0: out            (optionally clamped to [-1, 1])
//   mean_model  = c1[t] x0-hat + c2[t] x_t,   mean_true = c1[t] x_start + c2[t] x_t               (posterior_mean_coef1 / 2)
//   t != 0      : normal_kl(mean_true, post_logvar[t]; mean_model, model_logvar[t])
//   t == 0      : -discretized_gaussian_log_likelihood(x_start; mean_model, 0.5 model_logvar[t])
//   vb[b]       = mean over (T, C, H, W) of term * mask[b, frame] / ln 2       (nn.mean_flat: NOT divided by the mask count)
//
// Numerics.  mean_true - mean_model is evaluated as c1 (x_start - x0-hat): the c2 x_t parts cancel exactly.  The decoder
// term keeps the reference's tanh approximation of the normal CDF, Phi(x) ~ 0.5 (1 + tanh u(x)) with
// u = sqrt(2/pi)(x + 0.044715 x^3), in its sigmoid form 0.5 (1 + tanh u) = sigmoid(2u):
//   log cdf_plus         = logsigmoid(A),  A = 2 u(plus_in)
//   log (1 - cdf_min)    = logsigmoid(-B), B = 2 u(min_in)
//   log (cdf_plus - cdf_min) = logsigmoid(A) + logsigmoid(-B) + log(1 - exp(B - A))      (A > B always: u is increasing)
// which has no 1 + tanh cancellation in the tails.  The reference's clamp(min=1e-12) of the three arguments is part of the
// definition and is kept as max(log, log 1e-12); so are the x < -0.999 / x > 0.999 branches.  The build has no fast-math
// flag: expf / logf / log1pf / expm1f are the accurate library forms.
//
// Shape of the kernels: lfvdm_masked_mse / lfvdm_masked_mse_bwd (diffusion_ops.hip).  Forward: one workgroup of 1024
// threads per batch row, 16-byte loads, wave64 shuffle sums, then the 16 wave partials added in index order by one thread -
// no float atomics, bitwise reproducible.  The per-row scalars are gathered from the tables once per workgroup (uniform
// loads).  Memory-bound: three or four input streams, one optional output stream.
#include <math.h>

#include "common_hip.h"

namespace {

enum { MEAN_EPS = 0, MEAN_X0 = 1 };

constexpr float kLogClamp = -27.631021115928547f;      // log(1e-12)
constexpr float kTwoSqrt2OverPi = 1.5957691216057308f;  // 2 sqrt(2 / pi)
constexpr float kCubic = 0.044715f;
constexpr float kBin = 1.0f / 255.0f;
constexpr float kInvLn2 = 1.4426950408889634f;

// per batch row, uniform over the workgroup
struct RowScalars {
    float r, rm1, c1, c2;
    float k0, k1;        // KL element = k0 + k1 d^2, d = mean_true - mean_model
    float inv_std;       // exp(-0.5 model_logvar[t])
    float inv_var;       // exp(-model_logvar[t])
    bool decoder;        // t == 0
};

template <int MEAN>
__device__ __forceinline__ RowScalars row_scalars(const int64_t* __restrict__ t, int b, const float* __restrict__ t_recip,
                                                  const float* __restrict__ t_recipm1, const float* __restrict__ t_c1,
                                                  const float* __restrict__ t_c2, const float* __restrict__ t_post_lv,
                                                  const float* __restrict__ t_model_lv) {
    RowScalars s;
    const int64_t tb = t[b];
    // x0 mode reads the two tables only where eps is recovered from x0-hat (eps_mse); they may be null otherwise
    s.r = t_recip ? t_recip[tb] : 0.f;
    s.rm1 = t_recipm1 ? t_recipm1[tb] : 0.f;
    s.c1 = t_c1[tb];
    s.c2 = t_c2[tb];
    const float lv2 = t_model_lv[tb];
    // 0.5 (-1 + lv2 - lv1 + exp(lv1 - lv2)): the three terms cancel to second order in lv2 - lv1 (exactly 0 for
    // FIXED_SMALL), so this one scalar per row is formed in double
    const double dl = t_post_lv ? (double)lv2 - (double)t_post_lv[tb] : 0.0;
    s.k0 = (float)(0.5 * (dl + expm1(-dl)));
    s.inv_var = expf(-lv2);
    s.k1 = 0.5f * s.inv_var;
    s.inv_std = expf(-0.5f * lv2);
    s.decoder = tb == 0;
    return s;
}

__device__ __forceinline__ float log_sigmoid(float z) { return fminf(z, 0.f) - log1pf(expf(-fabsf(z))); }
__device__ __forceinline__ float two_u(float x) { return kTwoSqrt2OverPi * (x + kCubic * x * x * x); }
__device__ __forceinline__ float two_du(float x) { return kTwoSqrt2OverPi * (1.f + 3.f * kCubic * x * x); }

// -log-likelihood of x_start under the discretized Gaussian (losses.py:50-77)
__device__ __forceinline__ float decoder_nll(float xs, float mean, float inv_std) {
    const float c = xs - mean;
    const float A = two_u(inv_std * (c + kBin)), Bv = two_u(inv_std * (c - kBin));
    float lp;
    if (xs < -0.999f) lp = log_sigmoid(A);
    else if (xs > 0.999f) lp = log_sigmoid(-Bv);
    else lp = log_sigmoid(A) + log_sigmoid(-Bv) + logf(-expm1f(Bv - A));
    return -fmaxf(lp, kLogClamp);      // log(0) = -inf and a NaN both end at the clamp, as clamp(min=1e-12) ends them
}

// d(-log-likelihood) / d mean; 0 where the 1e-12 clamp is active
__device__ __forceinline__ float decoder_nll_dmean(float xs, float mean, float inv_std) {
    const float c = xs - mean;
    const float p = inv_std * (c + kBin), m = inv_std * (c - kBin);
    const float A = two_u(p), Bv = two_u(m);
    const float dA = -two_du(p) * inv_std, dB = -two_du(m) * inv_std;      // d / d mean
    float dlp;
    if (xs < -0.999f) {
        dlp = log_sigmoid(A) > kLogClamp ? expf(log_sigmoid(-A)) * dA : 0.f;
    } else if (xs > 0.999f) {
        dlp = log_sigmoid(-Bv) > kLogClamp ? -expf(log_sigmoid(Bv)) * dB : 0.f;
    } else {
        const float lsA = log_sigmoid(A), lsnB = log_sigmoid(-Bv);
        const float E = -expm1f(Bv - A);
        const float lp = lsA + lsnB + logf(E);
        // sigma'(A) / delta = sigma(-A) / (sigma(-B) E),  sigma'(B) / delta = sigma(B) / (sigma(A) E): both ratios <= 1
        dlp = lp > kLogClamp ? (expf(log_sigmoid(-A) - lsnB) * dA - expf(log_sigmoid(Bv) - lsA) * dB) / E : 0.f;
    }
    return -dlp;
}

template <int MEAN>
struct Elem {
    float term, p0, dx, de;      // the bound's element, x0-hat, x0-hat - x_start, eps - noise
};

template <int MEAN>
__device__ __forceinline__ Elem<MEAN> vb_elem(const RowScalars& s, float xs, float xt, float out, float nz, int clip,
                                              bool want_eps) {
    Elem<MEAN> e;
    float p0 = MEAN == MEAN_X0 ? out : s.r * xt - s.rm1 * out;
    bool clamped = false;
    if (clip) {
        const float q = fminf(fmaxf(p0, -1.f), 1.f);
        clamped = q != p0;
        p0 = q;
    }
    if (s.decoder) {
        e.term = decoder_nll(xs, s.c1 * p0 + s.c2 * xt, s.inv_std);
    } else {
        const float d = s.c1 * (xs - p0);
        e.term = s.k0 + s.k1 * d * d;
    }
    e.p0 = p0;
    e.dx = p0 - xs;
    e.de = 0.f;
    if (want_eps) {
        // _predict_eps_from_xstart (:348-352); an unclamped epsilon-mode x0-hat gives back the output itself
        const float eps = (MEAN == MEAN_EPS && !clamped) ? out : (s.r * xt - p0) / s.rm1;
        e.de = eps - nz;
    }
    return e;
}

template <int MEAN>
__global__ __launch_bounds__(1024) void vb_terms_kernel(const float* __restrict__ x_start, const float* __restrict__ x_t,
                                                        const float* __restrict__ model_out, const float* __restrict__ noise,
                                                        const int64_t* __restrict__ t, const float* __restrict__ t_recip,
                                                        const float* __restrict__ t_recipm1, const float* __restrict__ t_c1,
                                                        const float* __restrict__ t_c2, const float* __restrict__ t_post_lv,
                                                        const float* __restrict__ t_model_lv, const float* __restrict__ mask,
                                                        int clip, float* __restrict__ vb, float* __restrict__ xstart_mse,
                                                        float* __restrict__ eps_mse, float* __restrict__ pred, int T,
                                                        int frame_inner, int out_ld, int col_base, int vec) {
    const int b = blockIdx.x;
    const RowScalars s = row_scalars<MEAN>(t, b, t_recip, t_recipm1, t_c1, t_c2, t_post_lv, t_model_lv);
    const size_t base = (size_t)b * T * frame_inner;
    const bool want_eps = eps_mse != nullptr;
    float av = 0.f, ax = 0.f, ae = 0.f;
    if (vec) {
        const int q = frame_inner >> 2, total = T * q;
        for (int e = threadIdx.x; e < total; e += 1024) {
            const float mk = mask ? mask[b * T + e / q] : 1.f;
            const size_t at = base + (size_t)e * 4;
            const f32x4 xs = ld4(x_start + at), xt = ld4(x_t + at), mo = ld4(model_out + at);
            const f32x4 nz = want_eps ? ld4(noise + at) : (f32x4){0.f, 0.f, 0.f, 0.f};
            f32x4 p;
            float sv = 0.f, sx = 0.f, se = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const Elem<MEAN> el = vb_elem<MEAN>(s, xs[k], xt[k], mo[k], nz[k], clip, want_eps);
                sv += el.term;
                sx += el.dx * el.dx;
                se += el.de * el.de;
                p[k] = el.p0;
            }
            av += sv * mk;
            ax += sx * mk;
            ae += se * mk;
            if (pred) st4(pred + at, p);
        }
    } else {
        for (int f = 0; f < T; ++f) {
            const float mk = mask ? mask[b * T + f] : 1.f;
            for (int i = threadIdx.x; i < frame_inner; i += 1024) {
                const size_t at = base + (size_t)f * frame_inner + i;
                const Elem<MEAN> el = vb_elem<MEAN>(s, x_start[at], x_t[at], model_out[at], want_eps ? noise[at] : 0.f, clip,
                                                    want_eps);
                av += el.term * mk;
                ax += el.dx * el.dx * mk;
                ae += el.de * el.de * mk;
                if (pred) pred[at] = el.p0;
            }
        }
    }
    __shared__ float red[3][16];
    av = wave_sum(av);
    ax = wave_sum(ax);
    ae = wave_sum(ae);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = av;
        red[1][threadIdx.x >> 6] = ax;
        red[2][threadIdx.x >> 6] = ae;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float tv = 0.f, tx = 0.f, te = 0.f;
        for (int w = 0; w < 16; ++w) {
            tv += red[0][w];
            tx += red[1][w];
            te += red[2][w];
        }
        // column of the (B, out_ld) results: col_base - t[b] (the loops' descending walk), or 0; never outside the row
        const long col = col_base >= 0 ? (long)col_base - (long)t[b] : 0;
        if (col >= 0 && col < out_ld) {
            const float inv_n = 1.0f / (float)((size_t)T * frame_inner);
            const size_t o = (size_t)b * out_ld + col;
            vb[o] = tv * inv_n * kInvLn2;
            if (xstart_mse) xstart_mse[o] = tx * inv_n;
            if (eps_mse) eps_mse[o] = te * inv_n;
        }
    }
}

// d vb[b] / d out * g[b], clip_denoised = False:  KL rows  -(mean_true - mean_model) exp(-logvar) dmean/dout,
// decoder rows through the sigmoid form, zero under a clamp;  dmean/dout = -c1 sqrt_recipm1 (epsilon) | c1 (x0)
template <int MEAN>
__global__ __launch_bounds__(256) void vb_terms_bwd_kernel(const float* __restrict__ x_start, const float* __restrict__ x_t,
                                                           const float* __restrict__ model_out, const int64_t* __restrict__ t,
                                                           const float* __restrict__ t_recip, const float* __restrict__ t_recipm1,
                                                           const float* __restrict__ t_c1, const float* __restrict__ t_c2,
                                                           const float* __restrict__ t_model_lv, const float* __restrict__ mask,
                                                           const float* __restrict__ g, float* __restrict__ dout, int T,
                                                           int frame_inner, int vec) {
    const int b = blockIdx.y;
    const RowScalars s = row_scalars<MEAN>(t, b, t_recip, t_recipm1, t_c1, t_c2, nullptr, t_model_lv);
    const size_t base = (size_t)b * T * frame_inner;
    const long total = (long)T * frame_inner;
    const float dmean = MEAN == MEAN_X0 ? s.c1 : -s.c1 * s.rm1;
    const float sc = g[b] * kInvLn2 / (float)total * dmean;
    auto grad = [&](float xs, float xt, float out) -> float {
        const float p0 = MEAN == MEAN_X0 ? out : s.r * xt - s.rm1 * out;
        if (s.decoder) return decoder_nll_dmean(xs, s.c1 * p0 + s.c2 * xt, s.inv_std);
        return -(s.c1 * (xs - p0)) * s.inv_var;
    };
    if (vec) {
        const long total4 = total >> 2;
        const int q = frame_inner >> 2;
        for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total4; e += (long)gridDim.x * 256) {
            const float mk = mask ? mask[b * T + (int)(e / q)] : 1.f;
            const size_t at = base + (size_t)e * 4;
            const f32x4 xs = ld4(x_start + at), xt = ld4(x_t + at), mo = ld4(model_out + at);
            f32x4 d;
#pragma unroll
            for (int k = 0; k < 4; ++k) d[k] = grad(xs[k], xt[k], mo[k]) * (sc * mk);
            st4(dout + at, d);
        }
    } else {
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
            const float mk = mask ? mask[b * T + (int)(i / frame_inner)] : 1.f;
            dout[base + i] = grad(x_start[base + i], x_t[base + i], model_out[base + i]) * (sc * mk);
        }
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int lfvdm_vb_terms(const float* x_start, const float* x_t, const float* model_out, const float* noise,
                              const int64_t* t, const float* sqrt_recip_acp, const float* sqrt_recipm1_acp, const float* c1,
                              const float* c2, const float* post_log_var, const float* model_log_var, const float* mask,
                              int mean_type, int clip, float* vb, float* xstart_mse, float* eps_mse, float* pred_xstart, int B,
                              int T, int frame_inner, int out_ld, int col_base, void* stream) {
    if (B <= 0 || T <= 0 || frame_inner <= 0 || out_ld <= 0) return LFVDM_E_SHAPE;
    if (!x_start || !x_t || !model_out || !t || !c1 || !c2 || !post_log_var || !model_log_var || !vb) return LFVDM_E_SHAPE;
    if (mean_type != LFVDM_MEAN_EPS && mean_type != LFVDM_MEAN_X0) return LFVDM_E_SHAPE;
    // epsilon mode always reads the two tables; x0 mode only to recover eps for eps_mse
    if ((mean_type == LFVDM_MEAN_EPS || eps_mse) && (!sqrt_recip_acp || !sqrt_recipm1_acp)) return LFVDM_E_SHAPE;
    if (eps_mse && !noise) return LFVDM_E_SHAPE;
    if (col_base < 0 && out_ld != 1) return LFVDM_E_SHAPE;
    const int vec = (frame_inner & 3) == 0 && aligned16(x_start) && aligned16(x_t) && aligned16(model_out) &&
                    (!eps_mse || aligned16(noise)) && (!pred_xstart || aligned16(pred_xstart));
#define LFVDM_VB(M)                                                                                                              \
    hipLaunchKernelGGL((vb_terms_kernel<M>), dim3(B), dim3(1024), 0, (hipStream_t)stream, x_start, x_t, model_out, noise, t,      \
                       sqrt_recip_acp, sqrt_recipm1_acp, c1, c2, post_log_var, model_log_var, mask, clip, vb, xstart_mse, eps_mse, \
                       pred_xstart, T, frame_inner, out_ld, col_base, vec)
    if (mean_type == LFVDM_MEAN_X0) LFVDM_VB(MEAN_X0);
    else LFVDM_VB(MEAN_EPS);
#undef LFVDM_VB
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}

extern "C" int lfvdm_vb_terms_bwd(const float* x_start, const float* x_t, const float* model_out, const int64_t* t,
                                  const float* sqrt_recip_acp, const float* sqrt_recipm1_acp, const float* c1, const float* c2,
                                  const float* model_log_var, const float* mask, const float* g, int mean_type, int clip,
                                  float* d_out, int B, int T, int frame_inner, void* stream) {
    if (B <= 0 || T <= 0 || frame_inner <= 0) return LFVDM_E_SHAPE;
    if (!x_start || !x_t || !model_out || !t || !c1 || !c2 || !model_log_var || !g || !d_out) return LFVDM_E_SHAPE;
    if (mean_type != LFVDM_MEAN_EPS && mean_type != LFVDM_MEAN_X0) return LFVDM_E_SHAPE;
    if (mean_type == LFVDM_MEAN_EPS && (!sqrt_recip_acp || !sqrt_recipm1_acp)) return LFVDM_E_SHAPE;
    if (clip) return LFVDM_E_UNSUPPORTED;      // the training loss never clips (gaussian_diffusion.py:749)
    const int vec = (frame_inner & 3) == 0 && aligned16(x_start) && aligned16(x_t) && aligned16(model_out) && aligned16(d_out);
    long gx = ((long)T * frame_inner / (vec ? 4 : 1) + 255) / 256;
    if (gx > 1024) gx = 1024;
    if (gx < 1) gx = 1;
#define LFVDM_VB_BWD(M)                                                                                                        \
    hipLaunchKernelGGL((vb_terms_bwd_kernel<M>), dim3((unsigned)gx, B), dim3(256), 0, (hipStream_t)stream, x_start, x_t,          \
                       model_out, t, sqrt_recip_acp, sqrt_recipm1_acp, c1, c2, model_log_var, mask, g, d_out, T, frame_inner, vec)
    if (mean_type == LFVDM_MEAN_X0) LFVDM_VB_BWD(MEAN_X0);
    else LFVDM_VB_BWD(MEAN_EPS);
#undef LFVDM_VB_BWD
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}
