// GroupNorm forward: the spatial form (coefficients, statistics and the materialised act(x*A + B), one launch or the
// chunked pair on large maps), then the temporal form.  All HBM/L2-bound; wave = 64.  The backward is norm_backward.hip.
#include "common_hip.h"
#include "gn_wave_body.h"

namespace {

// -------------------------------------------------------------------------------------
// gn_coef: one workgroup per (sample n, slice of 8 groups).  Two exact passes (mean, then
// centred variance) like ATen's CPU GroupNorm; small slices (<= 8 float4 per thread, i.e. every level of the
// 16x16 latent configs) stay in registers between the passes, larger ones are re-read from L2 for pass 2.
// Thread (pl, q): pixel lane pl strides over the P positions, q = float4 channel quad.
// -------------------------------------------------------------------------------------
constexpr int GN_GPW = 8;        // groups per workgroup
constexpr int GN_THREADS = 256;
constexpr int GN_MAXCW = 256;    // channels per workgroup: supports C <= 1024

template <int KEEP>      // float4 per thread held in registers between the passes: 8, or 16 for slices of up to 16 pixel lanes' worth
__global__ __launch_bounds__(GN_THREADS) void gn_coef_kernel(
    const float* __restrict__ s0, const float* __restrict__ s1, int C0, int C1, int P,
    const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ film, int film_div,
    int film_ld, float eps, float* __restrict__ coefA, float* __restrict__ coefB, float* __restrict__ stats,
    float* __restrict__ act_out, int act_mode) {
    const int C = C0 + C1;
    const int cg = C / 32;
    const float rcg = __builtin_amdgcn_rcpf((float)cg);
    const int CW = GN_GPW * cg;       // channels handled here
    const int Q = CW / 4;             // float4 quads
    const int n = blockIdx.x;
    const int cbase = blockIdx.y * CW;
    const int PL = GN_THREADS / Q;    // pixel lanes
    const int tid = threadIdx.x;
    const bool active = tid < PL * Q;
    const int q = active ? tid % Q : 0;
    const int pl = active ? tid / Q : 0;
    const int c = cbase + q * 4;

    __shared__ float part[GN_THREADS * 4];  // [pl][CW] partial channel sums
    __shared__ float chs[GN_MAXCW];
    __shared__ float gmean[GN_GPW], grstd[GN_GPW];
    __shared__ __attribute__((aligned(16))) float shA[GN_MAXCW], shB[GN_MAXCW];

    const size_t pos0 = (size_t)n * P;
    const bool pow2q = (Q & (Q - 1)) == 0 && Q <= 64;      // workgroup-uniform
    const bool cached = P <= KEEP * PL;       // workgroup-uniform
    f32x4 keep[KEEP];
    for (int pass = 0; pass < 2; ++pass) {
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        if (active) {
            f32x4 mu = {0.f, 0.f, 0.f, 0.f};
            if (pass) {
                mu.x = gmean[fdiv_small(q * 4 + 0, cg, rcg)]; mu.y = gmean[fdiv_small(q * 4 + 1, cg, rcg)];
                mu.z = gmean[fdiv_small(q * 4 + 2, cg, rcg)]; mu.w = gmean[fdiv_small(q * 4 + 3, cg, rcg)];
            }
            if (cached) {
#pragma unroll
                for (int i = 0; i < KEEP; ++i) {
                    const int p = pl + i * PL;
                    if (pass == 0) {
                        keep[i] = (p < P) ? ld_cat(s0, s1, C0, C1, pos0 + p, c) : (f32x4){0.f, 0.f, 0.f, 0.f};
                        s += keep[i];
                    } else if (p < P) {
                        const f32x4 v = keep[i] - mu;
                        s += v * v;
                    }
                }
            } else {
                for (int p = pl; p < P; p += PL) {
                    f32x4 v = ld_cat(s0, s1, C0, C1, pos0 + p, c);
                    if (pass) { v = v - mu; s += v * v; } else { s += v; }
                }
            }
            if (pow2q) {
                // quads of a wave repeat every Q lanes: butterfly over the pixel lanes of the wave, then one partial
                // row per wave (a serial sum over all PL pixel lanes - 64 dependent LDS reads at C = 64 - was half of
                // this kernel's time)
                for (int off = Q; off < 64; off <<= 1) {
                    s.x += __shfl_xor(s.x, off, 64); s.y += __shfl_xor(s.y, off, 64);
                    s.z += __shfl_xor(s.z, off, 64); s.w += __shfl_xor(s.w, off, 64);
                }
                if ((tid & 63) < Q) st4(part + ((tid >> 6) * Q + q) * 4, s);
            } else {
                st4(part + (pl * Q + q) * 4, s);
            }
        }
        __syncthreads();
        const int rows = pow2q ? GN_THREADS / 64 : PL;
        for (int cc = tid; cc < CW; cc += GN_THREADS) {
            float t = 0.f;
            for (int i = 0; i < rows; ++i) t += part[i * CW + cc];
            chs[cc] = t;
        }
        __syncthreads();
        if (tid < GN_GPW) {
            float t = 0.f;
            for (int i = 0; i < cg; ++i) t += chs[tid * cg + i];
            const float inv = 1.0f / (float)(cg * P);
            if (pass == 0) gmean[tid] = t * inv;
            else grstd[tid] = 1.0f / sqrtf(t * inv + eps);
        }
        __syncthreads();
    }
    if (stats && tid < GN_GPW) {   // (mean, rstd) per (sample, group) for the backward pass
        stats[((size_t)n * 32 + blockIdx.y * GN_GPW + tid) * 2 + 0] = gmean[tid];
        stats[((size_t)n * 32 + blockIdx.y * GN_GPW + tid) * 2 + 1] = grstd[tid];
    }
    for (int cc = tid; cc < CW; cc += GN_THREADS) {
        const int ch = cbase + cc;
        const int g = fdiv_small(cc, cg, rcg);
        float A = grstd[g] * gamma[ch];
        float B = beta[ch] - gmean[g] * A;
        if (film) {
            const float* f = film + (size_t)(n / film_div) * film_ld;
            const float sc = 1.0f + f[ch];
            A *= sc;
            B = B * sc + f[C + ch];
        }
        if (coefA) {
            coefA[(size_t)n * C + ch] = A;
            coefB[(size_t)n * C + ch] = B;
        }
        shA[cc] = A;
        shB[cc] = B;
    }
    if (act_out == nullptr) return;
    // materialise act(x*A + B) as ONE contiguous [N*P][C] tensor (the virtual concat becomes a real one): on gfx950
    // the fp32 MFMAs run on the vector ALUs, so a prologue fused into the consuming implicit GEMM - re-evaluated for
    // every tap and every filter tile - sits on the GEMM's critical path; evaluating it once here is cheaper.
    __syncthreads();
    if (active) {
        const f32x4 a4 = ld4(shA + q * 4), b4 = ld4(shB + q * 4);
        if (cached) {
#pragma unroll
            for (int i = 0; i < KEEP; ++i) {
                const int p = pl + i * PL;
                if (p < P) {
                    f32x4 v = keep[i] * a4 + b4;
                    if (act_mode == LFVDM_ACT_SILU) { v.x = silu_f(v.x); v.y = silu_f(v.y); v.z = silu_f(v.z); v.w = silu_f(v.w); }
                    st4(act_out + (pos0 + p) * C + c, v);
                }
            }
        } else {
            for (int p = pl; p < P; p += PL) {
                f32x4 v = ld_cat(s0, s1, C0, C1, pos0 + p, c) * a4 + b4;
                if (act_mode == LFVDM_ACT_SILU) { v.x = silu_f(v.x); v.y = silu_f(v.y); v.z = silu_f(v.z); v.w = silu_f(v.w); }
                st4(act_out + (pos0 + p) * C + c, v);
            }
        }
    }
}

// -------------------------------------------------------------------------------------
// gn_wave: the same GroupNorm for maps of <= 256 positions with 2 / 4 / 8 / 16 channels per group (C = 64 ... 512), ONE
// WAVE per (sample, 16 channels): lane = (pixel lane pl = lane >> 2, channel quad q = lane & 3), the slice
// [P][16 channels] sits in <= 16 float4 per lane, and both reductions are wave butterflies (over the 16 pixel lanes,
// then over the 1 / 2 / 4 quad lanes of a group) - no LDS, no barrier.  The workgroup kernel above spends seven
// barriers and four LDS round trips on 16 KB of data: 5.8 us per launch against ~4 here, 15 launches per denoising step.
// -------------------------------------------------------------------------------------
template <int CG>      // channels per group: 2, 4, 8, 16
__global__ __launch_bounds__(64) void gn_wave_kernel(
    const float* __restrict__ s0, const float* __restrict__ s1, int C0, int C1, int P,
    const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ film, int film_div,
    int film_ld, float eps, float* __restrict__ coefA, float* __restrict__ coefB, float* __restrict__ stats,
    float* __restrict__ act_out, int act_mode, int ldo) {
    gn_wave_body<CG, false>(blockIdx.x, blockIdx.y, threadIdx.x, s0, s1, C0, C1, P, gamma, beta, film, film_div, film_ld, eps, coefA,
                            coefB, stats, act_out, act_mode, ldo);
}

// the same unit shared by the four waves of a workgroup (gn_wave_body, NW = 4): maps of >= 128 positions
template <int CG>
__global__ __launch_bounds__(256) void gn_wave4_kernel(
    const float* __restrict__ s0, const float* __restrict__ s1, int C0, int C1, int P,
    const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ film, int film_div,
    int film_ld, float eps, float* __restrict__ coefA, float* __restrict__ coefB, float* __restrict__ stats,
    float* __restrict__ act_out, int act_mode, int ldo) {
    gn_wave_body<CG, false, 4>(blockIdx.x, blockIdx.y, threadIdx.x & 63, s0, s1, C0, C1, P, gamma, beta, film, film_div, film_ld, eps,
                               coefA, coefB, stats, act_out, act_mode, ldo, __builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
}

// a wave kernel by its group width (2 / 4 / 8 / 16 channels per group: checked by the caller)
#define LFVDM_GN_BY_CG(K, cg, grid, block, s, ...)                                      \
    do {                                                                                \
        if ((cg) == 2) hipLaunchKernelGGL(K<2>, grid, block, 0, s, __VA_ARGS__);        \
        else if ((cg) == 4) hipLaunchKernelGGL(K<4>, grid, block, 0, s, __VA_ARGS__);   \
        else if ((cg) == 8) hipLaunchKernelGGL(K<8>, grid, block, 0, s, __VA_ARGS__);   \
        else hipLaunchKernelGGL(K<16>, grid, block, 0, s, __VA_ARGS__);                 \
    } while (0)

// one wave per (sample, 16 channels) when the map and the group width allow it; false = use the workgroup kernels
inline bool gn_wave_launch(const float* src0, const float* src1, int C0, int C1, int N, int P, const float* gamma,
                           const float* beta, const float* film, int film_div, int film_ld, float eps, float* coefA,
                           float* coefB, float* stats, float* out, int act, hipStream_t s) {
    static const bool off = getenv("LFVDM_GN_NO_WAVE") != nullptr;          // A/B aid
    const int C = C0 + C1, cg = C / 32;
    if (off || P > 256 || C0 % 16 || (cg != 2 && cg != 4 && cg != 8 && cg != 16) || N > 65535) return false;
    const dim3 grid(N, C / 16);
    // four waves per unit on the larger maps (LFVDM_GN_WAVE4_MINP: smallest map that takes it, default 128; 0 = never).
    // Measured at cfg B (12 launches per denoising step, 16x16 maps): 70-74 -> 60-63 us per step, 1157-1160 -> 1170-1175
    // steps/s; eight waves per unit (512 threads, 2 float4 per lane): equal to four, not kept
    static const int minp4 = getenv("LFVDM_GN_WAVE4_MINP") ? atoi(getenv("LFVDM_GN_WAVE4_MINP")) : 128;
    if (minp4 > 0 && P >= minp4 && P % 64 == 0)
        LFVDM_GN_BY_CG(gn_wave4_kernel, cg, grid, dim3(256), s, src0, src1, C0, C1, P, gamma, beta, film, film_div, film_ld, eps,
                       coefA, coefB, stats, out, act, 0);
    else
        LFVDM_GN_BY_CG(gn_wave_kernel, cg, grid, dim3(64), s, src0, src1, C0, C1, P, gamma, beta, film, film_div, film_ld, eps,
                       coefA, coefB, stats, out, act, 0);
    return true;
}

// -------------------------------------------------------------------------------------
// Large maps (P > 8 pixel lanes' worth: pixel space, 32x32 latents): the (sample, 8 groups) decomposition above gives
// N*4 workgroups that each walk their whole slice three times, one load at a time - 80 workgroups streaming 2 MB each at
// 128x128 (1-2 ms per GroupNorm, a third of the pixel-space step).  Here a workgroup owns a CHUNK of 8*PL positions of
// the slice, held in registers:
//   pass 1 (gn_chunk_stats_kernel): exact two-pass (mean, M2) of the chunk per group -> part[n][g][s] = (mean_s, M2_s)
//   pass 2 (gn_chunk_apply_kernel): every workgroup combines the S partials of its 8 groups in a fixed order
//     mean = sum n_s mean_s / n,  M2 = sum (M2_s + n_s (mean_s - mean)^2)      (Chan et al.; as exact as the two-pass)
//   and applies the affine (+FiLM)(+activation) to its chunk, whose loads were issued before the combination.
// Deterministic; x is read twice and written once by thousands of workgroups.
// -------------------------------------------------------------------------------------
constexpr int GN_KEEP = 8;

struct GnChunkGeom { int C0, C1, P, S, PL; };

__device__ __forceinline__ void gn_chunk_load(const float* s0, const float* s1, const GnChunkGeom& g, size_t pos0, int p_first,
                                              int pl, int c, f32x4 (&keep)[GN_KEEP]) {
#pragma unroll
    for (int i = 0; i < GN_KEEP; ++i) {
        const int p = p_first + pl + i * g.PL;
        keep[i] = ld_cat(s0, s1, g.C0, g.C1, pos0 + min(p, g.P - 1), c);
    }
}

__global__ __launch_bounds__(GN_THREADS) void gn_chunk_stats_kernel(const float* __restrict__ s0, const float* __restrict__ s1,
                                                                    GnChunkGeom g, float* __restrict__ part_out) {
    const int C = g.C0 + g.C1, cg = C / 32, CW = GN_GPW * cg, Q = CW / 4, PL = g.PL;
    const float rcg = __builtin_amdgcn_rcpf((float)cg);
    const int sidx = blockIdx.x, n = blockIdx.z, cbase = blockIdx.y * CW;
    const int tid = threadIdx.x;
    const bool active = tid < PL * Q;
    const int q = active ? tid % Q : 0, pl = active ? tid / Q : 0;
    const int c = cbase + q * 4;
    const int p_first = sidx * (GN_KEEP * PL);
    const int npos = min(GN_KEEP * PL, g.P - p_first);
    __shared__ float part[GN_THREADS * 4];
    __shared__ float chs[GN_MAXCW];
    __shared__ float gmean[GN_GPW];
    f32x4 keep[GN_KEEP];
    gn_chunk_load(s0, s1, g, (size_t)n * g.P, p_first, pl, c, keep);
    for (int pass = 0; pass < 2; ++pass) {
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        if (active) {
            f32x4 mu = {0.f, 0.f, 0.f, 0.f};
            if (pass) {
                mu.x = gmean[fdiv_small(q * 4 + 0, cg, rcg)]; mu.y = gmean[fdiv_small(q * 4 + 1, cg, rcg)];
                mu.z = gmean[fdiv_small(q * 4 + 2, cg, rcg)]; mu.w = gmean[fdiv_small(q * 4 + 3, cg, rcg)];
            }
#pragma unroll
            for (int i = 0; i < GN_KEEP; ++i) {
                if (pl + i * PL < npos) {
                    if (pass == 0) { s += keep[i]; } else { const f32x4 v = keep[i] - mu; s += v * v; }
                }
            }
            st4(part + (pl * Q + q) * 4, s);
        }
        __syncthreads();
        for (int cc = tid; cc < CW; cc += GN_THREADS) {
            float t = 0.f;
            for (int i = 0; i < PL; ++i) t += part[i * CW + cc];
            chs[cc] = t;
        }
        __syncthreads();
        if (tid < GN_GPW) {
            float t = 0.f;
            for (int i = 0; i < cg; ++i) t += chs[tid * cg + i];
            float* o = part_out + (((size_t)n * 32 + blockIdx.y * GN_GPW + tid) * g.S + sidx) * 2;
            if (pass == 0) { gmean[tid] = t / (float)(cg * npos); o[0] = gmean[tid]; }
            else o[1] = t;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(GN_THREADS) void gn_chunk_apply_kernel(
    const float* __restrict__ s0, const float* __restrict__ s1, GnChunkGeom g, const float* __restrict__ part_in,
    const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ film, int film_div,
    int film_ld, float eps, float* __restrict__ coefA, float* __restrict__ coefB, float* __restrict__ stats,
    float* __restrict__ act_out, int act_mode) {
    const int C = g.C0 + g.C1, cg = C / 32, CW = GN_GPW * cg, Q = CW / 4, PL = g.PL;
    const float rcg = __builtin_amdgcn_rcpf((float)cg);
    const int sidx = blockIdx.x, n = blockIdx.z, cbase = blockIdx.y * CW;
    const int tid = threadIdx.x;
    const bool active = tid < PL * Q;
    const int q = active ? tid % Q : 0, pl = active ? tid / Q : 0;
    const int c = cbase + q * 4;
    const int PC = GN_KEEP * PL;
    const int p_first = sidx * PC;
    const int npos = min(PC, g.P - p_first);
    __shared__ float gmean[GN_GPW], grstd[GN_GPW];
    __shared__ __attribute__((aligned(16))) float shA[GN_MAXCW], shB[GN_MAXCW];
    f32x4 keep[GN_KEEP];
    gn_chunk_load(s0, s1, g, (size_t)n * g.P, p_first, pl, c, keep);       // in flight during the combination
    {   // 32 lanes per group, fixed summation order
        const int grp = tid >> 5, j = tid & 31;
        const float* pp = part_in + ((size_t)n * 32 + blockIdx.y * GN_GPW + grp) * g.S * 2;
        float sm = 0.f;
        for (int s = j; s < g.S; s += 32) sm += (float)(cg * min(PC, g.P - s * PC)) * pp[2 * s];
        for (int o = 16; o > 0; o >>= 1) sm += __shfl_xor(sm, o, 64);
        const float ntot = (float)cg * (float)g.P;
        const float mean = sm / ntot;
        float m2 = 0.f;
        for (int s = j; s < g.S; s += 32) {
            const float d = pp[2 * s] - mean;
            m2 += pp[2 * s + 1] + (float)(cg * min(PC, g.P - s * PC)) * d * d;
        }
        for (int o = 16; o > 0; o >>= 1) m2 += __shfl_xor(m2, o, 64);
        if (j == 0) {
            gmean[grp] = mean;
            grstd[grp] = 1.0f / sqrtf(m2 / ntot + eps);
        }
    }
    __syncthreads();
    if (stats && sidx == 0 && tid < GN_GPW) {
        stats[((size_t)n * 32 + blockIdx.y * GN_GPW + tid) * 2 + 0] = gmean[tid];
        stats[((size_t)n * 32 + blockIdx.y * GN_GPW + tid) * 2 + 1] = grstd[tid];
    }
    for (int cc = tid; cc < CW; cc += GN_THREADS) {
        const int ch = cbase + cc;
        const int gi = fdiv_small(cc, cg, rcg);
        float A = grstd[gi] * gamma[ch];
        float B = beta[ch] - gmean[gi] * A;
        if (film) {
            const float* f = film + (size_t)(n / film_div) * film_ld;
            const float sc = 1.0f + f[ch];
            A *= sc;
            B = B * sc + f[C + ch];
        }
        if (coefA && sidx == 0) {
            coefA[(size_t)n * C + ch] = A;
            coefB[(size_t)n * C + ch] = B;
        }
        shA[cc] = A;
        shB[cc] = B;
    }
    if (act_out == nullptr) return;
    __syncthreads();
    if (active) {
        const f32x4 a4 = ld4(shA + q * 4), b4 = ld4(shB + q * 4);
        const size_t pos0 = (size_t)n * g.P + p_first;
#pragma unroll
        for (int i = 0; i < GN_KEEP; ++i) {
            const int p = pl + i * PL;
            if (p < npos) {
                f32x4 v = keep[i] * a4 + b4;
                if (act_mode == LFVDM_ACT_SILU) { v.x = silu_f(v.x); v.y = silu_f(v.y); v.z = silu_f(v.z); v.w = silu_f(v.w); }
                st4(act_out + (pos0 + p) * C + c, v);
            }
        }
    }
}

// does the slice need (and fit) the 16-float4 register budget of the single-launch kernel?
inline bool gn_keep16(int C, int P) {
    const int PL = GN_THREADS / (GN_GPW * (C / 32) / 4);
    return P > 8 * PL && P <= 16 * PL;
}

// chunked decomposition for (C, P): chunks per slice (0 = the single-launch kernel holds the slice in registers)
inline int gn_chunks(int C, int P, int* pl_out) {
    const int Q = GN_GPW * (C / 32) / 4;
    const int PL = GN_THREADS / Q;
    if (pl_out) *pl_out = PL;
    if (P <= 2 * GN_KEEP * PL) return 0;       // up to 16 float4 per thread: the single-launch kernel keeps the slice
    return (P + GN_KEEP * PL - 1) / (GN_KEEP * PL);
}

// Every refusal of the spatial forward, before anything is launched.  need_out: the entry materialises act(x*A + B) and
// must be given `out`; a coefficients-only entry must be given coefA / coefB or stats.
inline int gn_fwd_check(const float* src0, const float* src1, int C0, int C1, int N, int P, const float* gamma, const float* beta,
                        const float* film, int film_div, bool need_out, const float* out, const float* coefA, const float* coefB,
                        const float* stats) {
    const int C = C0 + C1;
    if (N <= 0 || P <= 0 || C <= 0 || C % 32 || C0 % 4 || C > 1024) return LFVDM_E_SHAPE;
    if (!src0 || !gamma || !beta || (C1 > 0 && !src1)) return LFVDM_E_SHAPE;
    if ((film && film_div <= 0) || (coefA == nullptr) != (coefB == nullptr)) return LFVDM_E_SHAPE;
    if (need_out ? !out : (!coefA && !stats)) return LFVDM_E_SHAPE;
    return LFVDM_OK;
}

// The single-launch forward: one wave per (sample, 16 channels) where gn_wave_launch takes the shape, else a workgroup per
// (sample, 8 groups) with the register budget the slice needs.  out = NULL: coefficients / statistics only.
inline int gn_fwd_launch(const float* src0, const float* src1, int C0, int C1, int N, int P, const float* gamma,
                         const float* beta, const float* film, int film_div, int film_ld, float eps, float* out, int act,
                         float* coefA, float* coefB, float* stats, hipStream_t s) {
    if (!gn_wave_launch(src0, src1, C0, C1, N, P, gamma, beta, film, film_div, film_ld, eps, coefA, coefB, stats, out, act, s)) {
        const auto kernel = gn_keep16(C0 + C1, P) ? gn_coef_kernel<16> : gn_coef_kernel<8>;
        hipLaunchKernelGGL(kernel, dim3(N, 32 / GN_GPW), dim3(GN_THREADS), 0, s, src0, src1, C0, C1, P, gamma, beta, film, film_div,
                           film_ld, eps, coefA, coefB, stats, out, act);
    }
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}

// -------------------------------------------------------------------------------------
// gn_temporal: one wave per (b, pixel); the sample is [T][C] with row stride P*C.
// Writes the normalised rows (they are also the residual of the attention block).
// -------------------------------------------------------------------------------------
constexpr int GT_MAXC = 512;

__global__ __launch_bounds__(256) void gn_temporal_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float eps,
                                                          float* __restrict__ y, int B, int T, int P, int C) {
    __shared__ float chs_all[4][GT_MAXC];
    __shared__ float gstat_all[4][64];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const long sample = (long)blockIdx.x * 4 + wave;
    if (sample >= (long)B * P) return;  // whole wave exits together
    float* chs = chs_all[wave];
    float* gstat = gstat_all[wave];
    const int b = (int)(sample / P), p = (int)(sample % P);
    const int cg = C / 32;
    const float rcg = __builtin_amdgcn_rcpf((float)cg);
    const int Q = C / 4;
    const size_t base = ((size_t)b * T * P + p) * C;
    const size_t tstride = (size_t)P * C;
    const int E = T * Q;

    // lane layout: QL lanes along the channel quads, TL lanes along the frames (TL > 1 only when
    // the quads of one frame fill less than a wave); per-channel sums are combined with shuffles,
    // so the result is deterministic (no LDS atomics).
    const int TL = (Q <= 64 && 64 % Q == 0) ? 64 / Q : 1;
    const int QL = 64 / TL;
    const int ql = lane % QL, tl = lane / QL;
    for (int pass = 0; pass < 2; ++pass) {
        for (int q = ql; q < Q; q += QL) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f};
            f32x4 mu = {0.f, 0.f, 0.f, 0.f};
            if (pass) {
                mu.x = gstat[fdiv_small(q * 4 + 0, cg, rcg)]; mu.y = gstat[fdiv_small(q * 4 + 1, cg, rcg)];
                mu.z = gstat[fdiv_small(q * 4 + 2, cg, rcg)]; mu.w = gstat[fdiv_small(q * 4 + 3, cg, rcg)];
            }
            for (int t = tl; t < T; t += TL) {
                f32x4 v = ld4(x + base + t * tstride + q * 4);
                if (pass) { v = v - mu; s += v * v; } else { s += v; }
            }
            for (int o = QL; o < 64; o <<= 1) {
                s.x += __shfl_xor(s.x, o, 64); s.y += __shfl_xor(s.y, o, 64);
                s.z += __shfl_xor(s.z, o, 64); s.w += __shfl_xor(s.w, o, 64);
            }
            if (tl == 0) st4(chs + q * 4, s);
        }
        wave_lds_fence();
        if (lane < 32) {
            float t = 0.f;
            for (int i = 0; i < cg; ++i) t += chs[lane * cg + i];
            const float inv = 1.0f / (float)(cg * T);
            if (pass == 0) gstat[lane] = t * inv;
            else gstat[32 + lane] = 1.0f / sqrtf(t * inv + eps);
        }
        wave_lds_fence();
    }
    for (int e = lane; e < E; e += 64) {
        const int t = e / Q, q = e - t * Q;
        f32x4 v = ld4(x + base + t * tstride + q * 4);
        const f32x4 ga = ld4(gamma + q * 4), be = ld4(beta + q * 4);
        f32x4 o;
        o.x = (v.x - gstat[fdiv_small(q * 4 + 0, cg, rcg)]) * gstat[32 + fdiv_small(q * 4 + 0, cg, rcg)] * ga.x + be.x;
        o.y = (v.y - gstat[fdiv_small(q * 4 + 1, cg, rcg)]) * gstat[32 + fdiv_small(q * 4 + 1, cg, rcg)] * ga.y + be.y;
        o.z = (v.z - gstat[fdiv_small(q * 4 + 2, cg, rcg)]) * gstat[32 + fdiv_small(q * 4 + 2, cg, rcg)] * ga.z + be.z;
        o.w = (v.w - gstat[fdiv_small(q * 4 + 3, cg, rcg)]) * gstat[32 + fdiv_small(q * 4 + 3, cg, rcg)] * ga.w + be.w;
        st4(y + base + t * tstride + q * 4, o);
    }
}

// Register-resident variant for C <= 256 (the channel quads of a frame fit one wave): the (b, pixel) sample - T x C
// floats, <= TIT float4 per lane - is read ONCE and both statistic passes and the normalisation run on registers
// (the kernel above reads it three times from L2, each pass a dependent round trip).  Same lane layout and same
// summation order as above: bitwise the same result.
template <int TIT>
__global__ __launch_bounds__(256) void gn_temporal_reg_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float eps,
                                                              float* __restrict__ y, int B, int T, int P, int C) {
    __shared__ float chs_all[4][256];
    __shared__ float gstat_all[4][64];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const long sample = (long)blockIdx.x * 4 + wave;
    if (sample >= (long)B * P) return;  // whole wave exits together
    float* chs = chs_all[wave];
    float* gstat = gstat_all[wave];
    const int b = (int)(sample / P), p = (int)(sample % P);
    const int cg = C / 32;
    const float rcg = __builtin_amdgcn_rcpf((float)cg);
    const int Q = C / 4;                 // <= 64, divides 64
    const size_t base = ((size_t)b * T * P + p) * C;
    const size_t tstride = (size_t)P * C;
    const int TL = 64 / Q;
    const int q = lane % Q, tl = lane / Q;
    f32x4 keep[TIT];
#pragma unroll
    for (int i = 0; i < TIT; ++i) {
        const int t = tl + i * TL;
        keep[i] = t < T ? ld4(x + base + t * tstride + q * 4) : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    f32x4 mu = {0.f, 0.f, 0.f, 0.f}, rs = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < TIT; ++i) {
            if (tl + i * TL < T) {
                if (pass) { const f32x4 v = keep[i] - mu; s += v * v; } else { s += keep[i]; }
            }
        }
        for (int o = Q; o < 64; o <<= 1) {
            s.x += __shfl_xor(s.x, o, 64); s.y += __shfl_xor(s.y, o, 64);
            s.z += __shfl_xor(s.z, o, 64); s.w += __shfl_xor(s.w, o, 64);
        }
        if (tl == 0) st4(chs + q * 4, s);
        wave_lds_fence();
        if (lane < 32) {
            float t = 0.f;
            for (int i = 0; i < cg; ++i) t += chs[lane * cg + i];
            const float inv = 1.0f / (float)(cg * T);
            if (pass == 0) gstat[lane] = t * inv;
            else gstat[32 + lane] = 1.0f / sqrtf(t * inv + eps);
        }
        wave_lds_fence();
        if (pass == 0) {
            mu.x = gstat[fdiv_small(q * 4 + 0, cg, rcg)]; mu.y = gstat[fdiv_small(q * 4 + 1, cg, rcg)];
            mu.z = gstat[fdiv_small(q * 4 + 2, cg, rcg)]; mu.w = gstat[fdiv_small(q * 4 + 3, cg, rcg)];
        } else {
            rs.x = gstat[32 + fdiv_small(q * 4 + 0, cg, rcg)]; rs.y = gstat[32 + fdiv_small(q * 4 + 1, cg, rcg)];
            rs.z = gstat[32 + fdiv_small(q * 4 + 2, cg, rcg)]; rs.w = gstat[32 + fdiv_small(q * 4 + 3, cg, rcg)];
        }
    }
    const f32x4 ga = ld4(gamma + q * 4), be = ld4(beta + q * 4);
#pragma unroll
    for (int i = 0; i < TIT; ++i) {
        const int t = tl + i * TL;
        if (t < T) {
            f32x4 o;
            o.x = (keep[i].x - mu.x) * rs.x * ga.x + be.x;
            o.y = (keep[i].y - mu.y) * rs.y * ga.y + be.y;
            o.z = (keep[i].z - mu.z) * rs.z * ga.z + be.z;
            o.w = (keep[i].w - mu.w) * rs.w * ga.w + be.w;
            st4(y + base + t * tstride + q * 4, o);
        }
    }
}

}  // namespace

extern "C" int lfvdm_gn_coef(const float* src0, const float* src1, int C0, int C1, int N, int P, const float* gamma,
                             const float* beta, const float* film, int film_div, int film_ld, float eps, float* coefA,
                             float* coefB, void* stream) {
    return lfvdm_gn_coef_stats(src0, src1, C0, C1, N, P, gamma, beta, film, film_div, film_ld, eps, coefA, coefB, nullptr,
                               stream);
}

extern "C" int lfvdm_gn_coef_stats(const float* src0, const float* src1, int C0, int C1, int N, int P, const float* gamma,
                                   const float* beta, const float* film, int film_div, int film_ld, float eps,
                                   float* coefA, float* coefB, float* stats, void* stream) {
    if (int rc = gn_fwd_check(src0, src1, C0, C1, N, P, gamma, beta, film, film_div, false, nullptr, coefA, coefB, stats)) return rc;
    return gn_fwd_launch(src0, src1, C0, C1, N, P, gamma, beta, film, film_div, film_ld, eps, nullptr, 0, coefA, coefB, stats,
                         (hipStream_t)stream);
}

extern "C" int lfvdm_gn_apply(const float* src0, const float* src1, int C0, int C1, int N, int P, const float* gamma,
                              const float* beta, const float* film, int film_div, int film_ld, float eps, int act,
                              float* out, float* coefA, float* coefB, float* stats, void* stream) {
    if (int rc = gn_fwd_check(src0, src1, C0, C1, N, P, gamma, beta, film, film_div, true, out, coefA, coefB, stats)) return rc;
    return gn_fwd_launch(src0, src1, C0, C1, N, P, gamma, beta, film, film_div, film_ld, eps, out, act, coefA, coefB, stats,
                         (hipStream_t)stream);
}

extern "C" int lfvdm_gn_apply_part(const float* src, int C, int N, int P, int cg, const float* gamma, const float* beta, float eps,
                                   int act, float* out, int ldo, void* stream) {
    if (!src || !gamma || !beta || !out || N <= 0 || N > 65535 || P <= 0 || P > 256 || C <= 0 || C % 16 || ldo < C || ldo % 4)
        return LFVDM_E_SHAPE;
    if ((cg != 2 && cg != 4 && cg != 8 && cg != 16) || C % cg) return LFVDM_E_UNSUPPORTED;
    LFVDM_GN_BY_CG(gn_wave_kernel, cg, dim3(N, C / 16), dim3(64), (hipStream_t)stream, src, (const float*)nullptr, C, 0, P, gamma,
                   beta, (const float*)nullptr, 1, 0, eps, (float*)nullptr, (float*)nullptr, (float*)nullptr, out, act, ldo);
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}

extern "C" long lfvdm_gn_apply_ws_floats(int C, int N, int P) {
    if (C <= 0 || C % 32 || C > 1024 || N <= 0 || P <= 0) return 0;
    const int S = gn_chunks(C, P, nullptr);
    return (long)N * 32 * S * 2;
}

extern "C" int lfvdm_gn_apply_ws(const float* src0, const float* src1, int C0, int C1, int N, int P, const float* gamma,
                                 const float* beta, const float* film, int film_div, int film_ld, float eps, int act,
                                 float* out, float* coefA, float* coefB, float* stats, float* ws, long ws_floats, void* stream) {
    if (int rc = gn_fwd_check(src0, src1, C0, C1, N, P, gamma, beta, film, film_div, true, out, coefA, coefB, stats)) return rc;
    int PL = 0;
    const int S = gn_chunks(C0 + C1, P, &PL);
    if (S == 0)
        return gn_fwd_launch(src0, src1, C0, C1, N, P, gamma, beta, film, film_div, film_ld, eps, out, act, coefA, coefB, stats,
                             (hipStream_t)stream);
    if (!ws || ws_floats < (long)N * 32 * S * 2 || N > 65535) return LFVDM_E_SHAPE;
    const GnChunkGeom g = {C0, C1, P, S, PL};
    const dim3 grid(S, 32 / GN_GPW, N);
    hipLaunchKernelGGL(gn_chunk_stats_kernel, grid, dim3(GN_THREADS), 0, (hipStream_t)stream, src0, src1, g, ws);
    LFVDM_CHECK_LAUNCH();
    hipLaunchKernelGGL(gn_chunk_apply_kernel, grid, dim3(GN_THREADS), 0, (hipStream_t)stream, src0, src1, g, (const float*)ws,
                       gamma, beta, film, film_div, film_ld, eps, coefA, coefB, stats, out, act);
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}

// The temporal form (gn_temporal_kernel / gn_temporal_reg_kernel).
extern "C" int lfvdm_gn_temporal(const float* x, const float* gamma, const float* beta, float eps, float* y, int B, int T,
                                 int P, int C, void* stream) {
    if (B <= 0 || T <= 0 || P <= 0 || C <= 0 || C % 32 || C > GT_MAXC) return LFVDM_E_SHAPE;
    const long samples = (long)B * P;
    const dim3 grid((unsigned)((samples + 3) / 4));
    const int Q = C / 4;
    if (Q <= 64 && 64 % Q == 0) {           // register-resident sample: frames per lane = ceil(T / (64 / Q))
        const int per_lane = (T + 64 / Q - 1) / (64 / Q);
        hipStream_t s = (hipStream_t)stream;
        if (per_lane <= 8) {
            hipLaunchKernelGGL(gn_temporal_reg_kernel<8>, grid, dim3(256), 0, s, x, gamma, beta, eps, y, B, T, P, C);
            LFVDM_CHECK_LAUNCH();
            return LFVDM_OK;
        }
        if (per_lane <= 16) {
            hipLaunchKernelGGL(gn_temporal_reg_kernel<16>, grid, dim3(256), 0, s, x, gamma, beta, eps, y, B, T, P, C);
            LFVDM_CHECK_LAUNCH();
            return LFVDM_OK;
        }
        if (per_lane <= 32) {
            hipLaunchKernelGGL(gn_temporal_reg_kernel<32>, grid, dim3(256), 0, s, x, gamma, beta, eps, y, B, T, P, C);
            LFVDM_CHECK_LAUNCH();
            return LFVDM_OK;
        }
    }
    hipLaunchKernelGGL(gn_temporal_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, gamma, beta, eps, y, B, T, P, C);
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}
