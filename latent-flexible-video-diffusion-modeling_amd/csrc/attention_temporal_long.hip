// Temporal attention with relative position terms (reference rpe.py:143-169) for LONG windows, 33 <= T <= 64 frames.
//
//   logits[t][s] = q_t . (k_s + R_k[t][s]) + scale * k_s . R_q[s][t]     (q scaled)
//   o[t]         = sum_s softmax_s(logits + two-clique mask)[s] * (v_s + R_v[t][s])
//
// The T <= 32 kernels (attention.hip, attention_temporal2.hip, attention_bwd.hip) stage whole [T][T] R slices per
// workgroup; at 64 frames one slice chunk alone exceeds the LDS.  Here a workgroup owns one (b, head), a GROUP of
// TL_TG = 16 query frames and a strip of TL_NPX = 16 pixels; lane = (pixel j, frame tq) with 4 pixels x 16 frames
// per wave.  The head dim is walked in chunks of TL_FC = 8 channels (any F that is a multiple of 8): per chunk the
// workgroup stages
//   Ra [TG][T*FC]  R_k (logit phases) / R_v (PV phases) rows of its query frames     - shared by the 16 pixels
//   Rb [TG][T*FC]  R_q transposed (row tq holds R_q[s][t0 + tq] for every s)        - shared by the 16 pixels
//   KV [NPX][T*FC] k (logit phases) / v (PV phases) of its pixels over all T frames - shared by the 16 query frames
// = 48 rows of T*FC + 4 floats (99 KB at T = 64).  A lane keeps all T logits in registers (as the T <= 32 kernels do),
// so the softmax needs no cross-lane step and the result is the same two-pass softmax as the short kernels, not an
// online rescaling.  The global loads of phase i + 1 are issued into registers before phase i computes.
//
// Backward (same decomposition as attention_bwd.hip; the dR kernel there covers ceil(T / 16) row tiles):
//   rows: lane = (pixel, query frame t): logits, dP, softmax, dS; writes the P / dS rows [B][P][heads][T][T], dq.
//   cols: lane = (pixel, key frame s):   dk[s] = scale * sum_t dS[t][s] (q_t + R_q[s][t]),  dv[s] = sum_t P[t][s] dO_t.
// No atomics: bitwise reproducible (deterministic mode needs nothing extra).
#include <hip/hip_runtime.h>

#include "attention_temporal.h"
#include "common_hip.h"
#include "lfvdm_hip.h"

namespace {

constexpr int TL_TG = 16;      // query (rows, forward) or key (cols) frames per workgroup
constexpr int TL_PPW = 4;      // pixels per wave (64 lanes = 4 pixels x 16 frames)
constexpr int TL_NPX = 16;     // pixels per workgroup
constexpr int TL_FC = 8;       // channels per staged chunk
constexpr int TL_NQ = TL_FC / 4;
constexpr int TL_RB = (TL_TG * TEMPORAL_MAXT_LONG * TL_NQ + 255) / 256;    // float4 per thread per R image
constexpr int TL_KB = (TL_NPX * TEMPORAL_MAXT_LONG * TL_NQ + 255) / 256;   // float4 per thread per pixel image

struct TLGeom {
    int T, P, C, heads, F, NC, NG;    // NC = F / FC chunks, NG = frame groups
};

struct TLStage {
    f32x4 ra[TL_RB], rb[TL_RB], kv[TL_KB], kv2[TL_KB];
};

// workgroup -> (b, head, frame group, pixel strip); lane -> (pixel j, frame tq)
struct TLPos {
    int b, h, t0, p0, j, tq;
};
__device__ __forceinline__ TLPos tl_pos(const TLGeom& g) {
    TLPos r;
    r.b = blockIdx.z;
    r.h = blockIdx.y;
    const int tg = blockIdx.x % g.NG;
    r.t0 = tg * TL_TG;
    r.p0 = (blockIdx.x / g.NG) * TL_NPX;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    r.j = wave * TL_PPW + lane / TL_TG;
    r.tq = lane % TL_TG;
    return r;
}

// Per-thread staging slots of the R images (image row = one of the workgroup's frames a, column = frame c: source row
// a * T + c, or c * T + a for the transposed R_q image) and of the pixel image (rows = pixels, columns = all T frames).
// Slots past the end are not committed; slots of frames / pixels past T / P are committed as zeros.
struct TLSlots {
    int r_g[TL_RB], r_t[TL_RB], r_l[TL_RB], k_g[TL_KB], k_l[TL_KB];
    unsigned r_ok, r_in, k_ok, k_in;
};
__device__ __forceinline__ void tl_slots(const TLGeom& g, int a0, int p0, int b, TLSlots& sl) {
    const int T = g.T, RST = T * TL_FC + 4;
    const float rT = 1.0f / (float)T;
    const int tid = threadIdx.x;
    sl.r_ok = sl.r_in = sl.k_ok = sl.k_in = 0;
#pragma unroll
    for (int i = 0; i < TL_RB; ++i) {
        const int e = tid + 256 * i;
        const int u = e % TL_NQ, ts = e / TL_NQ;
        const int aq = fdiv_small(ts, T, rT), c = ts - aq * T;
        const bool ok = e < TL_TG * T * TL_NQ, in = ok && a0 + aq < T;
        sl.r_ok |= ok ? (1u << i) : 0u;
        sl.r_in |= in ? (1u << i) : 0u;
        sl.r_g[i] = in ? (a0 + aq) * T + c : 0;       // R row (frame a0 + aq, frame c)
        sl.r_t[i] = in ? c * T + a0 + aq : 0;         // transposed R row (frame c, frame a0 + aq)
        sl.r_l[i] = aq * RST + c * TL_FC + 4 * u;
    }
#pragma unroll
    for (int i = 0; i < TL_KB; ++i) {
        const int e = tid + 256 * i;
        const int u = e % TL_NQ, js = e / TL_NQ;
        const int jj = fdiv_small(js, T, rT), s = js - jj * T;
        const bool ok = e < TL_NPX * T * TL_NQ, in = ok && p0 + jj < g.P;
        sl.k_ok |= ok ? (1u << i) : 0u;
        sl.k_in |= in ? (1u << i) : 0u;
        sl.k_g[i] = in ? (b * T + s) * g.P + p0 + jj : 0;    // token row
        sl.k_l[i] = jj * RST + s * TL_FC + 4 * u;
    }
}

// channel offset 4u of a slot (the same for R and pixel slots: u = e % NQ)
__device__ __forceinline__ int tl_u4(int i) { return 4 * ((threadIdx.x + 256 * i) % TL_NQ); }

// ================================================================================================ forward
__global__ __launch_bounds__(256)
void attn_tlong_fwd_kernel(const float* __restrict__ qkv, const float* __restrict__ Rq, const float* __restrict__ Rk,
                           const float* __restrict__ Rv, const float* __restrict__ mask, float* __restrict__ o,
                           float* __restrict__ attn_out, RSel rsel, TLGeom g) {
    extern __shared__ __attribute__((aligned(16))) float tl_smem[];
    const int T = g.T, P = g.P, C = g.C, heads = g.heads, F = g.F, NC = g.NC;
    const int RST = T * TL_FC + 4;
    float* Ra = tl_smem;                  // [TG][RST]
    float* Rb = Ra + TL_TG * RST;         // [TG][RST]
    float* KV = Rb + TL_TG * RST;         // [NPX][RST]
    const TLPos ps = tl_pos(g);
    const int b = ps.b, h = ps.h, t = ps.t0 + ps.tq, p = ps.p0 + ps.j;
    const bool active = t < T && p < P;
    const float scale = rsqrtf((float)F);
    const size_t ld = (size_t)3 * C;
    const size_t rb = rsel.slice(b, (int)gridDim.z);
    const float* RkB = Rk + rb * T * T * C + h * F;
    const float* RqB = Rq + rb * T * T * C + h * F;
    const float* RvB = Rv + rb * T * T * C + h * F;
    const float* qrow = qkv + ((size_t)(b * T + (active ? t : 0)) * P + (active ? p : 0)) * ld + h * F;

    TLSlots sl;
    tl_slots(g, ps.t0, ps.p0, b, sl);
    int u4[TL_RB > TL_KB ? TL_RB : TL_KB];
#pragma unroll
    for (int i = 0; i < (TL_RB > TL_KB ? TL_RB : TL_KB); ++i) u4[i] = tl_u4(i);

    TLStage st;
    f32x4 qn[TL_NQ];
    // phase ph < NC: logits of chunk ph (R_k, R_q^T, k); ph >= NC: PV of chunk ph - NC (R_v, v)
    auto issue = [&](int ph) {
        const bool lg = ph < NC;
        const int f0 = (lg ? ph : ph - NC) * TL_FC;
        const float* A = (lg ? RkB : RvB) + f0;
#pragma unroll
        for (int i = 0; i < TL_RB; ++i) {
            st.ra[i] = ld4(A + (size_t)sl.r_g[i] * C + u4[i]);
            if (lg) st.rb[i] = ld4(RqB + f0 + (size_t)sl.r_t[i] * C + u4[i]);     // R_q[s][t]
        }
        const float* K = qkv + (lg ? C : 2 * C) + h * F + f0;
#pragma unroll
        for (int i = 0; i < TL_KB; ++i) st.kv[i] = ld4(K + (size_t)sl.k_g[i] * ld + u4[i]);
        if (lg) {
#pragma unroll
            for (int u = 0; u < TL_NQ; ++u) qn[u] = ld4(qrow + f0 + 4 * u);
        }
    };
    auto commit = [&](int ph) {
        const bool lg = ph < NC;
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < TL_RB; ++i)
            if (sl.r_ok & (1u << i)) {
                const bool in = sl.r_in & (1u << i);
                st4(Ra + sl.r_l[i], in ? st.ra[i] : z);
                if (lg) st4(Rb + sl.r_l[i], in ? st.rb[i] : z);
            }
#pragma unroll
        for (int i = 0; i < TL_KB; ++i)
            if (sl.k_ok & (1u << i)) st4(KV + sl.k_l[i], (sl.k_in & (1u << i)) ? st.kv[i] : z);
    };

    float logit[TEMPORAL_MAXT_LONG];
#pragma unroll
    for (int s = 0; s < TEMPORAL_MAXT_LONG; ++s) logit[s] = 0.f;

    issue(0);
    for (int ph = 0; ph < NC; ++ph) {
        __syncthreads();
        commit(ph);
        f32x4 q4[TL_NQ];
#pragma unroll
        for (int u = 0; u < TL_NQ; ++u) q4[u] = qn[u] * scale;
        __syncthreads();
        issue(ph + 1);
        if (active) {
            const float* kr = KV + ps.j * RST;
            const float* rkr = Ra + ps.tq * RST;
            const float* rqr = Rb + ps.tq * RST;
#pragma unroll
            for (int s = 0; s < TEMPORAL_MAXT_LONG; ++s) {
                if (s < T) {
                    float a0 = 0.f, a1 = 0.f;
#pragma unroll
                    for (int u = 0; u < TL_NQ; ++u) {
                        const f32x4 k4 = ld4(kr + s * TL_FC + 4 * u);
                        const f32x4 rk4 = ld4(rkr + s * TL_FC + 4 * u);
                        const f32x4 rq4 = ld4(rqr + s * TL_FC + 4 * u);
                        a0 += q4[u].x * (k4.x + rk4.x) + q4[u].y * (k4.y + rk4.y) + q4[u].z * (k4.z + rk4.z) + q4[u].w * (k4.w + rk4.w);
                        a1 += k4.x * rq4.x + k4.y * rq4.y + k4.z * rq4.z + k4.w * rq4.w;
                    }
                    logit[s] += a0 + a1 * scale;
                }
            }
        }
    }

    // two-clique mask + softmax in registers (the arithmetic of the T <= 32 kernels)
    if (active) {
        const float mt = mask ? mask[b * T + t] : 1.f;
        float mx = -INFINITY;
#pragma unroll
        for (int s = 0; s < TEMPORAL_MAXT_LONG; ++s) {
            float v = -INFINITY;
            if (s < T) {
                v = logit[s];
                if (mask) {
                    const float ms = mask[b * T + s];
                    const float pen = 1.f - (mt * ms + (1.f - mt) * (1.f - ms));
                    v -= (pen == 1.f) ? INFINITY : pen;
                }
            }
            logit[s] = v;
            mx = fmaxf(mx, v);
        }
        float sum = 0.f;
#pragma unroll
        for (int s = 0; s < TEMPORAL_MAXT_LONG; ++s) {
            const float e = (logit[s] == -INFINITY) ? 0.f : __expf(logit[s] - mx);
            logit[s] = e;
            sum += e;
        }
        const float inv = 1.0f / sum;
#pragma unroll
        for (int s = 0; s < TEMPORAL_MAXT_LONG; ++s) logit[s] *= inv;
        if (attn_out) {
            float* ar = attn_out + ((((size_t)b * P + p) * heads + h) * T + t) * T;
#pragma unroll
            for (int s = 0; s < TEMPORAL_MAXT_LONG; ++s)
                if (s < T) ar[s] = logit[s];
        }
    }

    for (int ph = NC; ph < 2 * NC; ++ph) {
        __syncthreads();
        commit(ph);
        __syncthreads();
        if (ph + 1 < 2 * NC) issue(ph + 1);
        if (active) {
            const float* vr = KV + ps.j * RST;
            const float* rvr = Ra + ps.tq * RST;
            f32x4 acc[TL_NQ];
#pragma unroll
            for (int u = 0; u < TL_NQ; ++u) acc[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < TEMPORAL_MAXT_LONG; ++s) {
                if (s < T) {
                    float pr = logit[s];
                    asm volatile("" : "+v"(pr));     // no hoisted broadcast pairs (see attention.hip)
#pragma unroll
                    for (int u = 0; u < TL_NQ; ++u) acc[u] += pr * (ld4(vr + s * TL_FC + 4 * u) + ld4(rvr + s * TL_FC + 4 * u));
                }
            }
            float* orow = o + ((size_t)(b * T + t) * P + p) * C + h * F + (ph - NC) * TL_FC;
#pragma unroll
            for (int u = 0; u < TL_NQ; ++u) st4(orow + 4 * u, acc[u]);
        }
    }
}

// ================================================================================================ backward rows
__global__ __launch_bounds__(256)
void attn_tlong_bwd_rows_kernel(const float* __restrict__ qkv, const float* __restrict__ dO, const float* __restrict__ Rq,
                                const float* __restrict__ Rk, const float* __restrict__ Rv, const float* __restrict__ mask,
                                float* __restrict__ dqkv, float* __restrict__ Pg, float* __restrict__ dSg, TLGeom g) {
    extern __shared__ __attribute__((aligned(16))) float tl_smem[];
    const int T = g.T, P = g.P, C = g.C, heads = g.heads, F = g.F, NC = g.NC;
    const int RST = T * TL_FC + 4;
    float* Ra = tl_smem;
    float* Rb = Ra + TL_TG * RST;
    float* KV = Rb + TL_TG * RST;
    const TLPos ps = tl_pos(g);
    const int b = ps.b, h = ps.h, t = ps.t0 + ps.tq, p = ps.p0 + ps.j;
    const bool active = t < T && p < P;
    const float scale = rsqrtf((float)F);
    const size_t ld = (size_t)3 * C;
    const size_t rofs = (size_t)b * T * T * C + h * F;
    const float* RkB = Rk + rofs;
    const float* RqB = Rq + rofs;
    const float* RvB = Rv + rofs;
    const size_t tok = (size_t)(b * T + (active ? t : 0)) * P + (active ? p : 0);
    const float* qrow = qkv + tok * ld + h * F;
    const float* dorow = dO + tok * C + h * F;

    TLSlots sl;
    tl_slots(g, ps.t0, ps.p0, b, sl);
    int u4[TL_RB > TL_KB ? TL_RB : TL_KB];
#pragma unroll
    for (int i = 0; i < (TL_RB > TL_KB ? TL_RB : TL_KB); ++i) u4[i] = tl_u4(i);

    TLStage st;
    f32x4 qn[TL_NQ];
    // phase kind = ph / NC: 0 logits (R_k, R_q^T, k, q), 1 dP (R_v, v, dO), 2 dq (R_k, k)
    auto issue = [&](int ph) {
        const int kind = ph / NC, f0 = (ph - kind * NC) * TL_FC;
        const float* A = (kind == 1 ? RvB : RkB) + f0;
#pragma unroll
        for (int i = 0; i < TL_RB; ++i) {
            st.ra[i] = ld4(A + (size_t)sl.r_g[i] * C + u4[i]);
            if (kind == 0) st.rb[i] = ld4(RqB + f0 + (size_t)sl.r_t[i] * C + u4[i]);
        }
        const float* K = qkv + (kind == 1 ? 2 * C : C) + h * F + f0;
#pragma unroll
        for (int i = 0; i < TL_KB; ++i) st.kv[i] = ld4(K + (size_t)sl.k_g[i] * ld + u4[i]);
        if (kind < 2) {
            const float* QR = (kind == 1 ? dorow : qrow) + f0;
#pragma unroll
            for (int u = 0; u < TL_NQ; ++u) qn[u] = ld4(QR + 4 * u);
        }
    };
    auto commit = [&](int ph) {
        const bool lg = ph < NC;
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < TL_RB; ++i)
            if (sl.r_ok & (1u << i)) {
                const bool in = sl.r_in & (1u << i);
                st4(Ra + sl.r_l[i], in ? st.ra[i] : z);
                if (lg) st4(Rb + sl.r_l[i], in ? st.rb[i] : z);
            }
#pragma unroll
        for (int i = 0; i < TL_KB; ++i)
            if (sl.k_ok & (1u << i)) st4(KV + sl.k_l[i], (sl.k_in & (1u << i)) ? st.kv[i] : z);
    };

    float pr[TEMPORAL_MAXT_LONG], dp[TEMPORAL_MAXT_LONG];
#pragma unroll
    for (int s = 0; s < TEMPORAL_MAXT_LONG; ++s) {
        pr[s] = 0.f;
        dp[s] = 0.f;
    }

    issue(0);
    for (int ph = 0; ph < 2 * NC; ++ph) {
        __syncthreads();
        commit(ph);
        const bool lg = ph < NC;
        f32x4 q4[TL_NQ];
#pragma unroll
        for (int u = 0; u < TL_NQ; ++u) q4[u] = lg ? qn[u] * scale : qn[u];
        __syncthreads();
        issue(ph + 1);
        if (active) {
            const float* kr = KV + ps.j * RST;
            const float* rar = Ra + ps.tq * RST;
            const float* rbr = Rb + ps.tq * RST;
            if (lg) {
#pragma unroll
                for (int s = 0; s < TEMPORAL_MAXT_LONG; ++s) {
                    if (s < T) {
                        float a0 = 0.f, a1 = 0.f;
#pragma unroll
                        for (int u = 0; u < TL_NQ; ++u) {
                            const f32x4 k4 = ld4(kr + s * TL_FC + 4 * u);
                            const f32x4 rk4 = ld4(rar + s * TL_FC + 4 * u);
                            const f32x4 rq4 = ld4(rbr + s * TL_FC + 4 * u);
                            a0 += q4[u].x * (k4.x + rk4.x) + q4[u].y * (k4.y + rk4.y) + q4[u].z * (k4.z + rk4.z) + q4[u].w * (k4.w + rk4.w);
                            a1 += k4.x * rq4.x + k4.y * rq4.y + k4.z * rq4.z + k4.w * rq4.w;
                        }
                        pr[s] += a0 + a1 * scale;
                    }
                }
            } else {
#pragma unroll
                for (int s = 0; s < TEMPORAL_MAXT_LONG; ++s) {
                    if (s < T) {
                        float a0 = 0.f;
#pragma unroll
                        for (int u = 0; u < TL_NQ; ++u) {
                            const f32x4 v4 = ld4(kr + s * TL_FC + 4 * u);
                            const f32x4 rv4 = ld4(rar + s * TL_FC + 4 * u);
                            a0 += q4[u].x * (v4.x + rv4.x) + q4[u].y * (v4.y + rv4.y) + q4[u].z * (v4.z + rv4.z) + q4[u].w * (v4.w + rv4.w);
                        }
                        dp[s] += a0;
                    }
                }
            }
        }
        if (ph == NC - 1 && active) {
            const float mt = mask ? mask[b * T + t] : 1.f;
            float mx = -INFINITY;
#pragma unroll
            for (int s = 0; s < TEMPORAL_MAXT_LONG; ++s) {
                float v = -INFINITY;
                if (s < T) {
                    v = pr[s];
                    if (mask) {
                        const float ms = mask[b * T + s];
                        const float pen = 1.f - (mt * ms + (1.f - mt) * (1.f - ms));
                        v -= (pen == 1.f) ? INFINITY : pen;
                    }
                }
                pr[s] = v;
                mx = fmaxf(mx, v);
            }
            float sum = 0.f;
#pragma unroll
            for (int s = 0; s < TEMPORAL_MAXT_LONG; ++s) {
                const float e = (pr[s] == -INFINITY) ? 0.f : __expf(pr[s] - mx);
                pr[s] = e;
                sum += e;
            }
            const float inv = 1.0f / sum;
#pragma unroll
            for (int s = 0; s < TEMPORAL_MAXT_LONG; ++s) pr[s] *= inv;
        }
    }
    // dS = P * (dP - sum_s P dP); rows of P and dS to the workspace
    if (active) {
        float dsum = 0.f;
#pragma unroll
        for (int s = 0; s < TEMPORAL_MAXT_LONG; ++s) dsum += pr[s] * dp[s];
        const size_t wid = ((size_t)b * P + p) * heads + h;
        float* prow = Pg + (wid * T + t) * T;
        float* srow = dSg + (wid * T + t) * T;
#pragma unroll
        for (int s = 0; s < TEMPORAL_MAXT_LONG; ++s) {
            dp[s] = pr[s] * (dp[s] - dsum);
            if (s < T) {
                prow[s] = pr[s];
                srow[s] = dp[s];
            }
        }
    }
    // dq[t] = scale * sum_s dS[t][s] (k_s + R_k[t][s])
    for (int ph = 2 * NC; ph < 3 * NC; ++ph) {
        __syncthreads();
        commit(ph);
        __syncthreads();
        if (ph + 1 < 3 * NC) issue(ph + 1);
        if (active) {
            const float* kr = KV + ps.j * RST;
            const float* rkr = Ra + ps.tq * RST;
            f32x4 acc[TL_NQ];
#pragma unroll
            for (int u = 0; u < TL_NQ; ++u) acc[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < TEMPORAL_MAXT_LONG; ++s) {
                if (s < T) {
                    float w = dp[s];
                    asm volatile("" : "+v"(w));
#pragma unroll
                    for (int u = 0; u < TL_NQ; ++u) acc[u] += w * (ld4(kr + s * TL_FC + 4 * u) + ld4(rkr + s * TL_FC + 4 * u));
                }
            }
            float* orow = dqkv + tok * ld + h * F + (ph - 2 * NC) * TL_FC;
#pragma unroll
            for (int u = 0; u < TL_NQ; ++u) st4(orow + 4 * u, acc[u] * scale);
        }
    }
}

// ================================================================================================ backward cols
// lane = (pixel j, key frame s = s0 + sq).  Images: Ra [TG][T*FC] = R_q[s][.] rows of the key frames (R_q[s][t] is
// row s * T + t: no transpose), KV = q rows, KV2 = dO rows of the pixels over all T frames.
__global__ __launch_bounds__(256)
void attn_tlong_bwd_cols_kernel(const float* __restrict__ qkv, const float* __restrict__ dO, const float* __restrict__ Rq,
                                const float* __restrict__ Pg, const float* __restrict__ dSg, float* __restrict__ dqkv, TLGeom g) {
    extern __shared__ __attribute__((aligned(16))) float tl_smem[];
    const int T = g.T, P = g.P, C = g.C, heads = g.heads, F = g.F, NC = g.NC;
    const int RST = T * TL_FC + 4;
    float* Ra = tl_smem;                  // [TG][RST]
    float* KV = Ra + TL_TG * RST;         // [NPX][RST] q
    float* KV2 = KV + TL_NPX * RST;       // [NPX][RST] dO
    const TLPos ps = tl_pos(g);
    const int b = ps.b, h = ps.h, s = ps.t0 + ps.tq, p = ps.p0 + ps.j;
    const bool active = s < T && p < P;
    const float scale = rsqrtf((float)F);
    const size_t ld = (size_t)3 * C;
    const float* RqB = Rq + (size_t)b * T * T * C + h * F;

    TLSlots sl;
    tl_slots(g, ps.t0, ps.p0, b, sl);
    int u4[TL_RB > TL_KB ? TL_RB : TL_KB];
#pragma unroll
    for (int i = 0; i < (TL_RB > TL_KB ? TL_RB : TL_KB); ++i) u4[i] = tl_u4(i);

    // column s of this pixel's P and dS matrices
    float pc[TEMPORAL_MAXT_LONG], dc[TEMPORAL_MAXT_LONG];
    {
        const size_t wid = active ? ((size_t)b * P + p) * heads + h : 0;
        const float* pcol = Pg + wid * T * T + (active ? s : 0);
        const float* scol = dSg + wid * T * T + (active ? s : 0);
#pragma unroll
        for (int t = 0; t < TEMPORAL_MAXT_LONG; ++t) {
            pc[t] = (active && t < T) ? pcol[(size_t)t * T] : 0.f;
            dc[t] = (active && t < T) ? scol[(size_t)t * T] : 0.f;
        }
    }

    TLStage st;
    auto issue = [&](int ch) {
        const int f0 = ch * TL_FC;
#pragma unroll
        for (int i = 0; i < TL_RB; ++i) st.ra[i] = ld4(RqB + f0 + (size_t)sl.r_g[i] * C + u4[i]);
#pragma unroll
        for (int i = 0; i < TL_KB; ++i) {
            st.kv[i] = ld4(qkv + h * F + f0 + (size_t)sl.k_g[i] * ld + u4[i]);
            st.kv2[i] = ld4(dO + h * F + f0 + (size_t)sl.k_g[i] * C + u4[i]);
        }
    };
    auto commit = [&]() {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < TL_RB; ++i)
            if (sl.r_ok & (1u << i)) st4(Ra + sl.r_l[i], (sl.r_in & (1u << i)) ? st.ra[i] : z);
#pragma unroll
        for (int i = 0; i < TL_KB; ++i)
            if (sl.k_ok & (1u << i)) {
                const bool in = sl.k_in & (1u << i);
                st4(KV + sl.k_l[i], in ? st.kv[i] : z);
                st4(KV2 + sl.k_l[i], in ? st.kv2[i] : z);
            }
    };

    issue(0);
    for (int ch = 0; ch < NC; ++ch) {
        __syncthreads();
        commit();
        __syncthreads();
        if (ch + 1 < NC) issue(ch + 1);
        if (active) {
            const float* qr = KV + ps.j * RST;
            const float* dr = KV2 + ps.j * RST;
            const float* rq = Ra + ps.tq * RST;
            f32x4 accK[TL_NQ], accV[TL_NQ];
#pragma unroll
            for (int u = 0; u < TL_NQ; ++u) {
                accK[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
                accV[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int t = 0; t < TEMPORAL_MAXT_LONG; ++t) {
                if (t < T) {
                    float wk = dc[t], wv = pc[t];
                    asm volatile("" : "+v"(wk), "+v"(wv));
#pragma unroll
                    for (int u = 0; u < TL_NQ; ++u) {
                        accK[u] += wk * (ld4(qr + t * TL_FC + 4 * u) + ld4(rq + t * TL_FC + 4 * u));
                        accV[u] += wv * ld4(dr + t * TL_FC + 4 * u);
                    }
                }
            }
            float* orow = dqkv + ((size_t)(b * T + s) * P + p) * ld + h * F + ch * TL_FC;
#pragma unroll
            for (int u = 0; u < TL_NQ; ++u) {
                st4(orow + C + 4 * u, accK[u] * scale);
                st4(orow + 2 * C + 4 * u, accV[u]);
            }
        }
    }
}

TLGeom tl_geom(int T, int P, int C, int heads) {
    TLGeom g;
    g.T = T; g.P = P; g.C = C; g.heads = heads;
    g.F = C / heads;
    g.NC = g.F / TL_FC;
    g.NG = (T + TL_TG - 1) / TL_TG;
    return g;
}

dim3 tl_grid(const TLGeom& g, int B) {
    return dim3((unsigned)(g.NG * ((g.P + TL_NPX - 1) / TL_NPX)), (unsigned)g.heads, (unsigned)B);
}

size_t tl_lds(int T) { return (size_t)(2 * TL_TG + TL_NPX) * (T * TL_FC + 4) * sizeof(float); }

bool tl_covered(int T, int C, int heads) {
    return T > TEMPORAL_MAXT && T <= TEMPORAL_MAXT_LONG && (C / heads) % TL_FC == 0;
}

}  // namespace

// The long-window entries of attention_temporal.h: lfvdm_attn_temporal_ring (attention.hip) and lfvdm_attn_temporal_bwd
// (attention_bwd.hip) come here for 33 <= T <= 64.
int lfvdm_attn_temporal_long(const TemporalFwd& a) {
    if (!tl_covered(a.T, a.C, a.heads)) return LFVDM_E_UNSUPPORTED;
    const TLGeom g = tl_geom(a.T, a.P, a.C, a.heads);
    const size_t lds = tl_lds(a.T);
    static DynLdsLimit limit;
    if (int rc = limit.ensure(reinterpret_cast<const void*>(&attn_tlong_fwd_kernel), lds)) return rc;
    hipLaunchKernelGGL(attn_tlong_fwd_kernel, tl_grid(g, a.B), dim3(256), lds, a.s, a.qkv, a.Rq, a.Rk, a.Rv, a.mask, a.o, a.attn_out,
                       a.rsel, g);
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}

int lfvdm_attn_temporal_long_bwd(const TemporalBwd& a) {
    if (!tl_covered(a.T, a.C, a.heads)) return LFVDM_E_UNSUPPORTED;
    const TLGeom g = tl_geom(a.T, a.P, a.C, a.heads);
    const size_t lds = tl_lds(a.T);
    static DynLdsLimit limit_rows, limit_cols;
    if (int rc = limit_rows.ensure(reinterpret_cast<const void*>(&attn_tlong_bwd_rows_kernel), lds)) return rc;
    if (int rc = limit_cols.ensure(reinterpret_cast<const void*>(&attn_tlong_bwd_cols_kernel), lds)) return rc;
    const dim3 grid = tl_grid(g, a.B);
    hipLaunchKernelGGL(attn_tlong_bwd_rows_kernel, grid, dim3(256), lds, a.s, a.qkv, a.d_o, a.Rq, a.Rk, a.Rv, a.mask, a.dqkv, a.ws_p,
                       a.ws_ds, g);
    LFVDM_CHECK_LAUNCH();
    hipLaunchKernelGGL(attn_tlong_bwd_cols_kernel, grid, dim3(256), lds, a.s, a.qkv, a.d_o, a.Rq, a.ws_p, a.ws_ds, a.dqkv, g);
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}
