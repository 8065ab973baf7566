// The fused AdamW + EMA kernel, shared by lfvdm_adamw_ema (optim.hip) and lfvdm_adamw_ema_clip (grad_clip.hip).
// CLIP = false is the launch as it has always been (gradient scaled by a.grad_scale, squared norm accumulated into
// a.grad_sqsum); CLIP = true reads the clip record of lfvdm_grad_norm_finalize: the gradient is scaled by
// a.grad_scale * stat[1], a non-zero stat[2] turns the launch into a no-op, a.grad_sqsum is not touched.
#pragma once
#include "common_hip.h"

namespace {

// the extra kernel argument of the clipping instance: the record of lfvdm_grad_norm_finalize.  Empty otherwise: the
// plain instance compiles to the instructions it has always had.
template <bool CLIP> struct ClipStat {
    const float* p;
    __device__ const float* stat() const { return p; }
};
template <> struct ClipStat<false> {
    __device__ const float* stat() const { return nullptr; }
};

// what the gradient is multiplied by first: a.grad_scale, times the clip coefficient in the clipping instance
template <bool CLIP>
__device__ __forceinline__ float grad_scale_of(const lfvdm_adamw_args& a, float coef) {
    if constexpr (CLIP) return a.grad_scale * coef;
    else return a.grad_scale;
}

// one float4 of the update (gs = the gradient's scale); returns the new parameter quad and the squared gradient norm contribution
__device__ __forceinline__ f32x4 adamw_quad(const lfvdm_adamw_args& a, float gs, float step, f32x4 g, f32x4 p, f32x4& m, f32x4& v, float& sq) {
    g = g * gs;
    sq += g.x * g.x + g.y * g.y + g.z * g.z + g.w * g.w;
    p = p * (1.0f - a.lr * a.weight_decay);            // decoupled weight decay (torch AdamW)
    m = m * a.beta1 + g * (1.0f - a.beta1);
    v = v * a.beta2 + (g * g) * (1.0f - a.beta2);
    f32x4 d;
    d.x = sqrtf(v.x) / a.bias_corr2_sqrt + a.eps; d.y = sqrtf(v.y) / a.bias_corr2_sqrt + a.eps;
    d.z = sqrtf(v.z) / a.bias_corr2_sqrt + a.eps; d.w = sqrtf(v.w) / a.bias_corr2_sqrt + a.eps;
    p.x -= step * (m.x / d.x); p.y -= step * (m.y / d.y); p.z -= step * (m.z / d.z); p.w -= step * (m.w / d.w);
    return p;
}
__device__ __forceinline__ f32x4 ld4_nt(const float* q) { return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(q)); }
__device__ __forceinline__ void st4_nt(float* q, f32x4 v) { __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(q)); }

// NE = number of EMA copies (compile time: their loads join the batch), U float4 per thread and iteration.  Every load of
// an iteration is issued before the first use (round-3 lesson: a rolled loop of global loads is a chain of dependent round
// trips; here 2 * (4 + NE) 16-byte loads are in flight per thread), the streams that nothing re-reads soon - gradients in,
// moments and EMA copies out - are non-temporal (they would only push the parameters, which the next forward pass reads,
// out of the caches).  9 streams of 4 bytes per parameter: HBM-bound (hbm_phases.adamw_ema).
template <int NE, bool CLIP>
__global__ __launch_bounds__(256) void adamw_ema_kernel(const lfvdm_adamw_args a, const ClipStat<CLIP> clip) {
    // a gradient bucket was reduced before the backward pass had finished writing it (lfvdm_flag_wait gave up): the
    // gradients of this step are garbage - touch nothing, the host raises
    if (a.skip_flag && __hip_atomic_load(a.skip_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return;
    // ... or on ANOTHER rank: the word that rode in the last bucket's SUM all-reduce (any non-zero bit pattern)
    if (a.skip_flag2 && __hip_atomic_load(a.skip_flag2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return;
    float coef = 1.0f;
    if (CLIP) {
        // the record an earlier launch on this stream wrote: inf / NaN gradient norm -> nothing is read or written
        if (reinterpret_cast<const int32_t*>(clip.stat())[2] != 0) return;
        coef = clip.stat()[1];
    }
    constexpr int U = 2;
    const int64_t n4 = a.n / 4;
    float sq = 0.f;
    const float step = a.lr / a.bias_corr1;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i0 < n4; i0 += U * stride) {
        int64_t idx[U];
        f32x4 g[U], p[U], m[U], v[U], e[U][NE > 0 ? NE : 1];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = i0 + u * stride;
            idx[u] = i < n4 ? i : -1;
            const int64_t j = (i < n4 ? i : i0) * 4;          // (a clamped duplicate load; its result is not used)
            g[u] = ld4_nt(a.g + j);
            p[u] = ld4(a.p + j);
            m[u] = ld4_nt(a.m + j);
            v[u] = ld4_nt(a.v + j);
#pragma unroll
            for (int k = 0; k < NE; ++k) e[u][k] = ld4_nt(a.ema[k] + j);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (idx[u] < 0) continue;
            const int64_t j = idx[u] * 4;
            const f32x4 pn = adamw_quad(a, grad_scale_of<CLIP>(a, coef), step, g[u], p[u], m[u], v[u], sq);
            st4(a.p + j, pn);
            st4_nt(a.m + j, m[u]);
            st4_nt(a.v + j, v[u]);
#pragma unroll
            for (int k = 0; k < NE; ++k) st4_nt(a.ema[k] + j, e[u][k] * a.ema_rate[k] + pn * (1.0f - a.ema_rate[k]));   // targ*r + src*(1-r)
        }
    }
    // tail (n not a multiple of 4)
    if (blockIdx.x == 0 && threadIdx.x < (a.n & 3)) {
        const int64_t i = n4 * 4 + threadIdx.x;
        const float g = a.g[i] * grad_scale_of<CLIP>(a, coef);
        sq += g * g;
        float p = a.p[i] * (1.0f - a.lr * a.weight_decay);
        const float m = a.m[i] * a.beta1 + g * (1.0f - a.beta1);
        const float v = a.v[i] * a.beta2 + g * g * (1.0f - a.beta2);
        p -= step * (m / (sqrtf(v) / a.bias_corr2_sqrt + a.eps));
        a.p[i] = p; a.m[i] = m; a.v[i] = v;
        for (int e = 0; e < a.n_ema; ++e) a.ema[e][i] = a.ema[e][i] * a.ema_rate[e] + p * (1.0f - a.ema_rate[e]);
    }
    if (!CLIP && a.grad_sqsum) {         // (clip entry: the pre-clip norm is stat[0])
        sq = wave_sum(sq);
        __shared__ float red[4];
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sq;
        __syncthreads();
        if (threadIdx.x == 0) atomicAdd(a.grad_sqsum, red[0] + red[1] + red[2] + red[3]);
    }
}

// grid of either entry: one float4 per thread and pass, capped at 2048 workgroups of 256
inline unsigned adamw_ema_blocks(int64_t n) {
    int64_t blocks = (n / 4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    return (unsigned)blocks;
}

}  // namespace
