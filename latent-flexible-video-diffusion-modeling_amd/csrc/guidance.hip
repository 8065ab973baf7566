// Classifier-free guidance on the observed frames (Ho & Salimans 2022) with the rescale of Lin et al. 2024, section 3.4
// (lfvdm_cfg_combine, include/lfvdm_hip.h).  out2 holds two network outputs of the same x_t: rows [0, B) for the window as
// given (o_c), rows [B, 2B) for the window with its observed frames taken away (o_u).  Per element
//     o_g = o_u + w (o_c - o_u)          three roundings, never contracted
//     x0-hat_g = x0-hat(o_g)             of the model's mean type; an epsilon model's in the rounding `x0hat_fma` names
// and with rescale phi > 0 the whole row is multiplied by f = phi s_c / s_g + (1 - phi), s_c / s_g the population standard
// deviations of x0-hat(o_c) / x0-hat(o_g) over the SELECTED frames of the row.
//
//   phi == 0   one launch: x, o_c, o_u read once, xhat written once (16 B per element); stats = (0, 0, 1)
//   phi  > 0   two launches.  REDUCE writes the unscaled x0-hat_g to xhat and, per chunk of 4096 elements of a row, the
//              record (n, mean_c, M2_c, mean_g, M2_g) of its selected elements to the workspace - two passes over values
//              held in registers (the sum, then the squared deviations from the chunk's own mean), accumulated in double:
//              the variance is never formed as E[v^2] - mean^2, so an off-centre x0-hat costs nothing.  APPLY: every
//              workgroup merges the row's records itself with Chan's formula in one fixed order (lane l of wave 0 folds
//              chunks l, l + 64, ... in ascending order, then lane l takes lane l + 32, 16, ... 1), derives f and scales
//              its chunk of xhat in place; workgroup 0 of the row writes stats = (s_c, s_g, f).
// No atomics of any kind and no workgroup waits on another: two calls on the same inputs give the same bits.  Every record
// of the workspace is overwritten by REDUCE before APPLY reads it, so the workspace is never zero-filled.
//
// Vector accesses: a row starts at element b * inner of each tensor, so with 16-byte aligned pointers the first
// (-b * inner) mod 4 elements of a row (the lead) and the last (inner - lead) mod 4 (the tail) are scalar and everything
// in between moves as float4 - when B * inner is a multiple of 4, which puts o_u on the same phase as o_c.  Otherwise, or
// with an unaligned pointer, every access is scalar (the quads are then just groups of four elements).  The lead and the
// tail - at most six elements - belong to chunk 0.  Elements per frame need not be a multiple of 4: the frame of every
// element is looked up on its own.
#include "common_hip.h"

#include <math.h>

namespace {

constexpr int QPT = 4;                       // quads per thread
constexpr unsigned CHUNK_Q = 256 * QPT;      // quads per chunk = workgroup: 4096 elements
constexpr int REC = 5;                       // doubles per chunk record

struct CfgArgs {
    const float *x, *out2;
    const int64_t* t;
    const float *recip, *recipm1, *mask;
    float *xhat, *stats;
    double* ws;
    int B, T, eps_mode, fma, nch;
    unsigned inner, frame_inner;             // T * frame_inner < 2^31
    float w, phi;
};

// (the pragma keeps the products and the sums apart: see x0hat_of in dyn_threshold.hip, whose two roundings these are)
__device__ __forceinline__ float guided_of(float w, float oc, float ou) {
#pragma clang fp contract(off)
    const float d = oc - ou;
    const float m = w * d;
    return ou + m;
}

__device__ __forceinline__ float x0hat_of(const CfgArgs& p, float r, float rm1, float xv, float ov) {
#pragma clang fp contract(off)
    if (!p.eps_mode) return ov;
    const float m = rm1 * ov;
    const float two = r * xv - m;
    return p.fma ? __builtin_fmaf(r, xv, -m) : two;
}

__device__ __forceinline__ float scale_of(float phi, float sc, float sg) {
#pragma clang fp contract(off)
    const float a = phi * sc;
    const float q = __fdiv_rn(a, sg);
    return q + (1.f - phi);
}

template <bool VEC>
__device__ __forceinline__ f32x4 load4(const float* p) {
    if (VEC) return ld4(p);
    return (f32x4){p[0], p[1], p[2], p[3]};
}
template <bool VEC>
__device__ __forceinline__ void store4(float* p, f32x4 v) {
    if (VEC) { st4(p, v); return; }
    p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
}

// the row's geometry: lead scalars, nq quads, then the tail
struct RowGeom {
    unsigned lead, nq, rest;      // rest = lead + tail <= 6: the scalar elements, all owned by chunk 0
    __device__ unsigned scalar_index(unsigned j) const { return j < lead ? j : lead + 4 * nq + (j - lead); }
};
template <bool VEC>
__device__ __forceinline__ RowGeom geom_of(const CfgArgs& p, int b) {
    RowGeom g;
    const unsigned phase = (unsigned)(((size_t)b * p.inner) & 3);
    g.lead = VEC ? (4u - phase) & 3u : 0u;
    if (g.lead > p.inner) g.lead = p.inner;
    g.nq = (p.inner - g.lead) >> 2;
    g.rest = p.inner - 4 * g.nq;
    return g;
}

// sum over the workgroup in a fixed order: the lanes of a wave by xor, the four waves in wave order
__device__ __forceinline__ double block_sum(double v, double* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();                           // sh of an earlier call has been read by everyone
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// STATS = false: the whole op at phi == 0.  STATS = true: the REDUCE launch.
template <bool VEC, bool STATS>
__global__ __launch_bounds__(256) void cfg_reduce_kernel(const CfgArgs p) {
    __shared__ double sh[4];
    const int b = blockIdx.y, tid = threadIdx.x;
    const unsigned c = blockIdx.x;
    const RowGeom g = geom_of<VEC>(p, b);
    const size_t base = (size_t)b * p.inner, ubase = (size_t)(p.B + b) * p.inner;
    const float* mk = p.mask ? p.mask + (size_t)b * p.T : nullptr;
    float r = 0.f, rm1 = 0.f;
    if (p.eps_mode) {
        const int64_t tb = p.t[b];
        r = p.recip[tb];
        rm1 = p.recipm1[tb];
    }
    float vc[4 * QPT + 1], vg[4 * QPT + 1];      // x0-hat(o_c), x0-hat(o_g) of this thread's elements; 0 where not selected
    unsigned cnt = 0;
#pragma unroll
    for (int j = 0; j < QPT; ++j) {
        const unsigned q = c * CHUNK_Q + j * 256u + tid;
#pragma unroll
        for (int e = 0; e < 4; ++e) vc[4 * j + e] = vg[4 * j + e] = 0.f;
        if (q >= g.nq) continue;
        const unsigned i = g.lead + 4 * q;
        const f32x4 oc = load4<VEC>(p.out2 + base + i), ou = load4<VEC>(p.out2 + ubase + i);
        f32x4 xv = {0.f, 0.f, 0.f, 0.f};
        if (p.eps_mode) xv = load4<VEC>(p.x + base + i);
        f32x4 hg;
        hg.x = x0hat_of(p, r, rm1, xv.x, guided_of(p.w, oc.x, ou.x));
        hg.y = x0hat_of(p, r, rm1, xv.y, guided_of(p.w, oc.y, ou.y));
        hg.z = x0hat_of(p, r, rm1, xv.z, guided_of(p.w, oc.z, ou.z));
        hg.w = x0hat_of(p, r, rm1, xv.w, guided_of(p.w, oc.w, ou.w));
        store4<VEC>(p.xhat + base + i, hg);
        if (STATS) {
            unsigned f = i / p.frame_inner, rem = i - f * p.frame_inner;
            const float hc[4] = {x0hat_of(p, r, rm1, xv.x, oc.x), x0hat_of(p, r, rm1, xv.y, oc.y), x0hat_of(p, r, rm1, xv.z, oc.z),
                                 x0hat_of(p, r, rm1, xv.w, oc.w)};
            const float hgv[4] = {hg.x, hg.y, hg.z, hg.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (!mk || mk[f] != 0.f) {
                    vc[4 * j + e] = hc[e];
                    vg[4 * j + e] = hgv[e];
                    cnt += 1u << (4 * j + e);      // one bit per slot: which of them are selected
                }
                if (++rem == p.frame_inner) { rem = 0; ++f; }
            }
        }
    }
    vc[4 * QPT] = vg[4 * QPT] = 0.f;
    if (c == 0 && (unsigned)tid < g.rest) {      // the lead and the tail
        const unsigned i = g.scalar_index(tid);
        const float oc = p.out2[base + i], ou = p.out2[ubase + i], xv = p.eps_mode ? p.x[base + i] : 0.f;
        const float hg = x0hat_of(p, r, rm1, xv, guided_of(p.w, oc, ou));
        p.xhat[base + i] = hg;
        if (STATS && (!mk || mk[i / p.frame_inner] != 0.f)) {
            vc[4 * QPT] = x0hat_of(p, r, rm1, xv, oc);
            vg[4 * QPT] = hg;
            cnt += 1u << (4 * QPT);
        }
    }
    if (!STATS) {
        if (c == 0 && tid == 0) {
            p.stats[3 * b] = 0.f;
            p.stats[3 * b + 1] = 0.f;
            p.stats[3 * b + 2] = 1.f;
        }
        return;
    }
    // pass 1: count and sums -> the chunk's means
    double sc = 0.0, sg = 0.0;
#pragma unroll
    for (int k = 0; k <= 4 * QPT; ++k) {
        sc += (double)vc[k];
        sg += (double)vg[k];
    }
    // (block_sum holds barriers: every thread calls it, and what depends on n is selected afterwards)
    const double n = block_sum((double)__popc(cnt), sh);
    const double tc = block_sum(sc, sh), tg = block_sum(sg, sh);
    const double mc = n > 0.0 ? tc / n : 0.0;
    const double mg = n > 0.0 ? tg / n : 0.0;
    // pass 2: squared deviations from the chunk's own means, over the selected slots
    double qc = 0.0, qg = 0.0;
#pragma unroll
    for (int k = 0; k <= 4 * QPT; ++k) {
        if (cnt >> k & 1u) {
            const double dc = (double)vc[k] - mc, dg = (double)vg[k] - mg;
            qc = fma(dc, dc, qc);
            qg = fma(dg, dg, qg);
        }
    }
    qc = block_sum(qc, sh);
    qg = block_sum(qg, sh);
    if (tid == 0) {
        double* rec = p.ws + ((size_t)b * p.nch + c) * REC;
        rec[0] = n; rec[1] = mc; rec[2] = qc; rec[3] = mg; rec[4] = qg;
    }
}

struct Moments {
    double n, mc, qc, mg, qg;
};
// Chan, Golub & LeVeque: b folded into a; an empty side changes nothing
__device__ __forceinline__ void chan_merge(Moments& a, const Moments& b) {
    if (b.n == 0.0) return;
    if (a.n == 0.0) { a = b; return; }
    const double n = a.n + b.n, wb = b.n / n, wab = a.n * wb;
    const double dc = b.mc - a.mc, dg = b.mg - a.mg;
    a.mc += dc * wb;
    a.mg += dg * wb;
    a.qc += b.qc + dc * dc * wab;
    a.qg += b.qg + dg * dg * wab;
    a.n = n;
}

template <bool VEC>
__global__ __launch_bounds__(256) void cfg_apply_kernel(const CfgArgs p) {
    __shared__ float sf;
    const int b = blockIdx.y, tid = threadIdx.x;
    const unsigned c = blockIdx.x;
    if (tid < 64) {
        Moments m = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int k = tid; k < p.nch; k += 64) {
            const double* rec = p.ws + ((size_t)b * p.nch + k) * REC;
            const Moments o = {rec[0], rec[1], rec[2], rec[3], rec[4]};
            chan_merge(m, o);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            Moments other;
            other.n = __shfl_down(m.n, o, 64);
            other.mc = __shfl_down(m.mc, o, 64);
            other.qc = __shfl_down(m.qc, o, 64);
            other.mg = __shfl_down(m.mg, o, 64);
            other.qg = __shfl_down(m.qg, o, 64);
            if (tid < o) chan_merge(m, other);
        }
        if (tid == 0) {
            float s_c = 0.f, s_g = 0.f, f = 1.f;
            if (m.n > 0.0) {
                s_c = (float)sqrt(m.qc / m.n);
                s_g = (float)sqrt(m.qg / m.n);
                if (s_g != 0.f) f = scale_of(p.phi, s_c, s_g);
            }
            sf = f;
            if (c == 0) {
                p.stats[3 * b] = s_c;
                p.stats[3 * b + 1] = s_g;
                p.stats[3 * b + 2] = f;
            }
        }
    }
    __syncthreads();
    const float f = sf;
    const RowGeom g = geom_of<VEC>(p, b);
    float* row = p.xhat + (size_t)b * p.inner;
#pragma unroll
    for (int j = 0; j < QPT; ++j) {
        const unsigned q = c * CHUNK_Q + j * 256u + tid;
        if (q >= g.nq) continue;
        float* at = row + g.lead + 4 * q;
        const f32x4 v = load4<VEC>(at);
        store4<VEC>(at, (f32x4){v.x * f, v.y * f, v.z * f, v.w * f});
    }
    if (c == 0 && (unsigned)tid < g.rest) row[g.scalar_index(tid)] *= f;
}

template <bool VEC>
int launch_all(const CfgArgs& p, hipStream_t s) {
    const dim3 grid(p.nch, p.B), block(256);
    if (p.phi == 0.f) {
        hipLaunchKernelGGL((cfg_reduce_kernel<VEC, false>), grid, block, 0, s, p);
    } else {
        hipLaunchKernelGGL((cfg_reduce_kernel<VEC, true>), grid, block, 0, s, p);
        hipLaunchKernelGGL((cfg_apply_kernel<VEC>), grid, block, 0, s, p);
    }
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}

bool shape_ok(int B, int T, int64_t frame_inner) {
    if (B <= 0 || B > 32767 || T <= 0 || frame_inner <= 0) return false;      // out2 has 2 B rows; B rides in gridDim.y
    return frame_inner <= 0x7fffffff && (int64_t)T * frame_inner <= 0x7fffffff;      // indices are 32-bit per row
}

// chunks per row: every quad of a row, whatever its lead (a row with fewer quads leaves its last record empty)
int chunks_of(int64_t inner) {
    const int64_t q = inner / 4;
    return q <= CHUNK_Q ? 1 : (int)((q + CHUNK_Q - 1) / CHUNK_Q);
}

}  // namespace

extern "C" int lfvdm_cfg_workspace(int B, int64_t inner, size_t* bytes) {
    if (!bytes || !shape_ok(B, 1, inner)) return LFVDM_E_SHAPE;
    *bytes = (size_t)B * chunks_of(inner) * REC * sizeof(double);
    return LFVDM_OK;
}

extern "C" int lfvdm_cfg_combine(const float* x, const float* out2, const int64_t* t, const float* sqrt_recip_acp,
                                 const float* sqrt_recipm1_acp, int mean_type, int x0hat_fma, const float* frame_mask,
                                 float scale, float rescale, float* xhat, float* stats, void* workspace, int B, int T,
                                 int64_t frame_inner, void* stream) {
    if (mean_type != LFVDM_MEAN_EPS && mean_type != LFVDM_MEAN_X0) return LFVDM_E_SHAPE;
    const bool eps = mean_type == LFVDM_MEAN_EPS;
    if (!x || !out2 || !t || !xhat || !stats || !shape_ok(B, T, frame_inner)) return LFVDM_E_SHAPE;
    if (eps && (!sqrt_recip_acp || !sqrt_recipm1_acp)) return LFVDM_E_SHAPE;
    if (!(scale >= 0.f) || isinf(scale) || !(rescale >= 0.f && rescale <= 1.f)) return LFVDM_E_SHAPE;      // NaN fails both
    if (rescale > 0.f && (!workspace || ((uintptr_t)workspace & 7))) return LFVDM_E_SHAPE;
    const int64_t inner = (int64_t)T * frame_inner;
    const CfgArgs p = {x, out2, t, sqrt_recip_acp, sqrt_recipm1_acp, frame_mask, xhat, stats, (double*)workspace, B, T,
                       eps ? 1 : 0, x0hat_fma ? 1 : 0, chunks_of(inner), (unsigned)inner, (unsigned)frame_inner, scale, rescale};
    const bool vec = ((int64_t)B * inner) % 4 == 0 && !(((uintptr_t)out2 | (uintptr_t)xhat | (eps ? (uintptr_t)x : 0)) & 15);
    return vec ? launch_all<true>(p, (hipStream_t)stream) : launch_all<false>(p, (hipStream_t)stream);
}
