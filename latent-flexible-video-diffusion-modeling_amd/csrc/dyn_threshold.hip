// Dynamic thresholding of x0-hat (Saharia et al. 2022, Imagen section 2.3) as four launches on one stream
// (lfvdm_dyn_threshold, include/lfvdm_hip.h):  per batch row, s = the percentile-quantile of |x0-hat| over the SELECTED
// frames, raised to at least 1 and capped at max_value;  xhat = clamp(x0-hat, -s, s) / s  for every element.
//
// The quantile is EXACT (torch.quantile's linear interpolation between two order statistics): an MSD radix select on the
// bit pattern of |p0| - non-negative floats order as unsigned integers; the sign is cleared, so -0 is +0 - in three digit
// passes of 11 / 11 / 10 bits (the top digit has 10 significant bits: bit 31 is clear).  Both order statistics, of rank
// k = floor(pos) and min(k + 1, n_sel - 1), are TRACKED THROUGH THE SAME PASSES: the two ranks share a digit's histogram
// until their prefixes diverge, from then on pass 2 / 3 fill a second histogram for the second prefix.
//
//   launch 1  p0 = x0-hat -> xhat (all elements);  H1[digit 1] over the selected ones
//   launch 2  every workgroup scans H1 for the two ranks (bin, rank inside the bin);  H2A / H2B[digit 2] of the elements in
//             the chosen bin(s);  workgroup 0 of the row records the choice (and n_sel, frac) for launch 3
//   launch 3  the same one digit down: scans H2, fills H3A / H3B, records the 22-bit prefixes
//   launch 4  scans H3 -> v_lo, v_hi;  q = v_lo + (v_hi - v_lo) frac,  s = min(max(q, 1), max_value)  in fp32;
//             stats[b] = (v_lo, v_hi, s);  xhat rewritten in place
//
// A workgroup histograms into LDS (integer ds_add) and merges its non-empty bins into the row's global histogram with
// integer atomic adds: order-independent, so every byte of the result is reproducible.  No float atomics, no workgroup waits
// on another, no cooperative launch, no flag; the bin of a pass is found at the START of the next launch by every
// workgroup itself (a 2048-entry scan).  pos = percentile (n_sel - 1), k and frac are evaluated in double on the device
// (n_sel depends on the mask, which lives there).
//
// Workspace (lfvdm_dyn_threshold_workspace bytes, per row 5 histograms of 2048 words + 16 words of state): the caller
// zero-fills it ONCE; every call leaves it as the next call needs it without a memset - launch 3 clears H1 (read by launch
// 2 only), launch 4 clears H2, and launch 1 clears the H3 the previous call's launch 4 read.  The sequence is capturable.
//
// x0-hat of an epsilon model.  mean_x0hat<MEAN_EPS> of diffusion_ops.hip is `r x - rm1 out` with the contraction left to
// the compiler, and the compiler chose differently per instantiation (see multistep_mean there): the ancestral and the
// stochastic DDIM cells of lfvdm_update_x0 / lfvdm_update_rng_x0 round both products and subtract, the deterministic DDIM
// cell and the multistep entries evaluate fma(r, x, -(rm1 out)).  Sharing the inline would not pin either form here, so
// both are spelled out with intrinsics and `x0hat_fma` picks the one of the update that will consume xhat;
// tests/test_dyn_threshold_gpu.py compares each with the pred_xstart of the matching lfvdm_update_x0(clip = 0) cell bitwise.
//
// A row without a selected element gets v_lo = v_hi = 0 and s = 1.  NaN inputs are outside the contract (a NaN's bit
// pattern sorts above +inf, so the order statistics stay defined, but s and xhat are then whatever fminf / fmaxf make of it).
#include "common_hip.h"

#include <math.h>

namespace {

constexpr int BINS = 2048;
// word offsets inside one row's workspace
enum { W_H1 = 0, W_H2A = BINS, W_H2B = 2 * BINS, W_H3A = 3 * BINS, W_H3B = 4 * BINS, W_ST2 = 5 * BINS, W_ST3 = 5 * BINS + 8,
       WS_WORDS = 5 * BINS + 16 };

struct DynArgs {
    const float *x, *out;
    const int64_t* t;
    const float *recip, *recipm1, *mask;
    float *xhat, *stats;
    unsigned* ws;
    int T, frame_inner, eps_mode, fma;
    unsigned inner;              // T * frame_inner < 2^31
    double pct;
    float max_value;
};

__device__ __forceinline__ unsigned key_of(float v) { return __float_as_uint(v) & 0x7fffffffu; }

// The bins of the 2048-word histogram h that hold the elements of rank r[0] and r[1] (nr = 1: r[0] only):
// sel[2 j] = bin, sel[2 j + 1] = rank inside the bin.  All 256 threads; sel is left at 0 where the histogram is empty.
__device__ void scan_select(const unsigned* h, const unsigned* r, int nr, unsigned* sel, unsigned* wsum) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u32x4 a = *reinterpret_cast<const u32x4*>(h + 8 * tid), b = *reinterpret_cast<const u32x4*>(h + 8 * tid + 4);
    const unsigned c[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    unsigned tot = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) tot += c[j];
    unsigned incl = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
    }
    __syncthreads();                       // wsum of an earlier call has been read by everyone
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    unsigned excl = incl - tot;
    for (int w = 0; w < wave; ++w) excl += wsum[w];
    for (int k = 0; k < nr; ++k) {
        const unsigned rk = r[k];
        if (rk >= excl && rk - excl < tot) {
            unsigned cum = excl;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (rk >= cum && rk - cum < c[j]) {
                    sel[2 * k] = 8 * tid + j;
                    sel[2 * k + 1] = rk - cum;
                }
                cum += c[j];
            }
        }
    }
    __syncthreads();
}

// f(index inside the row, p0 or the stored value, selected) over this workgroup's share of row b
template <bool VEC, class F>
__device__ __forceinline__ void for_elements(const DynArgs& p, int b, F f) {
    const float* mk = p.mask ? p.mask + (size_t)b * p.T : nullptr;
    if (VEC) {
        const unsigned nq = p.inner >> 2;
        for (unsigned q = blockIdx.x * 256u + threadIdx.x; q < nq; q += gridDim.x * 256u) {
            const unsigned i = 4 * q;
            f(i, !mk || mk[i / (unsigned)p.frame_inner] != 0.f);
        }
    } else {
        for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < p.inner; i += gridDim.x * 256u)
            f(i, !mk || mk[i / (unsigned)p.frame_inner] != 0.f);
    }
}

// (__fmul_rn and __fsub_rn are plain operators to this compiler and would be contracted again: the pragma is what keeps the
// two-product form two products)
__device__ __forceinline__ float x0hat_of(const DynArgs& p, float r, float rm1, float xv, float ov) {
#pragma clang fp contract(off)
    if (!p.eps_mode) return ov;
    const float m = rm1 * ov;
    const float two = r * xv - m;
    return p.fma ? __builtin_fmaf(r, xv, -m) : two;
}

// the non-empty bins of an LDS histogram -> the row's global one
__device__ __forceinline__ void merge(unsigned* g, const unsigned* l, int n) {
    for (int i = threadIdx.x; i < n; i += 256)
        if (l[i]) atomicAdd(g + i, l[i]);
}

__device__ __forceinline__ void clear_words(unsigned* g, int n) {
    for (int i = 4 * threadIdx.x; i < n; i += 1024) *reinterpret_cast<u32x4*>(g + i) = (u32x4){0u, 0u, 0u, 0u};
}

template <bool VEC>
__global__ __launch_bounds__(256) void dyn_pass1_kernel(const DynArgs p) {
    __shared__ unsigned lh[BINS];
    const int b = blockIdx.y;
    unsigned* ws = p.ws + (size_t)b * WS_WORDS;
    if (blockIdx.x == 0) clear_words(ws + W_H3A, 2 * BINS);      // what the previous call's last launch read
    for (int i = threadIdx.x; i < BINS; i += 256) lh[i] = 0;
    __syncthreads();
    float r = 0.f, rm1 = 0.f;
    if (p.eps_mode) {
        const int64_t tb = p.t[b];
        r = p.recip[tb];
        rm1 = p.recipm1[tb];
    }
    const size_t base = (size_t)b * p.inner;
    for_elements<VEC>(p, b, [&](unsigned i, bool sel) {
        if (VEC) {
            const f32x4 ov = ld4(p.out + base + i);
            f32x4 v = ov;
            if (p.eps_mode) {
                const f32x4 xv = ld4(p.x + base + i);
                v = (f32x4){x0hat_of(p, r, rm1, xv.x, ov.x), x0hat_of(p, r, rm1, xv.y, ov.y), x0hat_of(p, r, rm1, xv.z, ov.z),
                            x0hat_of(p, r, rm1, xv.w, ov.w)};
            }
            st4(p.xhat + base + i, v);
            if (sel) {
                atomicAdd(&lh[key_of(v.x) >> 21], 1u);
                atomicAdd(&lh[key_of(v.y) >> 21], 1u);
                atomicAdd(&lh[key_of(v.z) >> 21], 1u);
                atomicAdd(&lh[key_of(v.w) >> 21], 1u);
            }
        } else {
            const float v = x0hat_of(p, r, rm1, p.eps_mode ? p.x[base + i] : 0.f, p.out[base + i]);
            p.xhat[base + i] = v;
            if (sel) atomicAdd(&lh[key_of(v) >> 21], 1u);
        }
    });
    __syncthreads();
    merge(ws + W_H1, lh, BINS);
}

// PASS 2: keys whose digit 1 is a chosen bin -> H2 by digit 2.  PASS 3: keys whose 22-bit prefix is chosen -> H3 by digit 3.
template <int PASS, bool VEC>
__global__ __launch_bounds__(256) void dyn_pass23_kernel(const DynArgs p) {
    __shared__ unsigned lhA[BINS], lhB[BINS];
    __shared__ unsigned sel[4], rk[2], wsum[4], misc[2];
    const int b = blockIdx.y, tid = threadIdx.x;
    unsigned* ws = p.ws + (size_t)b * WS_WORDS;
    for (int i = tid; i < BINS; i += 256) lhA[i] = lhB[i] = 0;
    if (tid < 4) sel[tid] = 0;
    if (tid < 2) misc[tid] = 0;
    __syncthreads();
    unsigned prefA, prefB;
    if (PASS == 2) {
        // n_sel = frame_inner * (frames with a non-zero mask); pos, k, frac in double
        if (p.mask) {
            unsigned c = 0;
            for (int f = tid; f < p.T; f += 256) c += p.mask[(size_t)b * p.T + f] != 0.f;
            if (c) atomicAdd(&misc[0], c);
            __syncthreads();
        }
        if (tid == 0) {
            const unsigned n_sel = (p.mask ? misc[0] : (unsigned)p.T) * (unsigned)p.frame_inner;
            unsigned k = 0, k2 = 0;
            float frac = 0.f;
            if (n_sel) {
                const double pos = p.pct * (double)(n_sel - 1);
                const double fl = floor(pos);
                k = (unsigned)fl;
                if (k > n_sel - 1) k = n_sel - 1;
                frac = (float)(pos - fl);
                k2 = k + 1 < n_sel ? k + 1 : n_sel - 1;
            }
            rk[0] = k;
            rk[1] = k2;
            misc[0] = n_sel;
            misc[1] = __float_as_uint(frac);
        }
        __syncthreads();
        scan_select(ws + W_H1, rk, 2, sel, wsum);
        prefA = sel[0];
        prefB = sel[2];
        if (blockIdx.x == 0 && tid == 0) {
            unsigned* st = ws + W_ST2;
            st[0] = sel[0]; st[1] = sel[1]; st[2] = sel[2]; st[3] = sel[3]; st[4] = misc[0]; st[5] = misc[1];
        }
    } else {
        const unsigned* st = ws + W_ST2;
        const unsigned binA = st[0], binB = st[2];
        if (tid == 0) { rk[0] = st[1]; rk[1] = st[3]; }
        if (blockIdx.x == 0) clear_words(ws + W_H1, BINS);      // launch 2 was its only reader
        __syncthreads();
        if (binA == binB) {
            scan_select(ws + W_H2A, rk, 2, sel, wsum);
        } else {
            scan_select(ws + W_H2A, rk, 1, sel, wsum);
            scan_select(ws + W_H2B, rk + 1, 1, sel + 2, wsum);
        }
        prefA = (binA << 11) | sel[0];
        prefB = (binB << 11) | sel[2];
        if (blockIdx.x == 0 && tid == 0) {
            unsigned* s3 = ws + W_ST3;
            s3[0] = prefA; s3[1] = sel[1]; s3[2] = prefB; s3[3] = sel[3];
        }
    }
    constexpr int SH = PASS == 2 ? 21 : 10;                       // the bits below the prefix
    constexpr unsigned DM = PASS == 2 ? 2047u : 1023u;            // the next digit
    constexpr int DS = PASS == 2 ? 10 : 0;
    const size_t base = (size_t)b * p.inner;
    auto put = [&](float v) {
        const unsigned u = key_of(v), pre = u >> SH, d = (u >> DS) & DM;
        if (pre == prefA) atomicAdd(&lhA[d], 1u);
        else if (pre == prefB) atomicAdd(&lhB[d], 1u);
    };
    for_elements<VEC>(p, b, [&](unsigned i, bool s) {
        if (!s) return;
        if (VEC) {
            const f32x4 v = ld4(p.xhat + base + i);
            put(v.x); put(v.y); put(v.z); put(v.w);
        } else {
            put(p.xhat[base + i]);
        }
    });
    __syncthreads();
    merge(ws + (PASS == 2 ? W_H2A : W_H3A), lhA, PASS == 2 ? BINS : 1024);
    if (prefA != prefB) merge(ws + (PASS == 2 ? W_H2B : W_H3B), lhB, PASS == 2 ? BINS : 1024);
}

template <bool VEC>
__global__ __launch_bounds__(256) void dyn_pass4_kernel(const DynArgs p) {
    __shared__ unsigned sel[4], rk[2], wsum[4];
    const int b = blockIdx.y, tid = threadIdx.x;
    unsigned* ws = p.ws + (size_t)b * WS_WORDS;
    const unsigned* s3 = ws + W_ST3;
    const unsigned prefA = s3[0], prefB = s3[2];
    const unsigned n_sel = ws[W_ST2 + 4];
    const float frac = __uint_as_float(ws[W_ST2 + 5]);
    if (tid < 4) sel[tid] = 0;
    if (tid == 0) { rk[0] = s3[1]; rk[1] = s3[3]; }
    if (blockIdx.x == 0) clear_words(ws + W_H2A, 2 * BINS);     // launch 3 was their only reader
    __syncthreads();
    if (prefA == prefB) {
        scan_select(ws + W_H3A, rk, 2, sel, wsum);
    } else {
        scan_select(ws + W_H3A, rk, 1, sel, wsum);
        scan_select(ws + W_H3B, rk + 1, 1, sel + 2, wsum);
    }
    float v_lo = 0.f, v_hi = 0.f, s = 1.f;
    if (n_sel) {
        v_lo = __uint_as_float((prefA << 10) | sel[0]);
        v_hi = __uint_as_float((prefB << 10) | sel[2]);
        const float q = __fadd_rn(v_lo, __fmul_rn(__fsub_rn(v_hi, v_lo), frac));
        s = fminf(fmaxf(q, 1.f), p.max_value);
    }
    if (blockIdx.x == 0 && tid == 0) {
        p.stats[3 * b] = v_lo;
        p.stats[3 * b + 1] = v_hi;
        p.stats[3 * b + 2] = s;
    }
    const size_t base = (size_t)b * p.inner;
    auto thr = [&](float v) { return __fdiv_rn(fminf(fmaxf(v, -s), s), s); };
    for_elements<VEC>(p, b, [&](unsigned i, bool) {
        if (VEC) {
            const f32x4 v = ld4(p.xhat + base + i);
            st4(p.xhat + base + i, (f32x4){thr(v.x), thr(v.y), thr(v.z), thr(v.w)});
        } else {
            p.xhat[base + i] = thr(p.xhat[base + i]);
        }
    });
}

template <bool VEC>
int launch_all(const DynArgs& p, int B, hipStream_t s) {
    const unsigned work = VEC ? p.inner >> 2 : p.inner;
    unsigned gx = (work + 255) / 256;
    if (gx > 1024) gx = 1024;
    if (gx < 1) gx = 1;
    const dim3 grid(gx, B), block(256);
    hipLaunchKernelGGL((dyn_pass1_kernel<VEC>), grid, block, 0, s, p);
    hipLaunchKernelGGL((dyn_pass23_kernel<2, VEC>), grid, block, 0, s, p);
    hipLaunchKernelGGL((dyn_pass23_kernel<3, VEC>), grid, block, 0, s, p);
    hipLaunchKernelGGL((dyn_pass4_kernel<VEC>), grid, block, 0, s, p);
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}

bool shape_ok(int B, int T, int64_t frame_inner) {
    if (B <= 0 || B > 65535 || T <= 0 || frame_inner <= 0) return false;
    return frame_inner <= 0x7fffffff && (int64_t)T * frame_inner <= 0x7fffffff;      // counts and indices are 32-bit per row
}

}  // namespace

extern "C" int lfvdm_dyn_threshold_workspace(int B, int64_t inner, size_t* bytes) {
    if (!bytes || !shape_ok(B, 1, inner)) return LFVDM_E_SHAPE;
    *bytes = (size_t)B * WS_WORDS * sizeof(unsigned);
    return LFVDM_OK;
}

extern "C" int lfvdm_dyn_threshold(const float* x, const float* model_out, const int64_t* t, const float* sqrt_recip_acp,
                                   const float* sqrt_recipm1_acp, int mean_type, int x0hat_fma, const float* frame_mask, int B,
                                   int T, int64_t frame_inner, double percentile, float max_value, float* xhat, float* stats,
                                   void* workspace, void* stream) {
    if (mean_type != LFVDM_MEAN_EPS && mean_type != LFVDM_MEAN_X0) return LFVDM_E_SHAPE;
    const bool eps = mean_type == LFVDM_MEAN_EPS;
    if (!x || !model_out || !t || !xhat || !stats || !workspace || !shape_ok(B, T, frame_inner)) return LFVDM_E_SHAPE;
    if (eps && (!sqrt_recip_acp || !sqrt_recipm1_acp)) return LFVDM_E_SHAPE;
    if (!(percentile > 0.0 && percentile <= 1.0) || !(max_value >= 1.f)) return LFVDM_E_SHAPE;      // NaN fails both
    if ((uintptr_t)workspace & 15) return LFVDM_E_SHAPE;
    const DynArgs p = {x, model_out, t, sqrt_recip_acp, sqrt_recipm1_acp, frame_mask, xhat, stats, (unsigned*)workspace, T,
                       (int)frame_inner, eps ? 1 : 0, x0hat_fma ? 1 : 0, (unsigned)((int64_t)T * frame_inner), percentile,
                       max_value};
    const bool vec = frame_inner % 4 == 0 && !(((uintptr_t)model_out | (uintptr_t)xhat | (eps ? (uintptr_t)x : 0)) & 15);
    return vec ? launch_all<true>(p, B, (hipStream_t)stream) : launch_all<false>(p, B, (hipStream_t)stream);
}
