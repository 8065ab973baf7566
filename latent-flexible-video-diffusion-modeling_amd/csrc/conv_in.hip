// The model's prologue: input compositing x*(1-obs) + x0*obs, the indicator channel and the first 3x3 conv in one
// launch, scalar or on the matrix cores; the sampler's clock can ride along (lfvdm_conv_in_tick).
#include "common_hip.h"

namespace {

// -------------------------------------------------------------------------------------
// conv_in: x*(1-obs)+x0*obs, indicator channel = obs, 3x3 pad-1 conv, channels-last output.
// Workgroup = 64 consecutive pixels x all filters: lane = pixel (the NCHW input planes are read as contiguous runs of
// the wave), wave w = filters [w*Cout/4, (w+1)*Cout/4) in quads; weights [(C+1)*9][Cout] in LDS, read as wave-uniform
// (broadcast) float4.  (The first version gave every thread one pixel and ONE quad: 16 threads re-loaded each input
// value and four times as many workgroups staged the weight table - 13 us for a 30 MFLOP layer.)
// -------------------------------------------------------------------------------------
// The sampler's clock rides in this launch (the first of a denoising step, and nothing in it reads the timestep): one
// extra workgroup does what lfvdm_sampler_tick_fetch does - t <- max(t - 1, 0), model timestep <- table[t], FiLM rows of
// the new t fetched from the chain's table - one launch less per step.
struct ConvInTick {
    int64_t* t;                // [B] or NULL: no clock in this launch
    const float* table;
    float* model_t;
    const float* rows_all;
    float* rows;
    int B, rows_ld, row_floats;
};

// The clock's workgroup.  Its FiLM-row fetch reads a cold corner of the chain's table: the rows are copied eight float4
// per thread at a time with all loads issued before the first store (the one-load-per-trip loop was six dependent round
// trips - longer than the convolution's workgroups once those run on the matrix cores).
__device__ __forceinline__ void conv_in_clock(const ConvInTick& tk, int64_t* tnew) {
    if ((int)threadIdx.x < tk.B) {
        int64_t v = tk.t[threadIdx.x] - 1;
        v = v < 0 ? 0 : v;
        tk.t[threadIdx.x] = v;
        tnew[threadIdx.x] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < tk.B) tk.model_t[threadIdx.x] = tk.table[tnew[threadIdx.x]];     // (off the rows' critical path)
    const int q4 = tk.row_floats >> 2;
    for (int b = 0; b < tk.B; ++b) {
        const float* src = tk.rows_all + ((size_t)tnew[b] * tk.B + b) * tk.rows_ld;
        float* dst = tk.rows + (size_t)b * tk.rows_ld;
        for (int i0 = threadIdx.x; i0 < q4; i0 += 256 * 8) {
            f32x4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + 256 * u;
                v[u] = i < q4 ? ld4(src + 4 * i) : (f32x4){0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + 256 * u;
                if (i < q4) st4(dst + 4 * i, v[u]);
            }
        }
    }
}

template <int QW, int CIT>      // QW float4 quads of output channels per thread (Cout = 16 * QW); CIT = C + 1 when it is
                                // known at compile time (4 / 5: the input gather is then fully unrolled), else 0
__global__ __launch_bounds__(256) void conv_in_kernel(const float* __restrict__ x, const float* __restrict__ x0,
                                                      const float* __restrict__ obs, const float* __restrict__ w,
                                                      const float* __restrict__ bias, float* __restrict__ out, int N,
                                                      int C, int H, int W, ConvInTick tk) {
    constexpr int Cout = 16 * QW;
    extern __shared__ __attribute__((aligned(16))) float wl[];  // [k = ci*9+tap][Cout]
    if (tk.t != nullptr && blockIdx.x == gridDim.x - 1) {        // the clock's workgroup (workgroup-uniform branch)
        conv_in_clock(tk, reinterpret_cast<int64_t*>(wl));
        return;
    }
    const int Ci = CIT ? CIT : C + 1;
    const int K = Ci * 9;
    constexpr int CP = Cout + 4;                  // padded LDS row: the transposing writes below spread over the banks
    // w is OIHW = [co][k]: read it as it lies (consecutive threads -> consecutive floats: coalesced; the first version
    // walked co fastest, 256 cache lines per wave load, in every one of the 160 workgroups) and transpose in LDS
    {
        // (four 16-byte loads in flight per thread: the one-load-per-trip form was eleven dependent L2 round trips)
        const float rK = __builtin_amdgcn_rcpf((float)K);
        const int total4 = (K * Cout) >> 2;                   // Cout is a multiple of 16
        for (int i0 = threadIdx.x; i0 < total4; i0 += 256 * 4) {
            f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i4 = i0 + 256 * u;
                v[u] = i4 < total4 ? ld4(w + 4 * (size_t)i4) : (f32x4){0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i4 = i0 + 256 * u;
                if (i4 < total4) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int i = 4 * i4 + e;
                        int co = (int)((float)i * rK);
                        int k = i - co * K;
                        if (k < 0) { k += K; co -= 1; }
                        if (k >= K) { k -= K; co += 1; }
                        wl[k * CP + co] = v[u][e];
                    }
                }
            }
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int grp = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int HW = H * W;
    const long total = (long)N * HW;
    const long pix = (long)blockIdx.x * 64 + lane;
    const bool live = pix < total;
    const long pp = live ? pix : total - 1;
    const int n = (int)(pp / HW);
    const int p = (int)(pp - (long)n * HW);
    const int oy = p / W, ox = p - oy * W;
    const float ob = obs[n];
    f32x4 acc[QW];
#pragma unroll
    for (int q = 0; q < QW; ++q) acc[q] = ld4(bias + (grp * QW + q) * 4);
    const float* xn = x + (size_t)n * C * HW;
    const float* x0n = x0 + (size_t)n * C * HW;
    const float* wg = wl + grp * QW * 4;
    if constexpr (CIT > 0) {
        // all 9 * (C + 1) composited inputs first (independent loads: one exposed latency), then the FMAs
        float v[9][CIT];
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int iy = oy + tap / 3 - 1, ix = ox + tap % 3 - 1;
            const bool inb = iy >= 0 && iy < H && ix >= 0 && ix < W;
            const int ip = inb ? iy * W + ix : p;
#pragma unroll
            for (int ci = 0; ci < CIT; ++ci) {
                float t = ob;
                if (ci < CIT - 1) t = xn[ci * HW + ip] * (1.0f - ob) + x0n[ci * HW + ip] * ob;
                v[tap][ci] = inb ? t : 0.f;
            }
        }
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int ci = 0; ci < CIT; ++ci) {
                const float* wk = wg + (ci * 9 + tap) * CP;
#pragma unroll
                for (int q = 0; q < QW; ++q) acc[q] += v[tap][ci] * ld4(wk + q * 4);
            }
    } else {
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int iy = oy + tap / 3 - 1, ix = ox + tap % 3 - 1;
            const bool inb = iy >= 0 && iy < H && ix >= 0 && ix < W;
            const int ip = inb ? iy * W + ix : p;
            for (int ci = 0; ci < Ci; ++ci) {
                float v = ob;
                if (ci < C) v = xn[ci * HW + ip] * (1.0f - ob) + x0n[ci * HW + ip] * ob;
                v = inb ? v : 0.f;
                const float* wk = wg + (ci * 9 + tap) * CP;
#pragma unroll
                for (int q = 0; q < QW; ++q) acc[q] += v * ld4(wk + q * 4);
            }
        }
    }
    if (live) {
        float* o = out + (size_t)pix * Cout + grp * QW * 4;
#pragma unroll
        for (int q = 0; q < QW; ++q) st4(o + q * 4, acc[q]);
    }
}

// The same convolution on the matrix cores, for the latent / pixel models (C + 1 = 5 or 4 input channels: K = 45 / 36).
// Per workgroup of 64 pixels the composited 3x3 patches are laid out as an im2col tile A[64][KP] in LDS (KP = K padded
// to a multiple of 4; a thread's pixel is fixed and its k values are wave-uniform: coalesced reads of the (B,T,C,H,W)
// tensors, scalar tap decode), the filters - OIHW rows ARE [Cout][K] - as W[Cout][KP]; each wave multiplies its 16 pixels
// by all filters with v_mfma_f32_16x16x4_f32.  Every global load of a phase is issued before the first use (fully
// unrolled: K is a template parameter): the scalar kernel above measures 11.5 us whatever its arithmetic costs - a first
// matrix-core version with a rolled gather loop (twelve dependent round trips) measured the same.
template <int NCT, int CI>      // Cout = 16 NCT; CI = C + 1
__global__ __launch_bounds__(256) void conv_in_mfma_kernel(const float* __restrict__ x, const float* __restrict__ x0,
                                                           const float* __restrict__ obs, const float* __restrict__ w,
                                                           const float* __restrict__ bias, float* __restrict__ out, int N,
                                                           int H, int W, ConvInTick tk) {
    constexpr int Cout = 16 * NCT, C = CI - 1, K = 9 * CI, KP = (K + 3) & ~3, KS = KP + 1;   // odd LDS row stride
    constexpr int NKI = KP / 4;          // k values per wave (k = wave + 4 i)
    extern __shared__ __attribute__((aligned(16))) float wl[];
    if (tk.t != nullptr && blockIdx.x == gridDim.x - 1) {        // the clock's workgroup (see conv_in_kernel)
        conv_in_clock(tk, reinterpret_cast<int64_t*>(wl));
        return;
    }
    float* As = wl;                  // [64][KS]
    float* Ws = wl + 64 * KS;        // [Cout][KS]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // ---- all global loads first: the filters (wave w stages rows w, w + 4, ...; lane = k) and the im2col values
    float wv[Cout / 4];
#pragma unroll
    for (int i = 0; i < Cout / 4; ++i) wv[i] = lane < K ? w[(size_t)(wave + 4 * i) * K + lane] : 0.f;
    const int HW = H * W;
    const long total = (long)N * HW;
    const long pix = (long)blockIdx.x * 64 + lane;
    const bool live = pix < total;
    const long pp = live ? pix : total - 1;
    const int n = (int)(pp / HW);
    const int pq = (int)(pp - (long)n * HW);
    const int oy = pq / W, ox = pq - oy * W;
    const float ob = obs[n];
    const float* xn = x + (size_t)n * C * HW;
    const float* x0n = x0 + (size_t)n * C * HW;
    float xa[NKI], xb[NKI];
    bool inb[NKI];
#pragma unroll
    for (int i = 0; i < NKI; ++i) {
        const int k = wave + 4 * i;              // wave-uniform
        const int ci = k / 9, tap = k - ci * 9;
        const int iy = oy + tap / 3 - 1, ix = ox + tap % 3 - 1;
        inb[i] = live && k < K && iy >= 0 && iy < H && ix >= 0 && ix < W;
        const int ip = inb[i] ? iy * W + ix : pq;
        const int cc = ci < C ? ci : 0;
        xa[i] = xn[cc * HW + ip];
        xb[i] = x0n[cc * HW + ip];
    }
#pragma unroll
    for (int i = 0; i < Cout / 4; ++i)
        if (lane < KP) Ws[(wave + 4 * i) * KS + lane] = wv[i];
#pragma unroll
    for (int i = 0; i < NKI; ++i) {
        const int k = wave + 4 * i;
        const int ci = k / 9;
        float v = ci < C ? xa[i] * (1.0f - ob) + xb[i] * ob : ob;
        As[lane * KS + k] = inb[i] ? v : 0.f;
    }
    __syncthreads();
    const int r16 = lane & 15, kq = lane >> 4;
    f32x4 acc[NCT];
#pragma unroll
    for (int c = 0; c < NCT; ++c) {
        const float b = bias[16 * c + r16];
        acc[c] = (f32x4){b, b, b, b};
    }
    const float* ar = As + (16 * wave + r16) * KS + kq;
    const float* wr = Ws + r16 * KS + kq;
#pragma unroll
    for (int s4 = 0; s4 < KP; s4 += 4) {
        const float a = ar[s4];
#pragma unroll
        for (int c = 0; c < NCT; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wr[16 * c * KS + s4], acc[c], 0, 0, 0);
    }
    // D: lane holds rows 4 (lane >> 4) + r, column lane & 15 of each 16x16 tile
    const long p0 = (long)blockIdx.x * 64 + 16 * wave + 4 * kq;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (p0 + r < total) {
            float* o = out + (size_t)(p0 + r) * Cout + r16;
#pragma unroll
            for (int c = 0; c < NCT; ++c) o[16 * c] = acc[c][r];
        }
    }
}

int conv_in_launch(const float* x, const float* x0, const float* obs, const float* w, const float* bias, float* out, int N,
                   int C, int H, int W, int Cout, const ConvInTick& tk, hipStream_t s) {
    if (N <= 0 || C <= 0 || Cout % 16 || Cout > 256 || H <= 0 || W <= 0) return LFVDM_E_SHAPE;
    size_t lds = (size_t)(C + 1) * 9 * (Cout + 4) * sizeof(float);      // padded rows (see the kernel)
    if (lds > 64 * 1024) return LFVDM_E_UNSUPPORTED;
    if (lds < 64 * sizeof(int64_t)) lds = 64 * sizeof(int64_t);
    const long total = (long)N * H * W;
    const dim3 grid((unsigned)((total + 63) / 64) + (tk.t ? 1u : 0u));
    {   // matrix-core form (see conv_in_mfma_kernel) for the latent / pixel inputs and 64 / 128 filters
        static const bool off = getenv("LFVDM_CONV_IN_SCALAR") != nullptr;       // A/B aid
        if (!off && (C == 4 || C == 3) && (Cout == 64 || Cout == 128)) {
            const int KP = (9 * (C + 1) + 3) & ~3;
            size_t l2 = (size_t)(64 + Cout) * (KP + 1) * sizeof(float);
            if (l2 < 64 * sizeof(int64_t)) l2 = 64 * sizeof(int64_t);
#define LFVDM_CIM(NCT, CI) hipLaunchKernelGGL((conv_in_mfma_kernel<NCT, CI>), grid, dim3(256), l2, s, x, x0, obs, w, bias, out, N, H, W, tk)
            if (C == 4) { if (Cout == 64) LFVDM_CIM(4, 5); else LFVDM_CIM(8, 5); }
            else { if (Cout == 64) LFVDM_CIM(4, 4); else LFVDM_CIM(8, 4); }
#undef LFVDM_CIM
            LFVDM_CHECK_LAUNCH();
            return LFVDM_OK;
        }
    }
#define LFVDM_CONV_IN(Q)                                                                                              \
    case Q:                                                                                                           \
        if (C == 4) hipLaunchKernelGGL((conv_in_kernel<Q, 5>), grid, dim3(256), lds, s, x, x0, obs, w, bias, out, N, C, H, W, tk);      \
        else if (C == 3) hipLaunchKernelGGL((conv_in_kernel<Q, 4>), grid, dim3(256), lds, s, x, x0, obs, w, bias, out, N, C, H, W, tk); \
        else hipLaunchKernelGGL((conv_in_kernel<Q, 0>), grid, dim3(256), lds, s, x, x0, obs, w, bias, out, N, C, H, W, tk);             \
        break;
    switch (Cout / 16) {
        LFVDM_CONV_IN(1) LFVDM_CONV_IN(2) LFVDM_CONV_IN(3) LFVDM_CONV_IN(4) LFVDM_CONV_IN(5) LFVDM_CONV_IN(6) LFVDM_CONV_IN(7)
        LFVDM_CONV_IN(8) LFVDM_CONV_IN(9) LFVDM_CONV_IN(10) LFVDM_CONV_IN(11) LFVDM_CONV_IN(12) LFVDM_CONV_IN(13)
        LFVDM_CONV_IN(14) LFVDM_CONV_IN(15) LFVDM_CONV_IN(16)
        default: return LFVDM_E_SHAPE;
    }
#undef LFVDM_CONV_IN
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}

}  // namespace

extern "C" int lfvdm_conv_in(const float* x, const float* x0, const float* obs, const float* w, const float* bias,
                             float* out, int N, int C, int H, int W, int Cout, void* stream) {
    const ConvInTick none = {nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0};
    return conv_in_launch(x, x0, obs, w, bias, out, N, C, H, W, Cout, none, (hipStream_t)stream);
}

extern "C" int lfvdm_conv_in_tick(const float* x, const float* x0, const float* obs, const float* w, const float* bias,
                                  float* out, int N, int C, int H, int W, int Cout, int64_t* t,
                                  const float* model_timestep_table, float* model_t, int B, const float* rows_all, int rows_ld,
                                  float* rows, int row_floats, void* stream) {
    if (B <= 0 || B > 64 || !t || !model_timestep_table || !model_t || !rows_all || !rows) return LFVDM_E_SHAPE;
    if (row_floats <= 0 || (row_floats & 3) || (rows_ld & 3) || rows_ld < row_floats) return LFVDM_E_SHAPE;
    const ConvInTick tk = {t, model_timestep_table, model_t, rows_all, rows, B, rows_ld, row_floats};
    return conv_in_launch(x, x0, obs, w, bias, out, N, C, H, W, Cout, tk, (hipStream_t)stream);
}
