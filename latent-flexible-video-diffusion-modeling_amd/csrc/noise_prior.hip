// Temporally correlated noise prior (the mixed / progressive priors of PYoCo, Ge et al., ICCV 2023, defined on the frame
// INDICES of a window): per sample the noise over frames at a fixed (channel, y, x) has covariance
//     K_ij = a + c rho^|f_i - f_j| + (1 - a - c) [i == j]
// and is drawn as L xi, L the lower Cholesky factor of K and xi i.i.d. N(0, 1) (contract: include/lfvdm_hip.h).
//
// noise_prior_factor_kernel: one workgroup of one wave per sample, lane i owns row i.  K and the left-looking Cholesky live
// in fp64 in LDS (T <= 64: 64^3 / 3 flops, two barriers per column - the cost does not matter, it runs once per chain);
// rows are padded to 65 doubles, so the lanes' 8-byte reads of one column fall on distinct banks and row j is a broadcast.
//
// noise_prior_fill_kernel: out[b][i][e] = sum_{j <= i} L[b][i][j] xi[b][j][e].  A workgroup owns ALL T frames of a tile of
// TE = 32 consecutive elements of one sample: it stages L (T x T, padded rows) and the T x 32 tile of xi in LDS - read from
// memory (mix mode) or drawn with Philox on NOISE_STREAM_PRIOR (draw mode) - meets a barrier and only then stores, which is
// what makes out == xi safe: no other workgroup reads or writes that tile.  The launch is latency-bound (0.65 MB at the
// largest sampler window): a small tile gives 256 workgroups there, 25 KB of LDS each.  A thread holds one quad of elements
// for one output row at a time (rows r, r + 32): one 16-byte LDS read of xi (8 distinct addresses per wave, each a
// broadcast) and one 4-byte read of L (8 rows 65 floats apart: distinct banks) per four fmaf.  The sum runs in ascending j
// whatever the grid: every output element is the same chain of fmaf in every launch.  No atomics.
#include "common_hip.h"
#include "philox_normal.h"

namespace {

constexpr int MAX_T = 64;            // frames per window (the temporal attention's limit as well)
constexpr int LROW = MAX_T + 1;      // padded row of L / K in LDS
constexpr int TE = 32;               // elements of a frame per workgroup tile
constexpr int MAX_ROWS = 65535;      // B rides in gridDim.y
constexpr double PIVOT_MIN = 1e-12;

__global__ __launch_bounds__(64) void noise_prior_factor_kernel(const int64_t* __restrict__ frames, double a, double c,
                                                                double rho, float* __restrict__ L_out, int T) {
    __shared__ double Ks[MAX_T * LROW];
    __shared__ unsigned long long fs[MAX_T];
    __shared__ double pivot;
    const int b = blockIdx.x, i = threadIdx.x;
    if (i < T) fs[i] = (unsigned long long)frames[(size_t)b * T + i];
    __syncthreads();
    if (i < T) {
        const long long fi = (long long)fs[i];
        for (int j = 0; j < i; ++j) {
            const long long fj = (long long)fs[j];
            // |f_i - f_j| exactly, whatever the two int64 values are (the unsigned difference cannot overflow)
            const unsigned long long gap = fi > fj ? fs[i] - fs[j] : fs[j] - fs[i];
            Ks[i * LROW + j] = a + c * pow(rho, (double)gap);
        }
        Ks[i * LROW + i] = 1.0;
    }
    __syncthreads();
    for (int j = 0; j < T; ++j) {
        const bool mine = i >= j && i < T;
        double s = 0.0;
        if (mine) {
            s = Ks[i * LROW + j];
            for (int k = 0; k < j; ++k) s -= Ks[i * LROW + k] * Ks[j * LROW + k];
        }
        if (i == j) pivot = s;
        __syncthreads();
        const double d = pivot;
        // the diagonal too is d / sqrt(d): the row of a repeated frame then equals its twin's bit for bit
        if (mine) Ks[i * LROW + j] = d < PIVOT_MIN ? 0.0 : s / sqrt(d);
        __syncthreads();
    }
    float* Lb = L_out + (size_t)b * T * T;
    for (int idx = i; idx < T * T; idx += 64) {
        const int r = idx / T, col = idx - r * T;
        Lb[idx] = col <= r ? (float)Ks[r * LROW + col] : 0.0f;
    }
}

// DRAW: xi drawn here; else read from `xi` (which may be `out`: neither is __restrict__).  VEC: E % 4 == 0 and 16-byte
// aligned pointers - a quad of the tile is inside the frame or outside it as a whole.
template <bool DRAW, bool VEC>
__global__ __launch_bounds__(256) void noise_prior_fill_kernel(const float* __restrict__ L, const float* xi,
                                                               const int64_t* __restrict__ seed, const int64_t* __restrict__ t,
                                                               float* out, int T, long E, int n_tiles) {
    __shared__ __attribute__((aligned(16))) float xs[MAX_T * TE];
    __shared__ float Ls[MAX_T * LROW];
    const int b = blockIdx.y, tid = threadIdx.x;
    const float* Lb = L + (size_t)b * T * T;
    for (int idx = tid; idx < T * T; idx += 256) {
        const int r = idx / T;
        Ls[r * LROW + (idx - r * T)] = Lb[idx];
    }
    const size_t base = (size_t)b * T * E;
    unsigned k0 = 0, k1 = 0, step = 0;
    if (DRAW) {
        const unsigned long long key = (unsigned long long)seed[0];
        k0 = (unsigned)key;
        k1 = (unsigned)(key >> 32);
        step = (unsigned)t[b];
    }
    const int q = tid & 7, r0 = tid >> 3;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long e0 = (long)tile * TE;
        if (VEC) {
            for (int idx = tid; idx < T * (TE / 4); idx += 256) {
                const int j = idx >> 3;
                const long e = e0 + 4 * (idx & 7);
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (e < E) {
                    const size_t off = (size_t)j * E + e;      // within the row of T * E elements: below 2^31
                    v = DRAW ? normal4_stream((unsigned)(off >> 2), (unsigned)b, step, NOISE_STREAM_PRIOR, k0, k1)
                             : ld4(xi + base + off);
                }
                st4(xs + j * TE + 4 * (idx & 7), v);
            }
        } else {
            for (int idx = tid; idx < T * TE; idx += 256) {
                const int j = idx >> 5;
                const long e = e0 + (idx & 31);
                xs[idx] = e < E ? xi[base + (size_t)j * E + e] : 0.f;
            }
        }
        __syncthreads();      // the whole tile (all T frames) is in LDS before anything of it is overwritten in memory
        const long e = e0 + 4 * q;
        for (int i = r0; i < T; i += 32) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int j = 0; j <= i; ++j) {
                const float l = Ls[i * LROW + j];
                const f32x4 x = *reinterpret_cast<const f32x4*>(xs + j * TE + 4 * q);
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] = __builtin_fmaf(l, x[k], acc[k]);
            }
            float* dst = out + base + (size_t)i * E + e;
            if (VEC) {
                if (e < E) st4(dst, acc);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (e + k < E) dst[k] = acc[k];
            }
        }
        __syncthreads();      // xs is staged again by the next tile of this workgroup
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int lfvdm_noise_prior_factor(const int64_t* frame_indices, double a, double c, double rho, float* L_out, int B, int T,
                                        void* stream) {
    if (!frame_indices || !L_out || B <= 0 || B > MAX_ROWS || T < 1 || T > MAX_T) return LFVDM_E_SHAPE;
    if (!(a >= 0.0) || !(c >= 0.0) || !(a + c <= 1.0 + 1e-12) || !(rho >= 0.0) || !(rho < 1.0)) return LFVDM_E_SHAPE;
    hipLaunchKernelGGL(noise_prior_factor_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, frame_indices, a, c, rho, L_out, T);
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}

extern "C" int lfvdm_noise_prior_fill(const float* L, const float* xi, const int64_t* seed, const int64_t* t, float* out, int B,
                                      int T, int64_t E, void* stream) {
    if (!L || !out || B <= 0 || B > MAX_ROWS || T < 1 || T > MAX_T || E < 1) return LFVDM_E_SHAPE;
    if ((int64_t)T * E > 2147483647LL) return LFVDM_E_SHAPE;
    const bool draw = xi == nullptr;
    const bool vec = (E & 3) == 0 && aligned16(out) && (draw || aligned16(xi));
    if (draw && (!seed || !t || !vec)) return LFVDM_E_SHAPE;
    const int n_tiles = (int)((E + TE - 1) / TE);
    const dim3 grid(n_tiles < 1024 ? n_tiles : 1024, B);
    hipStream_t st = (hipStream_t)stream;
#define LFVDM_PRIOR_FILL(DRAW, VEC)                                                                                      \
    hipLaunchKernelGGL((noise_prior_fill_kernel<DRAW, VEC>), grid, dim3(256), 0, st, L, xi, seed, t, out, T, (long)E, n_tiles)
    if (draw) LFVDM_PRIOR_FILL(true, true);
    else if (vec) LFVDM_PRIOR_FILL(false, true);
    else LFVDM_PRIOR_FILL(false, false);
#undef LFVDM_PRIOR_FILL
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}
