// Frame distances and greedy farthest-point selection for the adaptive sampling schemes (improved_diffusion/frame_select.py).
//
//   x (B, T, C, H, W) float32.  For two frames a, b and L levels (1..3):
//     d_L(a, b) = (1 / L) * sum_{l < L} mean((P_l(a - b))^2),  P_0 = identity, P_l = 2^l x 2^l average pooling.
//   Pooling is linear, so every level comes from one pass over the DIFFERENCE: with S = 2^(L-1), a lane that holds one
//   S x S block of a - b forms the block's level-0 squares, its 2 x 2 sums and (L = 3) its 4 x 4 sum in registers.  With
//   q_l = sum over the level-l blocks of (block sum)^2:  d_L = (q_0 + q_1 / 4 + q_2 / 16) / (L * C * H * W).
//   The difference form, never ||a||^2 + ||b||^2 - 2 a.b: neighbouring frames are nearly equal and the Gram form cancels
//   in fp32 exactly for the pairs the selection ranks.  So this is a streaming reduction, not an MFMA contraction.
//
// lfvdm_frame_dist_rows: one workgroup of 256 threads per (video, tile of TI = 4 new frames x TJ = 4 target frames), the
// targets being the list new ++ cand.  Thread t owns the blocks t, t + 256, ... of the frame: per block it loads the four
// new frames' values into registers ONCE and then the four targets' one after the other, so a tile of 16 pairs reads 8 frame
// chunks from memory instead of 32 (the choice of 4 x 4: 16 accumulators + (4 + 1) * S^2 block values + the differences
// compile to 50 / 76 / 204 VGPRs at L = 1 / 2 / 3 without scratch; a wider tile would spill at L = 3, and the kernel's limit is
// the loads, not the 16 pairs of arithmetic).  Each pair's partial is accumulated block by block in index order, then summed over the
// wave by an xor butterfly (every lane forms the same sums: a + b = b + a) and over the four waves in wave order.  No
// atomics.  The order depends on (C, H, W, L) alone - not on the tile, the slot inside the tile or the launch - and
// a - b = -(b - a) exactly with sums of negated terms negated exactly, so d(i, j) and d(j, i) are the same bits whoever
// computes them (a pair of two new frames is computed by two tiles and written twice with the same value).  The diagonal
// is written as 0.  An index outside [0, T) is never dereferenced and writes nothing.
//
// lfvdm_fps_select: one workgroup of 256 threads per video runs all n picks of the host loop
//     min_d = min(min_d, dist[cand[picks[i-1]], cand[:]]);  picks[i] = forced[i] if i < n_forced else argmax(min_d)
// in one launch: min_d lives in LDS (entry p is only ever touched by thread p % 256), a pick is a (value, lowest
// position) reduction by wave shuffles and then over the four waves through LDS, two barriers per pick.  NaN follows numpy
// (np.minimum propagates it, np.argmax returns the first one).  A forced position outside [0, n_cand) or a chosen frame
// outside [0, T) ends the selection: that pick and all later ones are -1.  Other candidates outside [0, T) read as 0.
#include "common_hip.h"

namespace {

constexpr int NT = 256, NW = NT / 64;
constexpr int TI = 4, TJ = 4;
constexpr int FPS_MAX_CAND = 4096;

template <int S>
__device__ __forceinline__ void load_block(const float* __restrict__ p, int W, bool vec, float (&v)[S * S]) {
    if constexpr (S == 1) {
        v[0] = p[0];
    } else if constexpr (S == 2) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (vec) {
                const f32x2 q = *reinterpret_cast<const f32x2*>(p + (size_t)r * W);
                v[2 * r] = q[0];
                v[2 * r + 1] = q[1];
            } else {
                v[2 * r] = p[(size_t)r * W];
                v[2 * r + 1] = p[(size_t)r * W + 1];
            }
        }
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (vec) {
                const f32x4 q = ld4(p + (size_t)r * W);
#pragma unroll
                for (int k = 0; k < 4; ++k) v[4 * r + k] = q[k];
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) v[4 * r + k] = p[(size_t)r * W + k];
            }
        }
    }
}

// q += q_0 + q_1 / 4 + q_2 / 16 of one S x S block of a - b.  No contraction: every slot of a tile runs the same roundings.
template <int L>
__device__ __forceinline__ float block_terms(const float (&a)[(1 << (L - 1)) * (1 << (L - 1))],
                                             const float (&b)[(1 << (L - 1)) * (1 << (L - 1))]) {
#pragma clang fp contract(off)
    constexpr int S = 1 << (L - 1);
    float d[S * S];
#pragma unroll
    for (int k = 0; k < S * S; ++k) d[k] = a[k] - b[k];
    float q0 = 0.f;
#pragma unroll
    for (int k = 0; k < S * S; ++k) q0 += d[k] * d[k];
    if constexpr (L == 1) {
        return q0;
    } else {
        constexpr int S2 = S / 2;
        float t[S2 * S2];
        float q1 = 0.f;
#pragma unroll
        for (int y = 0; y < S2; ++y)
#pragma unroll
            for (int x = 0; x < S2; ++x) {
                const float s = (d[(2 * y) * S + 2 * x] + d[(2 * y) * S + 2 * x + 1]) +
                                (d[(2 * y + 1) * S + 2 * x] + d[(2 * y + 1) * S + 2 * x + 1]);
                t[y * S2 + x] = s;
                q1 += s * s;
            }
        float r = q0 + 0.25f * q1;
        if constexpr (L == 3) {
            const float u = (t[0] + t[1]) + (t[2] + t[3]);
            r += 0.0625f * (u * u);
        }
        return r;
    }
}

__device__ __forceinline__ int list_frame(const int* __restrict__ new_idx, int n_new, const int* __restrict__ cand_idx,
                                          int n_tgt, int s, int T) {
    if (s >= n_tgt) return -1;
    const int f = s < n_new ? new_idx[s] : cand_idx[s - n_new];
    return (f < 0 || f >= T) ? -1 : f;
}

template <int L>
__global__ __launch_bounds__(NT) void frame_dist_rows_kernel(const float* __restrict__ x, int T, int C, int H, int W,
                                                             const int* __restrict__ new_idx, int n_new,
                                                             const int* __restrict__ cand_idx, int n_cand,
                                                             float* __restrict__ dist, int vec) {
    constexpr int S = 1 << (L - 1), E = S * S;
    __shared__ float red[NW][TI * TJ];
    const int b = blockIdx.z, i0 = blockIdx.y * TI, j0 = blockIdx.x * TJ;
    const int n_tgt = n_new + n_cand;
    const size_t D = (size_t)C * H * W;
    const float* __restrict__ xb = x + (size_t)b * T * D;

    // the tile's frames; an absent or refused slot reads frame 0 and is not written
    const float* pa[TI];
    const float* pb[TJ];
#pragma unroll
    for (int ti = 0; ti < TI; ++ti) pa[ti] = xb + (size_t)max(list_frame(new_idx, n_new, cand_idx, n_new, i0 + ti, T), 0) * D;
#pragma unroll
    for (int tj = 0; tj < TJ; ++tj) pb[tj] = xb + (size_t)max(list_frame(new_idx, n_new, cand_idx, n_tgt, j0 + tj, T), 0) * D;

    float q[TI][TJ];
#pragma unroll
    for (int ti = 0; ti < TI; ++ti)
#pragma unroll
        for (int tj = 0; tj < TJ; ++tj) q[ti][tj] = 0.f;

    const int Wb = W / S, per = (H / S) * Wb;
    const long nblk = (long)C * per;
    for (long p = threadIdx.x; p < nblk; p += NT) {
        size_t off = (size_t)p;
        if constexpr (S > 1) {
            const int c = (int)(p / per), r = (int)(p - (long)c * per);
            const int by = r / Wb, bx = r - by * Wb;
            off = ((size_t)c * H + (size_t)by * S) * W + (size_t)bx * S;
        }
        float a[TI][E];
#pragma unroll
        for (int ti = 0; ti < TI; ++ti) load_block<S>(pa[ti] + off, W, vec != 0, a[ti]);
#pragma unroll
        for (int tj = 0; tj < TJ; ++tj) {
            float bb[E];
            load_block<S>(pb[tj] + off, W, vec != 0, bb);
#pragma unroll
            for (int ti = 0; ti < TI; ++ti) q[ti][tj] += block_terms<L>(a[ti], bb);
        }
    }

    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int ti = 0; ti < TI; ++ti)
#pragma unroll
        for (int tj = 0; tj < TJ; ++tj) {
            const float s = wave_sum(q[ti][tj]);
            if ((threadIdx.x & 63) == 0) red[wave][ti * TJ + tj] = s;
        }
    __syncthreads();
    if (threadIdx.x < TI * TJ) {
        const int k = threadIdx.x, ti = k / TJ, tj = k - ti * TJ;
        const int fi = list_frame(new_idx, n_new, cand_idx, n_new, i0 + ti, T);
        const int fj = list_frame(new_idx, n_new, cand_idx, n_tgt, j0 + tj, T);
        if (fi >= 0 && fj >= 0) {
            float tot = red[0][k];
#pragma unroll
            for (int w = 1; w < NW; ++w) tot += red[w][k];
            const float v = fi == fj ? 0.f : (float)((double)tot / ((double)L * (double)D));
            float* __restrict__ db = dist + (size_t)b * T * T;
            db[(size_t)fi * T + fj] = v;
            db[(size_t)fj * T + fi] = v;
        }
    }
}

// numpy's order of the floats: NaN above everything
__device__ __forceinline__ bool np_gt(float a, float b) { return a != a ? b == b : a > b; }
__device__ __forceinline__ bool np_better(float va, int pa, float vb, int pb) {      // (va, pa) wins over (vb, pb)
    if (pa == 0x7fffffff) return false;
    if (pb == 0x7fffffff) return true;
    if (np_gt(va, vb)) return true;
    if (np_gt(vb, va)) return false;
    return pa < pb;
}

__global__ __launch_bounds__(NT) void fps_select_kernel(const float* __restrict__ dist, int T, const int* __restrict__ cand,
                                                        int n_cand, const int* __restrict__ forced, int n_forced, int n,
                                                        int* __restrict__ picks) {
    __shared__ float min_d[FPS_MAX_CAND];
    __shared__ float rv[NW];
    __shared__ int rp[NW];
    __shared__ int cur_s;
    const float* __restrict__ db = dist + (size_t)blockIdx.x * T * T;
    int* __restrict__ pk = picks + (size_t)blockIdx.x * n;
    for (int p = threadIdx.x; p < n_cand; p += NT) min_d[p] = __builtin_inff();
    if (threadIdx.x == 0) {
        int f = forced[0];
        if (f < 0 || f >= n_cand) f = -1;
        cur_s = f;
        pk[0] = f;
    }
    __syncthreads();
    for (int i = 1; i < n; ++i) {
        const int cur = cur_s;                                   // the same for every thread: read before barrier A
        const int row = cur >= 0 ? cand[cur] : -1;
        const bool ok = row >= 0 && row < T;
        const bool is_forced = i < n_forced;
        float bv = 0.f;
        int bp = 0x7fffffff;
        if (ok) {
            const float* __restrict__ dr = db + (size_t)row * T;
            for (int p = threadIdx.x; p < n_cand; p += NT) {
                const int j = cand[p];
                const float v = (j >= 0 && j < T) ? dr[j] : 0.f;
                const float o = min_d[p];
                const float m = (v != v || o != o) ? __builtin_nanf("") : fminf(o, v);
                min_d[p] = m;
                if (np_better(m, p, bv, bp)) {
                    bv = m;
                    bp = p;
                }
            }
            if (!is_forced) {
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const float ov = __shfl_xor(bv, o, 64);
                    const int op = __shfl_xor(bp, o, 64);
                    if (np_better(ov, op, bv, bp)) {
                        bv = ov;
                        bp = op;
                    }
                }
                if ((threadIdx.x & 63) == 0) {
                    rv[threadIdx.x >> 6] = bv;
                    rp[threadIdx.x >> 6] = bp;
                }
            }
        }
        __syncthreads();      // A
        if (threadIdx.x == 0) {
            int nxt = -1;
            if (ok) {
                if (is_forced) {
                    nxt = forced[i];
                    if (nxt < 0 || nxt >= n_cand) nxt = -1;
                } else {
                    float v = rv[0];
                    int p = rp[0];
                    for (int w = 1; w < NW; ++w)
                        if (np_better(rv[w], rp[w], v, p)) {
                            v = rv[w];
                            p = rp[w];
                        }
                    nxt = p;
                }
            }
            cur_s = nxt;
            pk[i] = nxt;
        }
        __syncthreads();      // B
    }
}

}  // namespace

extern "C" int lfvdm_frame_dist_rows(const float* x, int B, int T, int C, int H, int W, int L, const int32_t* new_idx, int n_new,
                                     const int32_t* cand_idx, int n_cand, float* dist, void* stream) {
    if (B <= 0 || T <= 0 || C <= 0 || H <= 0 || W <= 0 || n_new <= 0 || n_cand < 0) return LFVDM_E_SHAPE;
    if (L < 1 || L > 3) return LFVDM_E_SHAPE;
    if (!x || !dist || !new_idx || (n_cand > 0 && !cand_idx)) return LFVDM_E_SHAPE;
    const int S = 1 << (L - 1);
    if (H % S || W % S) return LFVDM_E_SHAPE;
    if ((long)C * H * W > 0x7fffffffL || B > 65535 || T > 65535) return LFVDM_E_SHAPE;
    const long ti = ((long)n_new + TI - 1) / TI, tj = ((long)n_new + n_cand + TJ - 1) / TJ;
    if (ti > 65535 || tj > 0x7fffffffL) return LFVDM_E_SHAPE;
    if (((uintptr_t)x & 3) || ((uintptr_t)dist & 3)) return LFVDM_E_SHAPE;
    // S floats per load where every block row starts on such a boundary: offsets are multiples of S floats already
    const int vec = ((uintptr_t)x & (4 * S - 1)) == 0;
    const dim3 grid((unsigned)tj, (unsigned)ti, (unsigned)B);
#define LFVDM_FD(LV)                                                                                                   \
    hipLaunchKernelGGL((frame_dist_rows_kernel<LV>), grid, dim3(NT), 0, (hipStream_t)stream, x, T, C, H, W, new_idx, n_new, \
                       cand_idx, n_cand, dist, vec)
    if (L == 1) LFVDM_FD(1);
    else if (L == 2) LFVDM_FD(2);
    else LFVDM_FD(3);
#undef LFVDM_FD
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}

extern "C" int lfvdm_fps_select(const float* dist, int B, int T, const int32_t* cand_idx, int n_cand, const int32_t* forced_pos,
                                int n_forced, int n, int32_t* picks, void* stream) {
    if (B <= 0 || T <= 0 || n_cand <= 0 || n_forced <= 0 || n <= 0) return LFVDM_E_SHAPE;
    if (!dist || !cand_idx || !forced_pos || !picks) return LFVDM_E_SHAPE;
    if (T > 65535) return LFVDM_E_SHAPE;
    if (n_cand > FPS_MAX_CAND) return LFVDM_E_UNSUPPORTED;
    hipLaunchKernelGGL(fps_select_kernel, dim3((unsigned)B), dim3(NT), 0, (hipStream_t)stream, dist, T, cand_idx, n_cand,
                       forced_pos, n_forced, n, picks);
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}
