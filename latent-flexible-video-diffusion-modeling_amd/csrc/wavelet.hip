// Haar wavelet diffusion space: pixels (N, C, H, W) <-> coefficients (N, 4^L C, H / 2^L, W / 2^L), L = 1 or 2 levels.
//
// One level maps the 2 x 2 block [[a, b], [c, d]] (rows, then columns) of a channel to four bands, in this order:
//   ll = s (a + b + c + d)    lh = s (a - b + c - d)  (difference along the width)
//   hl = s (a + b - c - d)  (difference along the height)    hh = s (a - b - c + d)
// s = 1/4 (LFVDM_WAVELET_RANGE: pixels in [-1, 1] give coefficients in [-1, 1] in every band) or 1/2
// (LFVDM_WAVELET_ORTHONORMAL: an isometry).  The inverse is the same butterfly times 1 / (4 s).
//
// Layout.  L = 1: channel blocks [ll | lh | hl | hh] of C channels each.  L = 2: the level is applied again to ll, and the
// three level-1 detail bands come to quarter resolution by space-to-depth, phase = 2 (row & 1) + (column & 1):
//   [ll2 | lh2 | hl2 | hh2 | lh1 phase 0..3 | hl1 phase 0..3 | hh1 phase 0..3], 16 blocks of C channels: channel k C + c.
// Optional per-coefficient-channel standardisation: encode ends with y = (y - mean[q]) * rstd[q], decode starts with
// y * std[q] + mean[q] (q over the 4^L C channels).
//
// Thread plan.  HBM-bound: every pixel is read once and every coefficient written once, everything in between lives in
// registers (no LDS, no atomics).  A thread owns, of one channel of one frame,
//   L = 2:               one 4 x 4 pixel block: four 16-byte row loads (float4; uchar4 for uint8), 16 coefficients, one
//                        4-byte store into each of the 16 planes;
//   L = 1, vector path:  two neighbouring 2 x 2 blocks: two row loads of four pixels, one 8-byte store into each plane;
//   L = 1, scalar path:  one 2 x 2 block.
// Consecutive lanes take consecutive output columns, so each plane store of a wave is one contiguous run (256 or 512
// bytes) and the row loads of a wave are contiguous too.  The vector path needs W a multiple of 4 and base pointers
// aligned to the access (16 bytes for float pixels, 4 for uint8, 8 for the L = 1 coefficient pairs); everything else
// takes the scalar path of the same arithmetic - results are bitwise equal on either path.
//
// Arithmetic: value = fma(scale, raw, shift); each butterfly is two levels of additions and one multiplication by a power
// of two: three roundings per level, none depending on the path or the launch geometry.  The decode's uint8 output is
// clamp(round-to-nearest-even((x + 1) 127.5), 0, 255): it ROUNDS (a `.to(uint8)` cast truncates), which is what makes
// uint8 -> encode -> decode the identity.
//
// lfvdm_prepare_batch_wavelet is lfvdm_prepare_batch with the encode folded into the gather: the same index table, the
// same clamp of a corrupt row, the same three mask / index outputs; frame (b, f) of the batch is the transform of
// pool frame (b, row).  Same device function as the encode: bitwise the two launches it replaces.
#include "common_hip.h"

namespace {

constexpr int NT = 256;

template <int DT>
struct Pix;
template <>
struct Pix<LFVDM_PIX_F32> {
    typedef float raw;
};
template <>
struct Pix<LFVDM_PIX_U8> {
    typedef uint8_t raw;
};

// CW raw pixels of one row -> floats (VEC: CW == 4, one 16-byte / 4-byte load)
template <int CW, int VEC>
__device__ __forceinline__ void load_row(const float* p, float (&v)[CW]) {
    if (VEC) {
        const f32x4 q = ld4(p);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = q[i];
    } else {
#pragma unroll
        for (int i = 0; i < CW; ++i) v[i] = p[i];
    }
}
template <int CW, int VEC>
__device__ __forceinline__ void load_row(const uint8_t* p, float (&v)[CW]) {
    if (VEC) {
        const uint32_t q = *reinterpret_cast<const uint32_t*>(p);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = (float)((q >> (8 * i)) & 0xffu);
    } else {
#pragma unroll
        for (int i = 0; i < CW; ++i) v[i] = (float)p[i];
    }
}

template <int CW, int VEC>
__device__ __forceinline__ void store_row(float* p, const float (&v)[CW]) {
    if (VEC) {
        st4(p, (f32x4){v[0], v[1], v[2], v[3]});
    } else {
#pragma unroll
        for (int i = 0; i < CW; ++i) p[i] = v[i];
    }
}
__device__ __forceinline__ uint32_t to_u8(float x) {
    const float r = rintf(__builtin_fmaf(x, 127.5f, 127.5f));      // round to nearest (even)
    return (uint32_t)fminf(fmaxf(r, 0.f), 255.f);                  // a NaN clamps to 0
}
template <int CW, int VEC>
__device__ __forceinline__ void store_row(uint8_t* p, const float (&v)[CW]) {
    if (VEC) {
        *reinterpret_cast<uint32_t*>(p) = to_u8(v[0]) | (to_u8(v[1]) << 8) | (to_u8(v[2]) << 16) | (to_u8(v[3]) << 24);
    } else {
#pragma unroll
        for (int i = 0; i < CW; ++i) p[i] = (uint8_t)to_u8(v[i]);
    }
}

// [[a, b], [c, d]] -> o[0..3] = ll, lh, hl, hh
__device__ __forceinline__ void haar(float a, float b, float c, float d, float s, float (&o)[4]) {
    const float p = a + b, q = c + d, r = a - b, t = c - d;
    o[0] = s * (p + q);
    o[1] = s * (r + t);
    o[2] = s * (p - q);
    o[3] = s * (r - t);
}
// ll, lh, hl, hh -> a, b, c, d
__device__ __forceinline__ void ihaar(float ll, float lh, float hl, float hh, float k, float& a, float& b, float& c, float& d) {
    const float p = ll + lh, q = ll - lh, r = hl + hh, t = hl - hh;
    a = k * (p + r);
    b = k * (q + t);
    c = k * (p - r);
    d = k * (q - t);
}

template <int L, int VEC>
struct Tile {
    static constexpr int TX = (L == 1 && VEC) ? 2 : 1;      // output columns per thread
    static constexpr int CW = TX << L;                      // pixel columns per thread
    static constexpr int R = 1 << L;                        // pixel rows per thread
    static constexpr int K = 1 << (2 * L);                  // planes per pixel channel
};

struct Where {
    long n;      // frame
    int c, oy, ox0;
};
// thread index -> (frame, channel, output row, first output column); Wg = threads per output row
__device__ __forceinline__ Where locate(long i, int C, int Ho, int Wg, int TX) {
    Where w;
    const long t = i / Wg;
    w.ox0 = (int)(i - t * Wg) * TX;
    const long p = t / Ho;
    w.oy = (int)(t - p * Ho);
    w.n = p / C;
    w.c = (int)(p - w.n * C);
    return w;
}

// the coefficients of one thread's tile of channel c of the frame at `src` -> its planes of the frame at `dst`
template <int L, int DT, int VEC>
__device__ __forceinline__ void encode_tile(const typename Pix<DT>::raw* __restrict__ src, float* __restrict__ dst, float scale,
                                            float shift, float s, const float* __restrict__ mean,
                                            const float* __restrict__ rstd, int C, int H, int W, const Where& w) {
    typedef Tile<L, VEC> T;
    const int Ho = H >> L, Wo = W >> L;
    float px[T::R][T::CW];
    const typename Pix<DT>::raw* __restrict__ row0 = src + ((size_t)w.c * H + ((size_t)w.oy << L)) * W + ((size_t)w.ox0 << L);
#pragma unroll
    for (int r = 0; r < T::R; ++r) {
        load_row<T::CW, VEC>(row0 + (size_t)r * W, px[r]);
#pragma unroll
        for (int x = 0; x < T::CW; ++x) px[r][x] = __builtin_fmaf(scale, px[r][x], shift);
    }
    float out[T::K][T::TX];
    if (L == 1) {
#pragma unroll
        for (int j = 0; j < T::TX; ++j) {
            float o[4];
            haar(px[0][2 * j], px[0][2 * j + 1], px[1][2 * j], px[1][2 * j + 1], s, o);
#pragma unroll
            for (int k = 0; k < 4; ++k) out[k][j] = o[k];
        }
    } else {
        float l1[2][2];
#pragma unroll
        for (int py = 0; py < 2; ++py)
#pragma unroll
            for (int qx = 0; qx < 2; ++qx) {
                float o[4];
                haar(px[2 * py][2 * qx], px[2 * py][2 * qx + 1], px[2 * py + 1][2 * qx], px[2 * py + 1][2 * qx + 1], s, o);
                l1[py][qx] = o[0];
#pragma unroll
                for (int band = 1; band < 4; ++band) out[4 + (band - 1) * 4 + 2 * py + qx][0] = o[band];
            }
        float o[4];
        haar(l1[0][0], l1[0][1], l1[1][0], l1[1][1], s, o);
#pragma unroll
        for (int k = 0; k < 4; ++k) out[k][0] = o[k];
    }
#pragma unroll
    for (int k = 0; k < T::K; ++k) {
        const int q = k * C + w.c;
        if (mean) {
            const float m = mean[q], rs = rstd[q];
#pragma unroll
            for (int j = 0; j < T::TX; ++j) out[k][j] = (out[k][j] - m) * rs;
        }
        float* __restrict__ o = dst + ((size_t)q * Ho + w.oy) * Wo + w.ox0;
        if (T::TX == 2) *reinterpret_cast<f32x2*>(o) = (f32x2){out[k][0], out[k][T::TX - 1]};
        else o[0] = out[k][0];
    }
}

template <int L, int DT, int VEC>
__global__ __launch_bounds__(NT) void wavelet_encode_kernel(const typename Pix<DT>::raw* __restrict__ pix, float* __restrict__ coef,
                                                            float scale, float shift, float s, const float* __restrict__ mean,
                                                            const float* __restrict__ rstd, int C, int H, int W, int Wg,
                                                            long total) {
    const long i = (long)blockIdx.x * NT + threadIdx.x;
    if (i >= total) return;
    const Where w = locate(i, C, H >> L, Wg, Tile<L, VEC>::TX);
    const size_t frame = (size_t)C * H * W;
    encode_tile<L, DT, VEC>(pix + w.n * frame, coef + w.n * frame, scale, shift, s, mean, rstd, C, H, W, w);
}

template <int L, int DT, int VEC>
__global__ __launch_bounds__(NT) void prepare_batch_wavelet_kernel(const typename Pix<DT>::raw* __restrict__ pool,
                                                                   const int32_t* __restrict__ table, float* __restrict__ batch,
                                                                   int64_t* __restrict__ frame_indices, float* __restrict__ obs_mask,
                                                                   float* __restrict__ latent_mask, float scale, float shift,
                                                                   float s, const float* __restrict__ mean,
                                                                   const float* __restrict__ rstd, int F, int Tp, int C, int H,
                                                                   int W, int Wg, long total) {
    const long i = (long)blockIdx.x * NT + threadIdx.x;
    if (i >= total) return;
    const Where w = locate(i, C, H >> L, Wg, Tile<L, VEC>::TX);      // w.n = b * F + f
    const int32_t* e = table + w.n * 4;
    int row = e[0];
    row = row < 0 ? 0 : (row >= Tp ? Tp - 1 : row);          // a corrupt table must not read outside the pool
    const long b = w.n / F;
    const size_t frame = (size_t)C * H * W;
    encode_tile<L, DT, VEC>(pool + ((size_t)b * Tp + row) * frame, batch + w.n * frame, scale, shift, s, mean, rstd, C, H, W, w);
    if (w.c == 0 && w.oy == 0 && w.ox0 == 0) {
        frame_indices[w.n] = (int64_t)e[1];
        obs_mask[w.n] = e[2] ? 1.f : 0.f;
        latent_mask[w.n] = e[3] ? 1.f : 0.f;
    }
}

template <int L, int DT, int VEC>
__global__ __launch_bounds__(NT) void wavelet_decode_kernel(const float* __restrict__ coef, typename Pix<DT>::raw* __restrict__ pix,
                                                            float k, const float* __restrict__ mean,
                                                            const float* __restrict__ sd, int C, int H, int W, int Wg, long total) {
    typedef Tile<L, VEC> T;
    const long i = (long)blockIdx.x * NT + threadIdx.x;
    if (i >= total) return;
    const Where w = locate(i, C, H >> L, Wg, T::TX);
    const int Ho = H >> L, Wo = W >> L;
    const size_t frame = (size_t)C * H * W;
    const float* __restrict__ src = coef + w.n * frame;
    float in[T::K][T::TX];
#pragma unroll
    for (int kk = 0; kk < T::K; ++kk) {
        const int q = kk * C + w.c;
        const float* __restrict__ p = src + ((size_t)q * Ho + w.oy) * Wo + w.ox0;
        if (T::TX == 2) {
            const f32x2 v = *reinterpret_cast<const f32x2*>(p);
            in[kk][0] = v[0];
            in[kk][T::TX - 1] = v[1];
        } else {
            in[kk][0] = p[0];
        }
        if (mean) {
            const float m = mean[q], sq = sd[q];
#pragma unroll
            for (int j = 0; j < T::TX; ++j) in[kk][j] = __builtin_fmaf(in[kk][j], sq, m);
        }
    }
    float px[T::R][T::CW];
    if (L == 1) {
#pragma unroll
        for (int j = 0; j < T::TX; ++j)
            ihaar(in[0][j], in[1][j], in[2][j], in[3][j], k, px[0][2 * j], px[0][2 * j + 1], px[1][2 * j], px[1][2 * j + 1]);
    } else {
        float l1[2][2];
        ihaar(in[0][0], in[1][0], in[2][0], in[3][0], k, l1[0][0], l1[0][1], l1[1][0], l1[1][1]);
#pragma unroll
        for (int py = 0; py < 2; ++py)
#pragma unroll
            for (int qx = 0; qx < 2; ++qx) {
                const int ph = 2 * py + qx;
                ihaar(l1[py][qx], in[4 + ph][0], in[8 + ph][0], in[12 + ph][0], k, px[2 * py][2 * qx], px[2 * py][2 * qx + 1],
                      px[2 * py + 1][2 * qx], px[2 * py + 1][2 * qx + 1]);
            }
    }
    typename Pix<DT>::raw* __restrict__ row0 =
        pix + w.n * frame + ((size_t)w.c * H + ((size_t)w.oy << L)) * W + ((size_t)w.ox0 << L);
#pragma unroll
    for (int r = 0; r < T::R; ++r) store_row<T::CW, VEC>(row0 + (size_t)r * W, px[r]);
}

bool aligned(const void* p, int a) { return ((uintptr_t)p & (uintptr_t)(a - 1)) == 0; }

// LFVDM_OK, or why the transform of (frames, C, H, W) pixels is refused; *s: the forward scale
int check_shape(long frames, int C, int H, int W, int levels, int norm, int dtype, float* s) {
    if (frames <= 0 || C <= 0 || H <= 0 || W <= 0) return LFVDM_E_SHAPE;
    if (dtype != LFVDM_PIX_F32 && dtype != LFVDM_PIX_U8) return LFVDM_E_SHAPE;
    if (norm != LFVDM_WAVELET_RANGE && norm != LFVDM_WAVELET_ORTHONORMAL) return LFVDM_E_SHAPE;
    if (levels != 1 && levels != 2) return LFVDM_E_UNSUPPORTED;
    const int m = (1 << levels) - 1;
    if ((H & m) || (W & m)) return LFVDM_E_SHAPE;
    // element counts stay below 2^31: (C H W) first, so that no product overflows a long
    const long chw = (long)C * H;
    if (chw > (1L << 31) / W || frames > (1L << 31) / (chw * W)) return LFVDM_E_UNSUPPORTED;
    *s = norm == LFVDM_WAVELET_RANGE ? 0.25f : 0.5f;
    return LFVDM_OK;
}

// the vector path: W a multiple of 4, pixel rows aligned to their 4-pixel access, coefficient pairs (L = 1) to 8 bytes
bool vector_ok(const void* pix, const float* coef, int dtype, int W, int levels) {
    return (W & 3) == 0 && aligned(pix, dtype == LFVDM_PIX_U8 ? 4 : 16) && aligned(coef, levels == 1 ? 8 : 4);
}

}  // namespace

#define LFVDM_WV_DISPATCH(LAUNCH)                                  \
    do {                                                           \
        if (levels == 1) {                                         \
            if (dtype == LFVDM_PIX_U8) {                           \
                if (vec) LAUNCH(1, LFVDM_PIX_U8, 1);               \
                else LAUNCH(1, LFVDM_PIX_U8, 0);                   \
            } else {                                               \
                if (vec) LAUNCH(1, LFVDM_PIX_F32, 1);              \
                else LAUNCH(1, LFVDM_PIX_F32, 0);                  \
            }                                                      \
        } else {                                                   \
            if (dtype == LFVDM_PIX_U8) {                           \
                if (vec) LAUNCH(2, LFVDM_PIX_U8, 1);               \
                else LAUNCH(2, LFVDM_PIX_U8, 0);                   \
            } else {                                               \
                if (vec) LAUNCH(2, LFVDM_PIX_F32, 1);              \
                else LAUNCH(2, LFVDM_PIX_F32, 0);                  \
            }                                                      \
        }                                                          \
    } while (0)

extern "C" int lfvdm_wavelet_encode(const void* pix, int dtype, float scale, float shift, float* coef, const float* mean,
                                    const float* rstd, int N, int C, int H, int W, int levels, int norm, void* stream) {
    float s;
    if (!pix || !coef || (mean == nullptr) != (rstd == nullptr)) return LFVDM_E_SHAPE;
    const int rc = check_shape(N, C, H, W, levels, norm, dtype, &s);
    if (rc != LFVDM_OK) return rc;
    const int vec = vector_ok(pix, coef, dtype, W, levels);
    const int Wg = (W >> levels) / ((levels == 1 && vec) ? 2 : 1);
    const long total = (long)N * C * (H >> levels) * Wg;
#define LFVDM_WV_ENC(L, DT, V)                                                                                                  \
    hipLaunchKernelGGL((wavelet_encode_kernel<L, DT, V>), dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream, \
                       (const Pix<DT>::raw*)pix, coef, scale, shift, s, mean, rstd, C, H, W, Wg, total)
    LFVDM_WV_DISPATCH(LFVDM_WV_ENC);
#undef LFVDM_WV_ENC
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}

extern "C" int lfvdm_wavelet_decode(const float* coef, const float* mean, const float* std, void* pix, int dtype, int N, int C,
                                    int H, int W, int levels, int norm, void* stream) {
    float s;
    if (!pix || !coef || (mean == nullptr) != (std == nullptr)) return LFVDM_E_SHAPE;
    const int rc = check_shape(N, C, H, W, levels, norm, dtype, &s);
    if (rc != LFVDM_OK) return rc;
    const float k = 0.25f / s;
    const int vec = vector_ok(pix, coef, dtype, W, levels);
    const int Wg = (W >> levels) / ((levels == 1 && vec) ? 2 : 1);
    const long total = (long)N * C * (H >> levels) * Wg;
#define LFVDM_WV_DEC(L, DT, V)                                                                                                  \
    hipLaunchKernelGGL((wavelet_decode_kernel<L, DT, V>), dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream, \
                       coef, (Pix<DT>::raw*)pix, k, mean, std, C, H, W, Wg, total)
    LFVDM_WV_DISPATCH(LFVDM_WV_DEC);
#undef LFVDM_WV_DEC
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}

extern "C" int lfvdm_prepare_batch_wavelet(const void* pool, int dtype, float scale, float shift, const int32_t* table,
                                           float* batch, int64_t* frame_indices, float* obs_mask, float* latent_mask,
                                           const float* mean, const float* rstd, int B, int F, int Tp, int C, int H, int W,
                                           int levels, int norm, void* stream) {
    float s;
    if (!pool || !table || !batch || !frame_indices || !obs_mask || !latent_mask) return LFVDM_E_SHAPE;
    if ((mean == nullptr) != (rstd == nullptr)) return LFVDM_E_SHAPE;
    if (B <= 0 || F <= 0 || Tp <= 0 || B > 65535) return LFVDM_E_SHAPE;
    int rc = check_shape((long)B * F, C, H, W, levels, norm, dtype, &s);
    if (rc == LFVDM_OK) rc = check_shape((long)B * Tp, C, H, W, levels, norm, dtype, &s);      // the pool stays below 2^31 too
    if (rc != LFVDM_OK) return rc;
    // frames start at multiples of C H W pixels: with W a multiple of 4 (and H of 2) every frame keeps the base's alignment
    const int vec = vector_ok(pool, batch, dtype, W, levels);
    const int Wg = (W >> levels) / ((levels == 1 && vec) ? 2 : 1);
    const long total = (long)B * F * C * (H >> levels) * Wg;
#define LFVDM_WV_PREP(L, DT, V)                                                                                                 \
    hipLaunchKernelGGL((prepare_batch_wavelet_kernel<L, DT, V>), dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0,         \
                       (hipStream_t)stream, (const Pix<DT>::raw*)pool, table, batch, frame_indices, obs_mask, latent_mask,     \
                       scale, shift, s, mean, rstd, F, Tp, C, H, W, Wg, total)
    LFVDM_WV_DISPATCH(LFVDM_WV_PREP);
#undef LFVDM_WV_PREP
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}
