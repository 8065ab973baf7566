// Per-frame mean squared error and mean SSIM of a batch of predicted videos against their ground truth: the two numbers
// behind the PSNR / SSIM curves of conditional video prediction (best of K samples per test video).
//
//   pred (K, N, C, H, W), truth (N, C, H, W), N = videos x frames, float32 or uint8; value = scale * raw + shift in [0, 1].
//   mse[k][n]  = mean over all C H W pixels of (x - y)^2
//   ssim[k][n] = mean over channels and over the (H - 10)(W - 10) valid positions of the SSIM map of Wang et al. 2004:
//                11 x 11 Gaussian window (sigma 1.5, sum 1, separable), no padding, L = 1, C1 = 0.01^2, C2 = 0.03^2,
//                mu_x, mu_y, E[x^2], E[y^2], E[xy] from the same window, biased moments,
//                (2 mu_x mu_y + C1)(2 s_xy + C2) / ((mu_x^2 + mu_y^2 + C1)(s_x^2 + s_y^2 + C2)).
//
// Tile plan.  frame_metrics_kernel: one workgroup of 256 threads per tile of TH x TW = 16 x 32 output positions of one
// (k, n, c) plane; truth is indexed by (n, c) and shared by the K samples.  The workgroup
//   1. stages the (TH + 10) x (TW + 10) input pixels under the tile, of both images, into LDS (16-byte loads where the
//      pointer and the row pitch allow: W a multiple of 4 floats / 16 bytes; scalar loads otherwise), out-of-image pixels
//      as 0, and adds up the squared differences of the pixels it owns;
//   2. runs the horizontal 11-tap pass of the five quantities x, y, x^2, y^2, xy into LDS ((TH + 10) rows x TW columns);
//   3. runs the vertical pass in registers (a thread owns one column and two adjacent rows: 12 LDS rows feed both), forms
//      the SSIM expression and masks positions outside the valid region;
//   4. sums both numbers with wave64 shuffles, then one thread adds the four wave partials in index order and writes
//      them to the workgroup's own slot partials[2 * wg], partials[2 * wg + 1], wg = plane * tiles + tile.
// frame_metrics_finish_kernel: one thread per (k, n) adds its C * tiles slots in index order (in double) and divides.
// No float atomics anywhere: the result is bitwise reproducible from run to run and independent of k.
//
// Who owns which input pixel (the halo is staged by up to four workgroups, its error is counted once).  Pixel (y, x)
// belongs to the tile whose 16 x 32 output block contains (y, x); the last tile row also owns every row below its block
// (down to H - 1) and the last tile column every column right of its block.  The tiles cover the valid positions
// [0, H - 10) x [0, W - 10), so those two strips are the 10 bottom rows and 10 right columns (plus the unused remainder
// of the last block), all of which the last tiles stage anyway.  Each pixel of the plane has exactly one owner.
//
// Accuracy.  The variances are differences of nearly equal numbers, E[x^2] - mu_x^2, and they stand next to C2 = 9e-4.
// On [0, 1] values an fp32 E[x^2] near 0.3 carries about 1e-7 after 22 accumulations, i.e. 1e-4 of C2: too much for a
// flat region, where the SSIM map is a ratio of (C2 + error) terms.  So the tile works on values CENTRED on a pivot, the
// raw value of the pixel in the middle of its staged window, x' = scale (raw - pivot): variances and the covariance are
// shift-invariant, mu_x = (scale pivot_x + shift) + mu_x'.  A constant region containing the pivot gives x' = 0 and
// variances of exactly 0; a smooth region gives |x'| << 1 and the rounding of E[x'^2] shrinks with x'^2.  What is left:
// the moments are sums of 121 products kept to a few ulp (6e-8) of E[x'^2] + E[y'^2] <= 2, typically below 1e-8 absolute,
// i.e. about 1e-5 of C2 per position in the worst placed tile, and these errors are of either sign, so the frame mean
// over thousands of positions sits well below 1e-5.  The squared error uses scale (raw_x - raw_y): the subtraction of
// neighbouring raw values is exact for uint8 and loses nothing to the shift for floats.  Never 0-255 arithmetic.
#include "common_hip.h"

namespace {

constexpr int WIN = 11, HALO = WIN - 1;
constexpr int TH = 16, TW = 32;
constexpr int IH = TH + HALO, IW = TW + HALO;      // staged window: 26 x 42
constexpr int IP = 48;                             // its LDS row pitch: three 16-pixel chunks / twelve 4-float chunks
constexpr int NT = 256;
constexpr float kC1 = 1e-4f, kC2 = 9e-4f;

// exp(-d^2 / 4.5) / sum, d = -5..5
__constant__ const float kG[WIN] = {1.0283800845e-03f, 7.5987581352e-03f, 3.6000772128e-02f, 1.0936068951e-01f,
                                    2.1300553771e-01f, 2.6601172486e-01f, 2.1300553771e-01f, 1.0936068951e-01f,
                                    3.6000772128e-02f, 7.5987581352e-03f, 1.0283800845e-03f};

template <int DT>
struct Pixel;
template <>
struct Pixel<LFVDM_PIX_F32> {
    typedef float raw;
    static constexpr int chunk = 4;      // pixels per 16-byte load
};
template <>
struct Pixel<LFVDM_PIX_U8> {
    typedef uint8_t raw;
    static constexpr int chunk = 16;
};

__device__ __forceinline__ void load_chunk(const float* p, float (&v)[4]) {
    const f32x4 q = ld4(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = q[i];
}
__device__ __forceinline__ void load_chunk(const uint8_t* p, float (&v)[16]) {
    const u32x4 q = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = (float)((q[i >> 2] >> (8 * (i & 3))) & 0xffu);
}

template <int DT, int VEC>
__global__ __launch_bounds__(NT) void frame_metrics_kernel(const typename Pixel<DT>::raw* __restrict__ pred,
                                                           const typename Pixel<DT>::raw* __restrict__ truth, float scale,
                                                           float shift, int NC, int H, int W, int tiles_x, int tiles_y,
                                                           long wg0, float* __restrict__ partials) {
    typedef typename Pixel<DT>::raw raw_t;
    constexpr int CH = Pixel<DT>::chunk;
    __shared__ float xs[IH][IP], ys[IH][IP];
    __shared__ float hq[5][IH][TW];
    __shared__ float red[2][NT / 64];

    const int tiles = tiles_x * tiles_y;
    const long wg = wg0 + blockIdx.x;
    const long plane = wg / tiles;                 // (k * N + n) * C + c
    const int tile = (int)(wg - plane * tiles);
    const int tyi = tile / tiles_x, txi = tile - tyi * tiles_x;
    const int oy0 = tyi * TH, ox0 = txi * TW;
    const raw_t* __restrict__ xp = pred + (size_t)plane * H * W;
    const raw_t* __restrict__ yp = truth + (size_t)(plane % NC) * H * W;
    // pixels this workgroup owns: its output block, extended to the image edge in the last tile row / column
    const int own_y1 = tyi == tiles_y - 1 ? H : oy0 + TH, own_x1 = txi == tiles_x - 1 ? W : ox0 + TW;
    // the pivot: the middle of the staged window, pulled inside the image
    const int py = min(oy0 + IH / 2, H - 1), px = min(ox0 + IW / 2, W - 1);
    const float pvx = (float)xp[(size_t)py * W + px], pvy = (float)yp[(size_t)py * W + px];

    float se = 0.f;
    if (VEC) {
        constexpr int CPR = IP / CH;      // chunks per staged row
        for (int i = threadIdx.x; i < IH * CPR; i += NT) {
            const int r = i / CPR, c0 = (i - r * CPR) * CH;
            const int gy = oy0 + r, gx0 = ox0 + c0;
            float vx[CH], vy[CH];
            const bool in = gy < H && gx0 < W;      // W is a multiple of the chunk: a chunk is inside or outside as a whole
            if (in) {
                load_chunk(xp + (size_t)gy * W + gx0, vx);
                load_chunk(yp + (size_t)gy * W + gx0, vy);
            }
#pragma unroll
            for (int k = 0; k < CH; ++k) {
                float a = 0.f, b = 0.f;
                if (in) {
                    a = scale * (vx[k] - pvx);
                    b = scale * (vy[k] - pvy);
                    if (gy < own_y1 && gx0 + k < own_x1) {
                        const float d = scale * (vx[k] - vy[k]);
                        se += d * d;
                    }
                }
                xs[r][c0 + k] = a;
                ys[r][c0 + k] = b;
            }
        }
    } else {
        for (int i = threadIdx.x; i < IH * IW; i += NT) {
            const int r = i / IW, c = i - r * IW;
            const int gy = oy0 + r, gx = ox0 + c;
            float a = 0.f, b = 0.f;
            if (gy < H && gx < W) {
                const float vx = (float)xp[(size_t)gy * W + gx], vy = (float)yp[(size_t)gy * W + gx];
                a = scale * (vx - pvx);
                b = scale * (vy - pvy);
                if (gy < own_y1 && gx < own_x1) {
                    const float d = scale * (vx - vy);
                    se += d * d;
                }
            }
            xs[r][c] = a;
            ys[r][c] = b;
        }
    }
    __syncthreads();

    // horizontal pass: (row r, output column c) <- 11 taps of x, y, x^2, y^2, xy
    for (int i = threadIdx.x; i < IH * TW; i += NT) {
        const int r = i / TW, c = i - r * TW;
        float mx = 0.f, my = 0.f, xx = 0.f, yy = 0.f, xy = 0.f;
#pragma unroll
        for (int j = 0; j < WIN; ++j) {
            const float g = kG[j], a = xs[r][c + j], b = ys[r][c + j];
            const float ga = g * a, gb = g * b;
            mx += ga;
            my += gb;
            xx += ga * a;
            yy += gb * b;
            xy += ga * b;
        }
        hq[0][r][c] = mx;
        hq[1][r][c] = my;
        hq[2][r][c] = xx;
        hq[3][r][c] = yy;
        hq[4][r][c] = xy;
    }
    __syncthreads();

    // vertical pass: column c, output rows r0 and r0 + 1 share the LDS rows r0 + 1 .. r0 + 10
    const int c = threadIdx.x & (TW - 1), r0 = 2 * (threadIdx.x / TW);
    float acc[2][5];
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
        for (int q = 0; q < 5; ++q) acc[o][q] = 0.f;
#pragma unroll
    for (int j = 0; j <= WIN; ++j) {
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const float v = hq[q][r0 + j][c];
            if (j < WIN) acc[0][q] += kG[j] * v;
            if (j >= 1) acc[1][q] += kG[j - 1] * v;
        }
    }
    const float bx = scale * pvx + shift, by = scale * pvy + shift;
    float ss = 0.f;
#pragma unroll
    for (int o = 0; o < 2; ++o) {
        const float mx = acc[o][0], my = acc[o][1];
        const float sxx = acc[o][2] - mx * mx, syy = acc[o][3] - my * my, sxy = acc[o][4] - mx * my;
        const float ux = bx + mx, uy = by + my;
        const float num = (2.f * ux * uy + kC1) * (2.f * sxy + kC2);
        const float den = (ux * ux + uy * uy + kC1) * (sxx + syy + kC2);
        const bool valid = oy0 + r0 + o < H - HALO && ox0 + c < W - HALO;
        ss += valid ? num / den : 0.f;
    }

    se = wave_sum(se);
    ss = wave_sum(ss);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = se;
        red[1][threadIdx.x >> 6] = ss;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float te = 0.f, ts = 0.f;
        for (int w = 0; w < NT / 64; ++w) {
            te += red[0][w];
            ts += red[1][w];
        }
        partials[2 * wg] = te;
        partials[2 * wg + 1] = ts;
    }
}

// (k, n) <- its C * tiles slots, added in index order
__global__ __launch_bounds__(NT) void frame_metrics_finish_kernel(const float* __restrict__ partials, long frames, int per_frame,
                                                                  double inv_pixels, double inv_positions,
                                                                  float* __restrict__ mse, float* __restrict__ ssim) {
    const long f = (long)blockIdx.x * NT + threadIdx.x;
    if (f >= frames) return;
    const float* __restrict__ p = partials + 2 * f * per_frame;
    double te = 0.0, ts = 0.0;
    for (int i = 0; i < per_frame; ++i) {
        te += (double)p[2 * i];
        ts += (double)p[2 * i + 1];
    }
    mse[f] = (float)(te * inv_pixels);
    ssim[f] = (float)(ts * inv_positions);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// tiles per plane; 0 if the shape is refused
long plane_tiles(int H, int W, int* tiles_x, int* tiles_y) {
    if (H < WIN || W < WIN) return 0;
    *tiles_x = (W - HALO + TW - 1) / TW;
    *tiles_y = (H - HALO + TH - 1) / TH;
    return (long)*tiles_x * *tiles_y;
}

}  // namespace

extern "C" long lfvdm_frame_metrics_workspace(int K, int N, int C, int H, int W) {
    int tx, ty;
    if (K <= 0 || N <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
    const long tiles = plane_tiles(H, W, &tx, &ty);
    const long frames = (long)K * N;
    if (tiles == 0 || frames > 0x7fffffffL || tiles > 0x7fffffffL / C || frames * C > (1L << 60) / tiles) return 0;
    return 2 * frames * C * tiles;
}

extern "C" int lfvdm_frame_metrics(const void* pred, const void* truth, int dtype, float scale, float shift, int K, int N,
                                   int C, int H, int W, float* mse, float* ssim, float* partials, long partials_floats,
                                   void* stream) {
    if (K <= 0 || N <= 0 || C <= 0 || H <= 0 || W <= 0) return LFVDM_E_SHAPE;
    if (H < WIN || W < WIN) return LFVDM_E_SHAPE;
    if (dtype != LFVDM_PIX_F32 && dtype != LFVDM_PIX_U8) return LFVDM_E_SHAPE;
    if (!pred || !truth || !mse || !ssim || !partials) return LFVDM_E_SHAPE;
    int tiles_x, tiles_y;
    const long tiles = plane_tiles(H, W, &tiles_x, &tiles_y);
    const long frames = (long)K * N;
    // the finish kernel's per-frame slot count and the truth's plane index are ints; slot indices fit a long with room
    if (frames > 0x7fffffffL || (long)N * C > 0x7fffffffL || tiles > 0x7fffffffL / C) return LFVDM_E_SHAPE;
    const long planes = frames * C;
    if (planes > (1L << 60) / tiles) return LFVDM_E_SHAPE;
    const long wgs = planes * tiles;
    if (partials_floats < 2 * wgs) return LFVDM_E_SHAPE;
    const int per_pixel = dtype == LFVDM_PIX_U8 ? 1 : 4;
    const int chunk = 16 / per_pixel;
    const int vec = (W % chunk) == 0 && aligned16(pred) && aligned16(truth) && (((size_t)H * W * per_pixel) & 15) == 0;
    // one workgroup per (plane, tile); a launch holds at most kMaxGrid of them (grid x block stays below 2^32 threads), so
    // only an evaluation of more than 16 million tiles takes more than one
    constexpr long kMaxGrid = (1L << 24) - 1;
#define LFVDM_FM(DT, V)                                                                                                  \
    hipLaunchKernelGGL((frame_metrics_kernel<DT, V>), dim3((unsigned)n), dim3(NT), 0, (hipStream_t)stream,                 \
                       (const Pixel<DT>::raw*)pred, (const Pixel<DT>::raw*)truth, scale, shift, N * C, H, W, tiles_x, tiles_y, \
                       wg0, partials)
    for (long wg0 = 0; wg0 < wgs; wg0 += kMaxGrid) {
        const long n = wgs - wg0 < kMaxGrid ? wgs - wg0 : kMaxGrid;
        if (dtype == LFVDM_PIX_U8) {
            if (vec) LFVDM_FM(LFVDM_PIX_U8, 1);
            else LFVDM_FM(LFVDM_PIX_U8, 0);
        } else {
            if (vec) LFVDM_FM(LFVDM_PIX_F32, 1);
            else LFVDM_FM(LFVDM_PIX_F32, 0);
        }
        LFVDM_CHECK_LAUNCH();
    }
#undef LFVDM_FM
    const double inv_pixels = 1.0 / ((double)C * H * W), inv_positions = 1.0 / ((double)C * (H - HALO) * (W - HALO));
    hipLaunchKernelGGL(frame_metrics_finish_kernel, dim3((unsigned)((frames + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream,
                       partials, frames, (int)(C * tiles), inv_pixels, inv_positions, mse, ssim);
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}
