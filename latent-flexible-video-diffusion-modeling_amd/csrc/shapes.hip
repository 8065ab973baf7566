// The "bouncing_shapes" video dataset, rendered on the device (improved_diffusion/shapes.py holds the host reference, which
// was written from this comment).  A few coloured discs and squares move in the frame and bounce off its walls; with
// `stochastic` a wall hit re-draws the velocity, so the future of a clip is multi-modal (Denton & Fergus 2018).  A video is
// a function of (seed, split, video index) and the parameters (H, W, n_shapes, T, stochastic), in INTEGER arithmetic only:
// the kernels and the host reference agree bit for bit.
//
// Units: positions, velocities and radii are fixed point, 1/16 pixel.  x runs along W, y along H.  Lmin = min(H, W).
//
// Random draws: Philox4x32-10 (philox_normal.h), key (k0, k1) = (low, high) word of the 64-bit dataset seed,
//   counter = (shape s, video index (low 32 bits; the Python side keeps indices below 2^32), frame, stream word)
//   stream word = 0x53480000 | split << 8 | purpose        split: 0 train, 1 test;  purpose: 0 INIT, 1 VELOCITY, 2 BOUNCE
//   speed(w)  = 8 + (w >> 8) % 41            8 .. 48 = 0.5 .. 3 pixels per frame
//   signed(w) = (w & 1) ? -speed(w) : speed(w)
// INIT (frame word 0) -> words r0..r3:
//   kind   = r0 & 1                          0 disc, 1 axis-aligned square
//   radius = 2 Lmin + (r0 >> 8) % (2 Lmin + 1)        Lmin/8 .. Lmin/4 pixels (radius of the disc / half side of the square)
//   colour = PALETTE[(r1 >> 8) % 8]          uint8 rgb, none of them the background (0, 0, 0)
//   x0     = radius + r2 % (16 W - 2 radius + 1)
//   y0     = radius + r3 % (16 H - 2 radius + 1)
// VELOCITY (frame word 0):  vx = signed(r0), vy = signed(r1)
// Frame 0 shows (x0, y0).  Frame t >= 1, per axis with lo = radius, hi = 16 L - radius (L = W for x, H for y):
//   p += v;  if p < lo: p = 2 lo - p, v = -v, bounced;  else if p > hi: p = 2 hi - p, v = -v, bounced
//   (hi - lo >= 8 L >= 64 > 48: one reflection always lands inside [lo, hi]).
// With stochastic != 0 and at least one axis bounced at frame t, BOUNCE (frame word t) -> r0..r3, applied after both axes moved:
//   x bounced: vx = sign(vx) speed(r0)  (the reflected direction, a new speed);  x did not bounce but y did: vx = signed(r2)
//   y bounced: vy = sign(vy) speed(r1);                                          y did not bounce but x did: vy = signed(r3)
//
// Coverage of pixel (px, py) by a shape at (cx, cy): the 4 x 4 subsample centres (16 px + 2 + 4 i, 16 py + 2 + 4 j), i, j in
// 0..3, with dx = sx - cx, dy = sy - cy: inside if dx^2 + dy^2 <= radius^2 (disc) or max(|dx|, |dy|) <= radius (square);
// k = number of subsamples inside, 0..16.  |dx|, |dy| < 4096 + 64: the squares fit an int32.
// Colour: painter's order, shape 0 first, over the background; per channel u8 = (prev (16 - k) + colour k + 8) >> 4.
// Output: uint8 [..][3][H][W], or float32 = lut[u8] with the 256-entry table the host computes with the very function that
// converts uint8 frames everywhere else (video_datasets._frames_uint8_to_signed_unit), so the two outputs agree bitwise.
//
// Two launches, both capturable, no atomics, no host synchronisation:
//   lfvdm_shapes_trajectories   one thread per (video, shape), sequential over the T frames (a stochastic bounce has no closed form)
//   lfvdm_shapes_render         grid (frame slot, batch element) as prepare_batch_kernel, times chunks of 256 pixel quads of the
//                               frame (one workgroup per frame leaves the chip idle at a training batch's few dozen frames); a thread owns 4 consecutive
//                               pixels of a row: one 16-byte store per channel (float32) or one packed 4-byte store (uint8)
#include "common_hip.h"
#include "philox_normal.h"

namespace {

enum { SHAPES_STREAM = 0x53480000, SHAPES_INIT = 0, SHAPES_VELOCITY = 1, SHAPES_BOUNCE = 2 };

__constant__ unsigned char SHAPES_PALETTE[8][3] = {{230, 40, 40},  {40, 200, 60},  {60, 90, 240},  {240, 220, 50},
                                                   {230, 60, 220}, {50, 220, 230}, {250, 140, 30}, {245, 245, 245}};

__device__ __forceinline__ int shapes_speed(unsigned w) { return 8 + (int)((w >> 8) % 41u); }
__device__ __forceinline__ int shapes_signed(unsigned w) { return (w & 1u) ? -shapes_speed(w) : shapes_speed(w); }

// traj [n_videos][T][S][2] int32 (x, y); consts [n_videos][S][4] int32 {kind, radius, r | g << 8 | b << 16, 0}
__global__ __launch_bounds__(64) void shapes_trajectories_kernel(const int64_t* __restrict__ video_idx, int32_t* __restrict__ traj,
                                                                 int32_t* __restrict__ consts, unsigned k0, unsigned k1,
                                                                 unsigned stream_base, int n_videos, int T, int S, int H, int W,
                                                                 int stochastic) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_videos * S) return;
    const int v = i / S, s = i - v * S;
    const unsigned vid = (unsigned)(uint64_t)video_idx[v];
    const int Lmin = H < W ? H : W;
    unsigned r[4];
    philox4x32_10((unsigned)s, vid, 0u, stream_base | SHAPES_INIT, k0, k1, r);
    const int kind = (int)(r[0] & 1u);
    const int rad = 2 * Lmin + (int)((r[0] >> 8) % (unsigned)(2 * Lmin + 1));
    const int ci = (int)((r[1] >> 8) % 8u);
    const int xlo = rad, xhi = 16 * W - rad, ylo = rad, yhi = 16 * H - rad;
    int x = rad + (int)(r[2] % (unsigned)(16 * W - 2 * rad + 1));
    int y = rad + (int)(r[3] % (unsigned)(16 * H - 2 * rad + 1));
    philox4x32_10((unsigned)s, vid, 0u, stream_base | SHAPES_VELOCITY, k0, k1, r);
    int vx = shapes_signed(r[0]), vy = shapes_signed(r[1]);
    int32_t* c = consts + (size_t)i * 4;
    c[0] = kind;
    c[1] = rad;
    c[2] = (int)SHAPES_PALETTE[ci][0] | ((int)SHAPES_PALETTE[ci][1] << 8) | ((int)SHAPES_PALETTE[ci][2] << 16);
    c[3] = 0;
    int2* out = reinterpret_cast<int2*>(traj) + (size_t)v * T * S + s;
    out[0] = make_int2(x, y);
    for (int t = 1; t < T; ++t) {
        bool bx = false, by = false;
        x += vx;
        if (x < xlo) { x = 2 * xlo - x; vx = -vx; bx = true; }
        else if (x > xhi) { x = 2 * xhi - x; vx = -vx; bx = true; }
        y += vy;
        if (y < ylo) { y = 2 * ylo - y; vy = -vy; by = true; }
        else if (y > yhi) { y = 2 * yhi - y; vy = -vy; by = true; }
        if (stochastic && (bx || by)) {
            philox4x32_10((unsigned)s, vid, (unsigned)t, stream_base | SHAPES_BOUNCE, k0, k1, r);
            if (bx) vx = vx < 0 ? -shapes_speed(r[0]) : shapes_speed(r[0]);
            else vx = shapes_signed(r[2]);
            if (by) vy = vy < 0 ? -shapes_speed(r[1]) : shapes_speed(r[1]);
            else vy = shapes_signed(r[3]);
        }
        out[(size_t)t * S] = make_int2(x, y);
    }
}

// Row `row` of batch element b is frame row % T of trajectory video b * (Tp / T) + row / T: with Tp = 2 T the rows are those of
// the pool [video 1 | padding video] that lfvdm_prepare_batch gathers from.  table == nullptr: slot f shows row f.
template <bool U8>
__global__ __launch_bounds__(256) void shapes_render_kernel(const int32_t* __restrict__ traj, const int32_t* __restrict__ consts,
                                                            const int32_t* __restrict__ table, const float* __restrict__ lut,
                                                            void* __restrict__ out_, int64_t* __restrict__ frame_indices,
                                                            float* __restrict__ obs_mask, float* __restrict__ latent_mask, int F,
                                                            int Tp, int T, int S, int H, int W) {
    __shared__ float lut_s[256];
    const int f = blockIdx.x, b = blockIdx.y;
    int row = f;
    if (table) {
        const int32_t* e = table + ((size_t)b * F + f) * 4;
        row = e[0];
        row = row < 0 ? 0 : (row >= Tp ? Tp - 1 : row);      // a corrupt table must not read outside the trajectory table
        if (frame_indices && threadIdx.x == 0 && blockIdx.z == 0) {
            frame_indices[(size_t)b * F + f] = (int64_t)e[1];
            obs_mask[(size_t)b * F + f] = e[2] ? 1.f : 0.f;
            latent_mask[(size_t)b * F + f] = e[3] ? 1.f : 0.f;
        }
    }
    const int sub = row / T, frame = row - sub * T;
    const size_t video = (size_t)b * (Tp / T) + sub;
    if (!U8) {
        lut_s[threadIdx.x] = lut[threadIdx.x];
        __syncthreads();
    }
    int cx[4], cy[4], rad[4], kind[4], rgb[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        if (s < S) {
            const int32_t* p = traj + ((video * T + frame) * S + s) * 2;
            const int32_t* c = consts + (video * S + s) * 4;
            cx[s] = p[0]; cy[s] = p[1]; kind[s] = c[0]; rad[s] = c[1]; rgb[s] = c[2];
        } else {
            cx[s] = cy[s] = rad[s] = kind[s] = rgb[s] = 0;
        }
    }
    const int wq = W >> 2, nq = H * wq, HW = H * W;
    const size_t base = ((size_t)b * F + f) * 3 * HW;
    for (int q = blockIdx.z * 256 + threadIdx.x; q < nq; q += 256 * gridDim.z) {
        const int py = q / wq, px0 = (q - py * wq) << 2;
        const int sx0 = 16 * px0 + 2, sy0 = 16 * py + 2;      // first subsample centre of the quad
        int col[4][3] = {};                                    // background (0, 0, 0)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            if (s >= S) break;
            // bounding box against the quad's subsample centres: x in [sx0, sx0 + 60], y in [sy0, sy0 + 12]
            if (cx[s] + rad[s] < sx0 || cx[s] - rad[s] > sx0 + 60 || cy[s] + rad[s] < sy0 || cy[s] - rad[s] > sy0 + 12) continue;
            const int r2 = rad[s] * rad[s];
            int k[4] = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int dy = sy0 + 4 * j - cy[s];
                const int ady = dy < 0 ? -dy : dy;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int dx = sx0 + 4 * i - cx[s];       // subsample i & 3 of pixel px0 + (i >> 2)
                    const int adx = dx < 0 ? -dx : dx;
                    const bool in = kind[s] ? ((adx > ady ? adx : ady) <= rad[s]) : (dx * dx + dy * dy <= r2);
                    k[i >> 2] += in ? 1 : 0;
                }
            }
#pragma unroll
            for (int p = 0; p < 4; ++p) {
#pragma unroll
                for (int c = 0; c < 3; ++c) col[p][c] = (col[p][c] * (16 - k[p]) + ((rgb[s] >> (8 * c)) & 255) * k[p] + 8) >> 4;
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const size_t at = base + (size_t)c * HW + (size_t)q * 4;
            if (U8) {
                const unsigned w = (unsigned)col[0][c] | ((unsigned)col[1][c] << 8) | ((unsigned)col[2][c] << 16) |
                                   ((unsigned)col[3][c] << 24);
                *reinterpret_cast<unsigned*>(static_cast<unsigned char*>(out_) + at) = w;
            } else {
                st4(static_cast<float*>(out_) + at, (f32x4){lut_s[col[0][c]], lut_s[col[1][c]], lut_s[col[2][c]], lut_s[col[3][c]]});
            }
        }
    }
}

bool shapes_params_ok(int T, int S, int H, int W) {
    return T >= 1 && T <= 1024 && S >= 1 && S <= 4 && H >= 8 && H <= 256 && W >= 8 && W <= 256 && !(H & 3) && !(W & 3);
}

}  // namespace

extern "C" int lfvdm_shapes_trajectories(const int64_t* video_idx, int32_t* traj, int32_t* consts, uint64_t seed, int split,
                                         int n_videos, int T, int n_shapes, int H, int W, int stochastic, void* stream) {
    if (!video_idx || !traj || !consts) return LFVDM_E_SHAPE;
    if (!shapes_params_ok(T, n_shapes, H, W) || n_videos <= 0 || n_videos > 2 * 65535 || split < 0 || split > 1) return LFVDM_E_SHAPE;
    if (reinterpret_cast<uintptr_t>(traj) & 7) return LFVDM_E_SHAPE;
    const int n = n_videos * n_shapes;
    hipLaunchKernelGGL(shapes_trajectories_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, video_idx, traj,
                       consts, (unsigned)(seed & 0xFFFFFFFFu), (unsigned)(seed >> 32),
                       (unsigned)SHAPES_STREAM | ((unsigned)split << 8), n_videos, T, n_shapes, H, W, stochastic);
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}

extern "C" int lfvdm_shapes_render(const int32_t* traj, const int32_t* consts, const int32_t* table, const float* lut, void* out,
                                   int dtype, int64_t* frame_indices, float* obs_mask, float* latent_mask, int B, int F, int Tp, int T,
                                   int n_shapes, int H, int W, void* stream) {
    if (!traj || !consts || !out) return LFVDM_E_SHAPE;
    if (dtype != LFVDM_PIX_F32 && dtype != LFVDM_PIX_U8) return LFVDM_E_UNSUPPORTED;
    if (dtype == LFVDM_PIX_F32 && !lut) return LFVDM_E_SHAPE;
    const int n_meta = (frame_indices != nullptr) + (obs_mask != nullptr) + (latent_mask != nullptr);
    if ((n_meta != 0 && n_meta != 3) || (n_meta == 3 && !table)) return LFVDM_E_SHAPE;      // all three with a table, or none
    if (!shapes_params_ok(T, n_shapes, H, W)) return LFVDM_E_SHAPE;
    if (B <= 0 || B > 65535 || F <= 0 || Tp < T || Tp % T || Tp / T > 2 || (!table && F > Tp)) return LFVDM_E_SHAPE;
    if (reinterpret_cast<uintptr_t>(out) & (dtype == LFVDM_PIX_F32 ? 15 : 3)) return LFVDM_E_SHAPE;
    // a training batch is a few dozen frames: one workgroup per frame would leave most of the chip idle (measured: 64 us for
    // 2 x 20 frames of 128 x 128), so a frame's quads are split into chunks of 256 along grid.z (at most 64: 256 x 256 pixels)
    const dim3 grid(F, B, (H * (W >> 2) + 255) / 256);
    if (dtype == LFVDM_PIX_U8)
        hipLaunchKernelGGL(shapes_render_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, traj, consts, table, lut, out,
                           frame_indices, obs_mask, latent_mask, F, Tp, T, n_shapes, H, W);
    else
        hipLaunchKernelGGL(shapes_render_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, traj, consts, table, lut, out,
                           frame_indices, obs_mask, latent_mask, F, Tp, T, n_shapes, H, W);
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}
