// Global-norm gradient clipping and the non-finite step skip of the fused optimizer, without a host synchronisation:
//   lfvdm_grad_norm_partials : one fp32 partial of sum (grad_scale*g)^2 per workgroup (one extra read of the gradient arena)
//   lfvdm_grad_norm_finalize : the partials added in index order in double -> {squared norm, clip coefficient, non-finite
//                              flag, running count of skipped steps}
//   lfvdm_adamw_ema_clip     : the AdamW + EMA launch (adamw_ema_body.h) with the gradient scaled by the coefficient, a
//                              no-op when the flag is up
// (torch.nn.utils.clip_grad_norm_ followed by opt.step(): one `.item()`-free norm per tensor and a foreach multiply there).
// Nothing here uses a float atomic or a "last workgroup" counter: the grid depends on n alone and every sum has a fixed
// order, so the record - and with it the clipped update - is bitwise reproducible from run to run.
#include "adamw_ema_body.h"

namespace {

constexpr int GN_THREADS = 256;
constexpr int GN_U = 4;                       // float4 loads in flight per thread
constexpr int64_t GN_QUADS_PER_WG = 4096;     // a workgroup sums at least this many float4 (4 passes) before the grid grows

// `g` may start anywhere on a 4-byte boundary: up to three leading floats (the scalar head) bring the float4 stream to a
// 16-byte boundary, up to three trailing floats (the scalar tail) finish it; both belong to workgroup 0.
__global__ __launch_bounds__(GN_THREADS) void grad_norm_partials_kernel(const float* g, int64_t n, float gs, float* partials) {
    int64_t head = (int64_t)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(g) & 15u)) & 15u) >> 2);
    if (head > n) head = n;
    const float* gb = g + head;
    const int64_t nb = n - head, n4 = nb / 4;
    const int tail = (int)(nb & 3);
    float sq = 0.f;
    const int64_t stride = (int64_t)gridDim.x * GN_THREADS;
    for (int64_t i0 = (int64_t)blockIdx.x * GN_THREADS + threadIdx.x; i0 < n4; i0 += GN_U * stride) {
        f32x4 q[GN_U];
        bool live[GN_U];
#pragma unroll
        for (int u = 0; u < GN_U; ++u) {              // every load of the pass is issued before the first use
            const int64_t i = i0 + u * stride;
            live[u] = i < n4;
            q[u] = ld4(gb + (live[u] ? i : i0) * 4);  // (a clamped duplicate load; its result is not used)
        }
#pragma unroll
        for (int u = 0; u < GN_U; ++u) {
            const f32x4 x = q[u] * gs;
            const float s = x.x * x.x + x.y * x.y + x.z * x.z + x.w * x.w;
            sq += live[u] ? s : 0.f;
        }
    }
    if (blockIdx.x == 0 && (int)threadIdx.x < (int)head + tail) {
        const int64_t i = (int)threadIdx.x < (int)head ? (int64_t)threadIdx.x : head + n4 * 4 + ((int)threadIdx.x - (int)head);
        const float x = g[i] * gs;
        sq += x * x;
    }
    sq = wave_sum(sq);
    __shared__ float red[GN_THREADS / 64];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sq;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(GN_THREADS) void grad_norm_finalize_kernel(const float* partials, int nparts, float max_norm, float* stat) {
    __shared__ float sp[LFVDM_GRAD_NORM_MAX_PARTS];
    for (int i = threadIdx.x; i < nparts; i += GN_THREADS) sp[i] = partials[i];
    __syncthreads();
    if (threadIdx.x != 0) return;
    double s = 0.0;
    for (int i = 0; i < nparts; ++i) s += (double)sp[i];          // index order, whatever the grid that wrote them
    const float sqn = (float)s;
    const float norm = (float)sqrt(s);
    const int bad = !(fabsf(sqn) <= 3.402823466e+38f);            // inf or NaN (an fp32 overflow of the squared norm included)
    float coef = 1.0f;
    if (max_norm > 0.f) coef = fminf(1.0f, max_norm / (norm + 1e-6f));   // torch.nn.utils.clip_grad_norm_
    if (bad) coef = 0.f;                                           // (not used: the optimizer launch skips)
    int32_t* si = reinterpret_cast<int32_t*>(stat);
    const int32_t skipped = si[3] + bad;
    stat[0] = sqn;
    stat[1] = coef;
    si[2] = bad;
    si[3] = skipped;
}

}  // namespace

extern "C" int lfvdm_grad_norm_nparts(int64_t n) {
    if (n <= 0) return 0;
    int64_t parts = (n / 4 + GN_QUADS_PER_WG - 1) / GN_QUADS_PER_WG;
    if (parts > LFVDM_GRAD_NORM_MAX_PARTS) parts = LFVDM_GRAD_NORM_MAX_PARTS;
    if (parts < 1) parts = 1;
    return (int)parts;
}

extern "C" int lfvdm_grad_norm_partials(const float* g, int64_t n, float grad_scale, float* partials, int nparts, void* stream) {
    if (n <= 0 || nparts != lfvdm_grad_norm_nparts(n) || (reinterpret_cast<uintptr_t>(g) & 3u)) return LFVDM_E_SHAPE;
    hipLaunchKernelGGL(grad_norm_partials_kernel, dim3((unsigned)nparts), dim3(GN_THREADS), 0, (hipStream_t)stream, g, n, grad_scale,
                       partials);
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}

extern "C" int lfvdm_grad_norm_finalize(const float* partials, int nparts, float max_norm, float* stat, void* stream) {
    if (nparts < 1 || nparts > LFVDM_GRAD_NORM_MAX_PARTS || !(max_norm == max_norm)) return LFVDM_E_SHAPE;
    hipLaunchKernelGGL(grad_norm_finalize_kernel, dim3(1), dim3(GN_THREADS), 0, (hipStream_t)stream, partials, nparts, max_norm, stat);
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}

extern "C" int lfvdm_adamw_ema_clip(const lfvdm_adamw_args* a, const float* stat, void* stream) {
    if (a->n <= 0 || a->n_ema < 0 || a->n_ema > 4 || !stat) return LFVDM_E_SHAPE;
    const unsigned blocks = adamw_ema_blocks(a->n);
    switch (a->n_ema) {
        case 0: hipLaunchKernelGGL((adamw_ema_kernel<0, true>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, *a, ClipStat<true>{stat}); break;
        case 1: hipLaunchKernelGGL((adamw_ema_kernel<1, true>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, *a, ClipStat<true>{stat}); break;
        case 2: hipLaunchKernelGGL((adamw_ema_kernel<2, true>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, *a, ClipStat<true>{stat}); break;
        case 3: hipLaunchKernelGGL((adamw_ema_kernel<3, true>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, *a, ClipStat<true>{stat}); break;
        default: hipLaunchKernelGGL((adamw_ema_kernel<4, true>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, *a, ClipStat<true>{stat}); break;
    }
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}
