// Loss head of a weighted training step: the two masked MSEs of training_losses (gaussian_diffusion.py:787-788 under the
// latent mask and under the eval mask) and the timestep-weighted loss, one pass over target and pred, and the weighted
// loss's closed-form gradient.
//
//   mse[b]      = mean over (T, frame_inner) of (target - pred)^2 * mask[b, frame]        (NOT divided by the mask count)
//   eval_mse[b] = the same under eval_mask
//   loss[b]     = mse[b] * wtab[clamp(t[b], 0, n_t - 1)]                                   (one fp32 product of the final mse)
//   dpred       = -2 (target - pred) * mask[b, frame] * wtab[...] * g[b] / (T * frame_inner)
//
// The weight is gathered by t[b] HERE, on the device: TrainLoop replays the micro-step as a captured graph whose t lives
// in the graph's static input bytes and changes with every replay, so a weight looked up by the host at capture time would
// be stale from the second step on.  The index is clamped: no t reads outside the table.
//
// The forward kernel is masked_mse_kernel (diffusion_ops.hip) with a second accumulator: the same thread-to-element mapping
// (float4 sweep over the whole row when frame_inner % 4 == 0, else frame by frame with scalar loads), the same expression per
// element, the same wave_sum and the same index-order sum of the 16 wave partials by thread 0 - so mse and eval_mse are
// bitwise what lfvdm_masked_mse returns on the same inputs, and the logs of weighted and unweighted runs are comparable.
// No atomics anywhere: deterministic.
#include "common_hip.h"

namespace {

__device__ __forceinline__ float row_weight(const int64_t* __restrict__ t, const float* __restrict__ wtab, int n_t, int b) {
    int64_t tb = t[b];
    tb = tb < 0 ? 0 : (tb > (int64_t)n_t - 1 ? (int64_t)n_t - 1 : tb);
    return wtab[tb];
}

__global__ __launch_bounds__(1024) void train_loss_kernel(const float* __restrict__ a, const float* __restrict__ bb,
                                                          const float* __restrict__ mask, const float* __restrict__ eval_mask,
                                                          const int64_t* __restrict__ t, const float* __restrict__ wtab, int n_t,
                                                          float* __restrict__ mse, float* __restrict__ eval_mse,
                                                          float* __restrict__ loss, int T, int frame_inner) {
    const int b = blockIdx.x;
    const size_t base = (size_t)b * T * frame_inner;
    float acc = 0.f, acc_e = 0.f;
    if ((frame_inner & 3) == 0) {
        const int q = frame_inner >> 2, total = T * q;
        for (int e = threadIdx.x; e < total; e += 1024) {
            const int f = e / q;
            const float mk = mask ? mask[b * T + f] : 1.f;
            const float me = eval_mask ? eval_mask[b * T + f] : 1.f;
            const f32x4 d = ld4(a + base + (size_t)e * 4) - ld4(bb + base + (size_t)e * 4);
            acc += ((d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w)) * mk;
            acc_e += ((d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w)) * me;
        }
    } else {
        for (int f = 0; f < T; ++f) {
            const float mk = mask ? mask[b * T + f] : 1.f;
            const float me = eval_mask ? eval_mask[b * T + f] : 1.f;
            for (int i = threadIdx.x; i < frame_inner; i += 1024) {
                const float d = a[base + (size_t)f * frame_inner + i] - bb[base + (size_t)f * frame_inner + i];
                acc += d * d * mk;
                acc_e += d * d * me;
            }
        }
    }
    __shared__ float red[2][16];
    acc = wave_sum(acc);
    acc_e = wave_sum(acc_e);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = acc;
        red[1][threadIdx.x >> 6] = acc_e;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.f, se = 0.f;
        for (int w = 0; w < 16; ++w) s += red[0][w];
        for (int w = 0; w < 16; ++w) se += red[1][w];
        const float m = s / (float)((size_t)T * frame_inner);
        mse[b] = m;
        eval_mse[b] = se / (float)((size_t)T * frame_inner);
        loss[b] = m * row_weight(t, wtab, n_t, b);
    }
}

// every element of dpred is written; shape of masked_mse_bwd_kernel, with 16-byte accesses (vec) when frame_inner % 4 == 0
// and the three pointers allow it - element by element the same arithmetic either way
__global__ __launch_bounds__(256) void train_loss_bwd_kernel(const float* __restrict__ target, const float* __restrict__ pred,
                                                             const float* __restrict__ mask, const int64_t* __restrict__ t,
                                                             const float* __restrict__ wtab, int n_t, const float* __restrict__ g,
                                                             float* __restrict__ dpred, int T, int frame_inner, int vec) {
    const int b = blockIdx.y;
    const size_t base = (size_t)b * T * frame_inner;
    const long total = (long)T * frame_inner;
    const float sc = (-2.0f * g[b] / (float)((size_t)T * frame_inner)) * row_weight(t, wtab, n_t, b);
    if (vec) {
        const long total4 = total >> 2;
        const int q = frame_inner >> 2;
        for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total4; e += (long)gridDim.x * 256) {
            const float mk = mask ? mask[b * T + (int)(e / q)] : 1.f;
            const size_t at = base + (size_t)e * 4;
            st4(dpred + at, (ld4(target + at) - ld4(pred + at)) * (sc * mk));
        }
    } else {
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
            const float mk = mask ? mask[b * T + (int)(i / frame_inner)] : 1.f;
            dpred[base + i] = (target[base + i] - pred[base + i]) * (sc * mk);
        }
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int lfvdm_train_loss(const float* target, const float* pred, const float* mask, const float* eval_mask,
                                const int64_t* t, const float* wtab, int n_t, float* mse, float* eval_mse, float* loss, int B,
                                int T, int frame_inner, void* stream) {
    if (B <= 0 || T <= 0 || frame_inner <= 0 || n_t <= 0) return LFVDM_E_SHAPE;
    if (!target || !pred || !t || !wtab || !mse || !eval_mse || !loss) return LFVDM_E_SHAPE;
    // the 16-byte sweep is part of the summation order (that of lfvdm_masked_mse): refused, not replaced, on odd pointers
    if ((frame_inner & 3) == 0 && !(aligned16(target) && aligned16(pred))) return LFVDM_E_UNSUPPORTED;
    hipLaunchKernelGGL(train_loss_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, target, pred, mask, eval_mask, t, wtab, n_t,
                       mse, eval_mse, loss, T, frame_inner);
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}

extern "C" int lfvdm_train_loss_bwd(const float* target, const float* pred, const float* mask, const int64_t* t, const float* wtab,
                                    int n_t, const float* g, float* dpred, int B, int T, int frame_inner, void* stream) {
    if (B <= 0 || T <= 0 || frame_inner <= 0 || n_t <= 0) return LFVDM_E_SHAPE;
    if (!target || !pred || !t || !wtab || !g || !dpred) return LFVDM_E_SHAPE;
    const int vec = (frame_inner & 3) == 0 && aligned16(target) && aligned16(pred) && aligned16(dpred);
    long gx = ((long)T * frame_inner / (vec ? 4 : 1) + 255) / 256;
    if (gx > 1024) gx = 1024;
    if (gx < 1) gx = 1;
    hipLaunchKernelGGL(train_loss_bwd_kernel, dim3((unsigned)gx, B), dim3(256), 0, (hipStream_t)stream, target, pred, mask, t, wtab,
                       n_t, g, dpred, T, frame_inner, vec);
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}
