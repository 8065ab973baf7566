// Fused AdamW + EMA + gradient-norm over one flat fp32 parameter arena (HBM-bound, float4 streams).
// Replaces per-tensor `opt.step()` (torch AdamW), `update_ema` (nn.py:55-65: 2 launches per tensor and
// rate) and `_log_grad_norm` (train_util.py:353-357: one `.item()` host sync per parameter tensor) of the
// reference's optimize_normal (train_util.py:346-351) with a single launch and no host synchronisation.
// The kernel lives in adamw_ema_body.h (the clipping entry of grad_clip.hip launches its second instance).
#include "adamw_ema_body.h"

extern "C" int lfvdm_adamw_ema(const lfvdm_adamw_args* a, void* stream) {
    if (a->n <= 0 || a->n_ema < 0 || a->n_ema > 4) return LFVDM_E_SHAPE;
    const unsigned blocks = adamw_ema_blocks(a->n);
    switch (a->n_ema) {
        case 0: hipLaunchKernelGGL((adamw_ema_kernel<0, false>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, *a, ClipStat<false>{}); break;
        case 1: hipLaunchKernelGGL((adamw_ema_kernel<1, false>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, *a, ClipStat<false>{}); break;
        case 2: hipLaunchKernelGGL((adamw_ema_kernel<2, false>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, *a, ClipStat<false>{}); break;
        case 3: hipLaunchKernelGGL((adamw_ema_kernel<3, false>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, *a, ClipStat<false>{}); break;
        default: hipLaunchKernelGGL((adamw_ema_kernel<4, false>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, *a, ClipStat<false>{}); break;
    }
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}
