// Host side shared by the temporal-attention files (attention.hip, attention_bwd.hip, attention_temporal2.hip,
// attention_temporal_long.hip): the argument records, the cross-file entries, the frame limits.  Not part of the C ABI.
#pragma once
#include "common_hip.h"

constexpr int TEMPORAL_MAXT = 32;        // frames per window of the kernels that keep a frame's logits in registers
constexpr int TEMPORAL_MAXT_LONG = 64;   // ... of the frame-group kernels (attention_temporal_long.hip)

// One launch's operands: filled once by the exported entry, read by field name at every hipLaunchKernelGGL.
struct TemporalFwd {
    const float *qkv, *Rq, *Rk, *Rv, *mask;
    float *o, *attn_out;
    int B, T, P, C, heads;
    RSel rsel;
    hipStream_t s;
};
struct TemporalBwd {
    const float *qkv, *d_o, *Rq, *Rk, *Rv, *mask;
    float *ws_p, *ws_ds, *dqkv;     // P rows, dS rows, gradient of qkv (as in lfvdm_hip.h)
    int B, T, P, C, heads;
    hipStream_t s;
};

// LFVDM_E_UNSUPPORTED = shape not covered: the caller goes on to its next kernel.
int lfvdm_attn_temporal2_try(const TemporalFwd& a);            // attention_temporal2.hip: head dims 16 / 32 / 64, small launches
int lfvdm_attn_temporal2_bwd_rows_try(const TemporalBwd& a);   // attention_temporal2.hip: the backward's rows kernel only
int lfvdm_attn_temporal_long(const TemporalFwd& a);            // attention_temporal_long.hip: 33 to 64 frames
int lfvdm_attn_temporal_long_bwd(const TemporalBwd& a);        // attention_temporal_long.hip: rows + cols kernels, same shapes
