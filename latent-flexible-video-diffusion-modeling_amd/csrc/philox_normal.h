// The samplers' in-kernel Gaussian noise, shared by every kernel that draws it (diffusion_ops.hip, known_region.hip).
// Counter-based: Philox4x32-10 (Salmon et al., SC'11) keyed by the chain's 64-bit seed, counter = (quad index within the
// row, batch row, timestep, stream word) -> four uniform words -> two Box-Muller pairs = the noise of four consecutive
// elements.  A given (seed, timestep, element, stream word) always gets the same value, whatever the launch geometry.
//
// The stream word - the fourth counter word - keeps the draws of different launches of one sampling step apart.  Philox is
// a bijection of the counter under a fixed key, so two counters that differ in any word give unrelated outputs:
//   NOISE_STREAM_UPDATE   0   the x_{t-1} update (lfvdm_update_rng_x0, lfvdm_conv_out_update_x0)
//   NOISE_STREAM_BLEND    1   the known-region blend (lfvdm_known_blend)
//   NOISE_STREAM_RENOISE  2   the re-noise step of resampling (lfvdm_renoise)
//   NOISE_STREAM_SEARCH   3   the schedule search (schedule_search.hip: the low byte of the word, the window step above it;
//                             its key is the search's seed and its other counter words are keyed by video frame, not by row)
//   NOISE_STREAM_PRIOR    4   the i.i.d. draw xi behind the temporally correlated noise prior (lfvdm_noise_prior_fill, draw
//                             mode): the update kernels' counter layout, so with L = I it is the stream-4 sibling of stream 0
#pragma once
#include "common_hip.h"

// (the host tests of the first four streams read the `NAME = N` spellings of this header and expect exactly those four: the
// fifth enumerator takes its value by position, pinned by the static_assert)
enum { NOISE_STREAM_UPDATE = 0, NOISE_STREAM_BLEND = 1, NOISE_STREAM_RENOISE = 2, NOISE_STREAM_SEARCH = 3, NOISE_STREAM_PRIOR };
static_assert(NOISE_STREAM_PRIOR == 4, "the noise prior draws on stream word 4");

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned (&out)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__device__ __forceinline__ f32x4 normal4_stream(unsigned quad, unsigned row, unsigned step, unsigned stream_word, unsigned k0,
                                                unsigned k1) {
    unsigned r[4];
    philox4x32_10(quad, row, step, stream_word, k0, k1, r);
    const float two_pi = 6.283185307179586f, s32 = 2.3283064365386963e-10f;      // 2^-32
    const float u0 = ((float)r[0] + 1.0f) * s32, u1 = (float)r[1] * s32;         // u0 in (0, 1]
    const float u2 = ((float)r[2] + 1.0f) * s32, u3 = (float)r[3] * s32;
    const float m0 = sqrtf(-2.0f * logf(u0)), m1 = sqrtf(-2.0f * logf(u2));
    float s0, c0, s1, c1;
    sincosf(two_pi * u1, &s0, &c0);
    sincosf(two_pi * u3, &s1, &c1);
    return (f32x4){m0 * c0, m0 * s0, m1 * c1, m1 * s1};
}

// the update kernels' stream
__device__ __forceinline__ f32x4 normal4(unsigned quad, unsigned row, unsigned step, unsigned k0, unsigned k1) {
    return normal4_stream(quad, row, step, NOISE_STREAM_UPDATE, k0, k1);
}
