// Search for optimised conditioning frames (improved_diffusion/optimal_schedule.py): one pass scores G candidate
// conditioning sets on V videos as a batch of W = G * V windows of K frame slots, window w showing video w % V.  A
// conditioning set reaches the device only as the int32 slot table [W][K] - the video frame a slot shows, -1 for a padding
// slot - and the role table [W][K] (LFVDM_SLOT_PAD / _OBS / _LATENT).  Three launches around the replayed U-Net step:
//
//   lfvdm_search_assemble      once per pass: gather the windows from the resident video pool into the plan's x0 and the
//                              evaluator's x_start, write the masks and the int64 frame indices.  HBM-bound gather shaped like
//                              prepare_batch_kernel: one workgroup per (slot, window), 16-byte accesses.
//   lfvdm_search_noise_qsample inside the replayed step: timestep position j <- ctl[0], t = t_list[j] handed to the plan's
//                              clock as t + 1 (the clock pre-decrements), the slot's noise and x_t = sa[t] x_start + sb[t] noise.
//                              The LAST workgroup to finish advances ctl[0]: every workgroup has read it by then (the ticket
//                              ctl[1] is an integer atomic; nothing else is exchanged inside the launch).  Everything that
//                              changes between replays - position, list length ctl[2], seed and window step key[0..1] - is
//                              read from device memory: one captured graph serves every pass of a search.
//   lfvdm_search_scores        once per pass, behind the n_t replays: scores[g] = mean over (video, position) of the terms
//                              lfvdm_vb_terms wrote, added in double in a fixed order by one thread per candidate.
//
// Noise keying.  normal4_stream of philox_normal.h under key = the search's 64-bit seed and the counter
//   (quad within the frame, video frame index, position j << 16 | video, window step s << 8 | NOISE_STREAM_SEARCH):
// a function of (seed, s, j, video, video frame, element) alone - not of the slot a frame sits in, nor of the window that
// holds it - so every candidate of every round of a window step sees its latent frames under the same noise.
#include "common_hip.h"
#include "philox_normal.h"

namespace {

constexpr int MAX_WINDOWS = 65535;        // W rides in gridDim.y
constexpr int MAX_POSITIONS = 65535;      // j and the video share a counter word, 16 bits each
constexpr int MAX_STEP = (1 << 24) - 1;   // the window step shares a counter word with the stream id

__global__ __launch_bounds__(256) void assemble_kernel(const float* __restrict__ pool, const int32_t* __restrict__ table,
                                                       const int32_t* __restrict__ role, float* __restrict__ x0,
                                                       float* __restrict__ x_start, float* __restrict__ obs_mask,
                                                       float* __restrict__ latent_mask, float* __restrict__ mask,
                                                       int64_t* __restrict__ frame_indices, int K, int V, int Tv,
                                                       int frame_elems) {
    const int k = blockIdx.x, w = blockIdx.y;
    const size_t at = (size_t)w * K + k;
    const int frame = table[at];
    // a frame index outside the pool is treated as padding: a corrupt table must not read outside the pool
    const bool pad = frame < 0 || frame >= Tv;
    const int r = pad ? LFVDM_SLOT_PAD : role[at];
    const float* src = pool + ((size_t)(w % V) * Tv + (pad ? 0 : frame)) * frame_elems;
    float* d0 = x0 + at * frame_elems;
    float* d1 = x_start + at * frame_elems;
    const int n4 = frame_elems >> 2;
    for (int i = threadIdx.x; i < n4; i += 256) {
        const f32x4 v = pad ? (f32x4){0.f, 0.f, 0.f, 0.f} : ld4(src + 4 * i);
        st4(d0 + 4 * i, v);
        st4(d1 + 4 * i, v);
    }
    if (threadIdx.x == 0) {
        const float o = r == LFVDM_SLOT_OBS ? 1.f : 0.f, l = r == LFVDM_SLOT_LATENT ? 1.f : 0.f;
        obs_mask[at] = o;
        latent_mask[at] = l;
        mask[at] = (o + l) > 0.f ? 1.f : 0.f;
        frame_indices[at] = pad ? 0 : (int64_t)frame;
    }
}

// x_start == nullptr: the noise alone (the eager backend's fill).  ctl == nullptr: position, seed and window step are the
// arguments j_arg / seed_arg / step_arg; else they are ctl[0] (clamped into [0, ctl[2])) and key[0], key[1].
__global__ __launch_bounds__(256) void noise_qsample_kernel(const float* __restrict__ x_start, const int32_t* __restrict__ table,
                                                            const int64_t* __restrict__ t_list, int32_t* ctl,
                                                            const int64_t* __restrict__ key, int j_arg,
                                                            unsigned long long seed_arg, int step_arg,
                                                            const float* __restrict__ sa, const float* __restrict__ sb,
                                                            float* __restrict__ noise, float* __restrict__ x_t, int64_t* t_buf,
                                                            int K, int V, int frame_elems) {
    const int k = blockIdx.x, w = blockIdx.y;
    // (plain loads: ctl[0] is written by the previous launch's last workgroup, never inside this launch before every
    // workgroup has passed this line - see the ticket below)
    int j = j_arg;
    if (ctl) {
        const int n_t = ctl[2];
        j = ctl[0];
        j = j >= n_t ? n_t - 1 : j;
        j = j < 0 ? 0 : j;
    }
    const unsigned long long seed = ctl ? (unsigned long long)key[0] : seed_arg;
    const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
    const unsigned step_word = (((unsigned)(ctl ? (int)key[1] : step_arg) & 0xFFFFFFu) << 8) | NOISE_STREAM_SEARCH;
    const size_t at = (size_t)w * K + k;
    const int frame = table[at];
    const size_t base = at * frame_elems;
    const int n4 = frame_elems >> 2;
    if (x_start) {
        const int64_t t = t_list[j];
        const float ca = sa[t], cb = sb[t];
        if (k == 0 && threadIdx.x == 0) t_buf[w] = t + 1;          // the plan's clock pre-decrements
        for (int q = threadIdx.x; q < n4; q += 256) {
            const f32x4 z = frame < 0 ? (f32x4){0.f, 0.f, 0.f, 0.f}
                                      : normal4_stream((unsigned)q, (unsigned)frame, ((unsigned)j << 16) | (unsigned)(w % V),
                                                       step_word, k0, k1);
            st4(noise + base + 4 * q, z);
            st4(x_t + base + 4 * q, ca * ld4(x_start + base + 4 * q) + cb * z);
        }
    } else {
        for (int q = threadIdx.x; q < n4; q += 256) {
            const f32x4 z = frame < 0 ? (f32x4){0.f, 0.f, 0.f, 0.f}
                                      : normal4_stream((unsigned)q, (unsigned)frame, ((unsigned)j << 16) | (unsigned)(w % V),
                                                       step_word, k0, k1);
            st4(noise + base + 4 * q, z);
        }
    }
    if (ctl) {
        __syncthreads();
        if (threadIdx.x == 0) {
            const int total = (int)(gridDim.x * gridDim.y);
            if (atomicAdd(&ctl[1], 1) == total - 1) {        // every workgroup has read ctl[0]
                atomicExch(&ctl[1], 0);
                ctl[0] = j + 1;
            }
        }
    }
}

__global__ void scores_kernel(const float* __restrict__ terms, const int64_t* __restrict__ t_list, float* __restrict__ scores,
                              int G, int V, int n_t, int ld, int col_base) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    double acc = 0.0;
    for (int v = 0; v < V; ++v) {
        const float* row = terms + (size_t)(g * V + v) * ld;
        for (int j = 0; j < n_t; ++j) {
            const long col = col_base >= 0 ? (long)col_base - (long)t_list[j] : (long)j;
            if (col >= 0 && col < ld) acc += (double)row[col];
        }
    }
    scores[g] = (float)(acc / ((double)V * (double)n_t));
}

bool noise_args_ok(const int32_t* table, float* noise, int W, int K, int V, int frame_elems, int step) {
    if (!table || !noise || W <= 0 || W > MAX_WINDOWS || K <= 0 || V <= 0 || V > MAX_POSITIONS) return false;
    if (frame_elems <= 0 || (frame_elems & 3) || step < 0 || step > MAX_STEP) return false;
    return !(reinterpret_cast<uintptr_t>(noise) & 15);
}

}  // namespace

extern "C" int lfvdm_search_assemble(const float* pool, const int32_t* table, const int32_t* role, float* x0, float* x_start,
                                     float* obs_mask, float* latent_mask, float* mask, int64_t* frame_indices, int W, int K,
                                     int V, int Tv, int frame_elems, void* stream) {
    if (!pool || !table || !role || !x0 || !x_start || !obs_mask || !latent_mask || !mask || !frame_indices) return LFVDM_E_SHAPE;
    if (W <= 0 || W > MAX_WINDOWS || K <= 0 || V <= 0 || Tv <= 0 || frame_elems <= 0 || (frame_elems & 3)) return LFVDM_E_SHAPE;
    if ((reinterpret_cast<uintptr_t>(pool) | reinterpret_cast<uintptr_t>(x0) | reinterpret_cast<uintptr_t>(x_start)) & 15)
        return LFVDM_E_SHAPE;
    hipLaunchKernelGGL(assemble_kernel, dim3(K, W), dim3(256), 0, (hipStream_t)stream, pool, table, role, x0, x_start, obs_mask,
                       latent_mask, mask, frame_indices, K, V, Tv, frame_elems);
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}

extern "C" int lfvdm_search_noise_qsample(const float* x_start, const int32_t* table, const int64_t* t_list, int32_t* ctl,
                                          const int64_t* key, const float* sqrt_acp, const float* sqrt_1macp, float* noise,
                                          float* x_t, int64_t* t_buf, int W, int K, int V, int frame_elems, void* stream) {
    if (!x_start || !t_list || !ctl || !key || !sqrt_acp || !sqrt_1macp || !x_t || !t_buf) return LFVDM_E_SHAPE;
    if (!noise_args_ok(table, noise, W, K, V, frame_elems, 0)) return LFVDM_E_SHAPE;
    if ((reinterpret_cast<uintptr_t>(x_start) | reinterpret_cast<uintptr_t>(x_t)) & 15) return LFVDM_E_SHAPE;
    hipLaunchKernelGGL(noise_qsample_kernel, dim3(K, W), dim3(256), 0, (hipStream_t)stream, x_start, table, t_list, ctl, key, 0,
                       0ull, 0, sqrt_acp, sqrt_1macp, noise, x_t, t_buf, K, V, frame_elems);
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}

extern "C" int lfvdm_search_noise_fill(const int32_t* table, uint64_t seed, int step, int j, float* noise, int W, int K, int V,
                                       int frame_elems, void* stream) {
    if (j < 0 || j >= MAX_POSITIONS || !noise_args_ok(table, noise, W, K, V, frame_elems, step)) return LFVDM_E_SHAPE;
    hipLaunchKernelGGL(noise_qsample_kernel, dim3(K, W), dim3(256), 0, (hipStream_t)stream, (const float*)nullptr, table,
                       (const int64_t*)nullptr, (int32_t*)nullptr, (const int64_t*)nullptr, j, (unsigned long long)seed, step,
                       (const float*)nullptr, (const float*)nullptr, noise, (float*)nullptr, (int64_t*)nullptr, K, V,
                       frame_elems);
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}

extern "C" int lfvdm_search_scores(const float* terms, const int64_t* t_list, float* scores, int G, int V, int n_t, int ld,
                                   int col_base, void* stream) {
    if (!terms || !scores || G <= 0 || V <= 0 || n_t <= 0 || ld <= 0) return LFVDM_E_SHAPE;
    if (col_base >= 0 ? !t_list : ld < n_t) return LFVDM_E_SHAPE;
    hipLaunchKernelGGL(scores_kernel, dim3((G + 63) / 64), dim3(64), 0, (hipStream_t)stream, terms, t_list, scores, G, V, n_t, ld,
                       col_base);
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}
