// The small-M grouped linear ("row-dot") of every embedding projection, its backward (float atomics or a fixed summation
// order), and the SiLU those launches apply to their inputs as a launch of its own.  All HBM/L2-bound; wave = 64.
#include "common_hip.h"

namespace {

// -------------------------------------------------------------------------------------
// rowdot: one wave per output row o of a job; up to 8 input rows share each weight load.
// -------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rowdot_kernel(const lfvdm_rowdot_job* __restrict__ jobs, int njobs, int total_rows) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= total_rows) return;
    int j = 0;
    while (j + 1 < njobs && jobs[j + 1].row0 <= row) ++j;
    const lfvdm_rowdot_job J = jobs[j];
    const int o = row - J.row0;
    const float* wrow = J.W + (size_t)o * J.K;
    const float bo = J.b ? J.b[o] : 0.f;
    for (int m0 = 0; m0 < J.M; m0 += 8) {
        float acc[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = 0.f;
        for (int k = lane * 4; k < J.K; k += 256) {
            const f32x4 wv = ld4(wrow + k);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (m0 + i >= J.M) break;
                f32x4 v;
                if (J.in_mode == 2) {
                    // sinusoidal embedding [cos | sin]; frequency table appended after the timesteps
                    const float t = J.in[m0 + i];
                    const float* fr = J.in + J.ldin;  // freqs[K/2]
                    const int half = J.K >> 1;
                    float e[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int kk = k + u;
                        e[u] = kk < half ? cosf(t * fr[kk]) : sinf(t * fr[kk - half]);
                    }
                    v.x = e[0]; v.y = e[1]; v.z = e[2]; v.w = e[3];
                } else {
                    v = ld4(J.in + (size_t)(m0 + i) * J.ldin + k);
                    if (J.in_mode == 1) {
                        v.x = silu_full_f(v.x); v.y = silu_full_f(v.y); v.z = silu_full_f(v.z); v.w = silu_full_f(v.w);
                    }
                }
                acc[i] += v.x * wv.x + v.y * wv.y + v.z * wv.z + v.w * wv.w;
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (m0 + i >= J.M) break;
            const float s = wave_sum(acc[i]);
            if (lane == 0) J.out[(size_t)(m0 + i) * J.ldout + o] = s + bo;
        }
    }
}

// Backward of the grouped small-M linears: one wave per block of RDB_ROWS output rows of one job.
//   dW[o][k] += sum_m dout[m][o] * actin(in[m][k]);  db[o] += sum_m dout[m][o];
//   din[m][k] += sum_o dout[m][o] * W[o][k]        (gradient w.r.t. the ACTIVATED input; float atomics, may be NULL)
// Every W row is read once.  din is tiny (M x K) and EVERY wave of a job adds to it: done per wave that is ~1700 waves
// hammering the same 1024 addresses (measured 63 us per launch, most of it atomic contention).  So the four waves of a
// workgroup sum their din partials in LDS and issue ONE set of atomics: 31.8 us.  (More tasks per wave would cut the
// atomics further but leaves too few workgroups for the dW read-modify-write stream: 2 tasks 44 us, 4 tasks 79 us.
// Workgroups whose tasks span two jobs fall back to per-task atomics.)
constexpr int RDB_ROWS = 8;    // rows per wave and task: the dW read-modify-write chain of a wave is serial, so keep it short
constexpr int RDB_TPW = 4;     // tasks per wave: upper bound of the LFVDM_ROWDOT_TPW tuning aid; the launcher uses 1
constexpr int RDB_KIT = 4;     // K <= 1024 on the grouped path (256 floats per lane sweep)
__global__ __launch_bounds__(256) void rowdot_bwd_kernel(const lfvdm_rowdot_bwd_job* __restrict__ jobs, int njobs, int total_tasks,
                                                         int tpw, const DetSlab ds) {
    __shared__ f32x4 red[3][4][RDB_KIT][64];         // waves 1..3 -> wave 0: [wave - 1][m][k sweep][lane]
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int first = blockIdx.x * (4 * tpw);
    const int last = min(first + 4 * tpw, total_tasks) - 1;
    int jf = 0, jl = 0;
    while (jf + 1 < njobs && jobs[jf + 1].task0 <= first) ++jf;
    while (jl + 1 < njobs && jobs[jl + 1].task0 <= last) ++jl;
    const lfvdm_rowdot_bwd_job J0 = jobs[jf];
    // (deterministic mode: every wave task stores its din partial to ITS row of the zero-filled slab - no grouping)
    const bool grouped = jf == jl && J0.din != nullptr && J0.M <= 4 && J0.K <= 256 * RDB_KIT && !ds.slab;   // workgroup-uniform
    f32x4 accG[4][RDB_KIT];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int it = 0; it < RDB_KIT; ++it) accG[i][it] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int r = 0; r < tpw; ++r) {
        const int task = first + wave + 4 * r;
        if (task >= total_tasks) break;
        int j = jf;
        while (j + 1 < njobs && jobs[j + 1].task0 <= task) ++j;
        const lfvdm_rowdot_bwd_job J = jobs[j];
        const int o0 = (task - J.task0) * RDB_ROWS;
        const int o1 = min(o0 + RDB_ROWS, J.O);
        for (int m0 = 0; m0 < J.M; m0 += 4) {
            const int mc = min(4, J.M - m0);
            int it = 0;
            for (int k = lane * 4; k < J.K; k += 256, ++it) {
                f32x4 inv[4], accD[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    accD[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
                    inv[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
                    if (i < mc) {
                        if (J.in_mode == 2) {
                            const float t = J.in[m0 + i];
                            const float* fr = J.in + J.ldin;
                            const int half = J.K >> 1;
#pragma unroll
                            for (int u = 0; u < 4; ++u) {
                                const int kk = k + u;
                                inv[i][u] = kk < half ? cosf(t * fr[kk]) : sinf(t * fr[kk - half]);
                            }
                        } else {
                            f32x4 v = ld4(J.in + (size_t)(m0 + i) * J.ldin + k);
                            if (J.in_mode == 1) {
                                v.x = silu_full_f(v.x); v.y = silu_full_f(v.y); v.z = silu_full_f(v.z); v.w = silu_full_f(v.w);
                            }
                            inv[i] = v;
                        }
                    }
                }
                // the task's RDB_ROWS output rows: weight rows, gradient rows and dout values are all requested before the
                // first use (one row per trip was a chain of dependent round trips: 32 us per launch)
                f32x4 wv[RDB_ROWS], gv[RDB_ROWS];
                float dv[RDB_ROWS][4];
#pragma unroll
                for (int u = 0; u < RDB_ROWS; ++u) {
                    const int o = min(o0 + u, o1 - 1);
                    wv[u] = ld4(J.W + (size_t)o * J.K + k);
                    gv[u] = ld4(J.dW + (size_t)o * J.K + k);
#pragma unroll
                    for (int i = 0; i < 4; ++i) dv[u][i] = i < mc ? J.dout[(size_t)(m0 + i) * J.lddout + o] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < RDB_ROWS; ++u) {
                    if (o0 + u < o1) {
                        f32x4 g = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            if (i < mc) {
                                g += inv[i] * dv[u][i];
                                accD[i] += wv[u] * dv[u][i];
                            }
                        }
                        st4(J.dW + (size_t)(o0 + u) * J.K + k, gv[u] + g);
                    }
                }
                if (grouped) {                       // (M <= 4: a single m0 pass; `it` < RDB_KIT)
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int q = 0; q < RDB_KIT; ++q)
                            if (q == it) accG[i][q] += accD[i];
                } else if (J.din) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        if (i < mc) {
                            float* dst = J.din + (size_t)(m0 + i) * J.lddin + k;
                            det_add(ds, task, dst + 0, accD[i].x); det_add(ds, task, dst + 1, accD[i].y);
                            det_add(ds, task, dst + 2, accD[i].z); det_add(ds, task, dst + 3, accD[i].w);
                        }
                    }
                }
            }
        }
        if (J.db && lane < o1 - o0) {
            float t = 0.f;
            for (int m = 0; m < J.M; ++m) t += J.dout[(size_t)m * J.lddout + o0 + lane];
            J.db[o0 + lane] += t;
        }
    }
    if (!grouped) return;                            // workgroup-uniform: no barrier is skipped by part of the workgroup
    if (wave > 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int q = 0; q < RDB_KIT; ++q) red[wave - 1][i][q][lane] = accG[i][q];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int q = 0; q < RDB_KIT; ++q) {
            const int k = lane * 4 + 256 * q;
            if (k < J0.K) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (i < J0.M) {
                        const f32x4 t = accG[i][q] + red[0][i][q][lane] + red[1][i][q][lane] + red[2][i][q][lane];
                        float* dst = J0.din + (size_t)i * J0.lddin + k;
                        atomicAdd(dst + 0, t.x); atomicAdd(dst + 1, t.y);
                        atomicAdd(dst + 2, t.z); atomicAdd(dst + 3, t.w);
                    }
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void silu_kernel(const float* __restrict__ in, float* __restrict__ out, long n4) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        f32x4 v = ld4(in + 4 * i);
        v.x = silu_full_f(v.x); v.y = silu_full_f(v.y); v.z = silu_full_f(v.z); v.w = silu_full_f(v.w);
        st4(out + 4 * i, v);
    }
}

}  // namespace

extern "C" int lfvdm_rowdot(const lfvdm_rowdot_job* jobs_dev, int njobs, int total_rows, void* stream) {
    if (njobs <= 0 || total_rows <= 0) return LFVDM_E_SHAPE;
    hipLaunchKernelGGL(rowdot_kernel, dim3((total_rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, jobs_dev, njobs,
                       total_rows);
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}

extern "C" int lfvdm_rowdot_bwd(const lfvdm_rowdot_bwd_job* jobs_dev, int njobs, int total_tasks, void* stream) {
    if (!jobs_dev || njobs <= 0 || total_tasks <= 0) return LFVDM_E_SHAPE;
    static const int tpw_env = getenv("LFVDM_ROWDOT_TPW") ? atoi(getenv("LFVDM_ROWDOT_TPW")) : 0;     // tuning aid
    const int tpw = tpw_env >= 1 && tpw_env <= RDB_TPW ? tpw_env : 1;
    const DetSlab none = {nullptr, nullptr, 0};
    hipLaunchKernelGGL(rowdot_bwd_kernel, dim3((total_tasks + 4 * tpw - 1) / (4 * tpw)), dim3(256), 0, (hipStream_t)stream,
                       jobs_dev, njobs, total_tasks, tpw, none);
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}

// Deterministic form: din_base / din_n = the array that holds every job's `din` rows (all jobs of the launch accumulate
// into it); det_ws holds total_tasks rows of din_n floats.  Zero-fill, partial stores, ordered sum.
extern "C" int lfvdm_rowdot_bwd_det(const lfvdm_rowdot_bwd_job* jobs_dev, int njobs, int total_tasks, float* din_base,
                                    int64_t din_n, float* det_ws, int64_t det_ws_floats, void* stream) {
    if (!jobs_dev || njobs <= 0 || total_tasks <= 0) return LFVDM_E_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    DetSlab ds = {nullptr, nullptr, 0};
    if (din_base) {
        if (!det_ws || din_n <= 0 || (int64_t)total_tasks * din_n > det_ws_floats) return LFVDM_E_SHAPE;
        if (hipMemsetAsync(det_ws, 0, (size_t)total_tasks * din_n * sizeof(float), s) != hipSuccess) return LFVDM_E_LAUNCH;
        ds = {det_ws, din_base, (long)din_n};
    }
    hipLaunchKernelGGL(rowdot_bwd_kernel, dim3((total_tasks + 3) / 4), dim3(256), 0, s, jobs_dev, njobs, total_tasks, 1, ds);
    LFVDM_CHECK_LAUNCH();
    if (din_base) return lfvdm_det_reduce_launch(din_base, det_ws, (long)din_n, total_tasks, s);
    return LFVDM_OK;
}

// out = x * sigmoid(x), the very silu_full_f the row-dot launches apply to their inputs in in_mode 1: materialising it once
// lets a launch with MANY batch rows (the sampler's per-chain tables) run in in_mode 0 instead of re-evaluating it per
// output row.  n must be a multiple of 4.
extern "C" int lfvdm_silu(const float* in, float* out, int64_t n, void* stream) {
    if (!in || !out || n <= 0 || (n & 3)) return LFVDM_E_SHAPE;
    long blocks = (n / 4 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(silu_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, in, out, (long)(n / 4));
    LFVDM_CHECK_LAUNCH();
    return LFVDM_OK;
}
