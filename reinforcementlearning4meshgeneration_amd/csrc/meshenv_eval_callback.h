// meshenv_eval_callback.h -- the two kernels that let SB3's EvalCallback (the reference's CustomCallback,
// rl/baselines/CustomizeCallback.py:241-310) decide on the device (include/meshenv_eval_callback.h):
// after a queued evaluation (meshenv_evaluate_queued: k_eval_begin, then policy, step and k_eval_tally per vector step) the
// records are reduced to one history row, compared with the best mean so far, and the live parameters are kept when the
// comparison says so -- the idiom of k_optim_step_gated's target_kl stop: the decision is a word in device memory that the
// next launch reads.
//
// k_eval_reduce.  ONE workgroup of 64 lanes.  Slot s of env e is recorded iff s - offset[e] < min(count[e], target[e]);
// everything else (envs with target 0, the slots of episodes that did not end in time) is a hole and is never read.
//   pass 1  lane l walks envs l, l + 64, ... in ascending order and each env's recorded slots in ascending order: the float64
//           sum of the returns from 0.0, and integer sums of the count, the lengths, the complete flags and the element
//           counts (over n_elem >= 0).  The 64 partial sums meet in an xor butterfly, p[l] += p[l ^ d], d = 32, 16, 8, 4, 2, 1:
//           both partners add the same two numbers, so every lane holds the same bits.
//   pass 2  the same walk and butterfly over (return - mean)^2 (-ffp-contract=off: a product, then a sum).
//   lane 0  mean = sum / recorded, std = sqrt(sum2 / recorded) (numpy's population std), the gate improved = recorded > 0 &&
//           mean > best_mean (strict; NaN never compares), the history row and the state.  A mean over nothing is written as
//           the quiet NaN 0x7FF8000000000000, not as 0.0 / 0.0, whose sign differs between machines.
// The order is restated in tests/eval_callback_ref.py and compared bit for bit.
//
// k_keep_best.  A multi-tensor copy gated by the `improved` word: grid (chunks, tensors), every workgroup reads the word
// once (thread 0, through LDS) and leaves when it is 0.  Per tensor: scalar copies up to the destination's first 16-byte
// boundary, float4 copies from there when the source is 16-byte aligned at that element, scalar copies otherwise and for the
// tail.  Plain C++ stores only.
#pragma once

#include "meshenv_eval.h"

namespace meshenv {

constexpr int kEvalRowDoubles = 9;     // num_timesteps mean std mean_len recorded short complete_rate mean_n_elem improved
constexpr int kEvalStateDoubles = 4;   // best_mean best_eval last_mean evaluations
constexpr int kKeepMaxEntries = 64;
constexpr int kKeepThreads = 256;
constexpr int kKeepMaxChunks = 64;     // workgroups per tensor at most: they stride over the rest

struct EvalReduceArgs {
    int n, total, row;
    double num_timesteps;
    const int32_t *target, *offset, *count;
    const double *ep_return;
    const int32_t *ep_length, *ep_flags, *ep_n_elem;
    const int32_t *short_envs;
    double *history;    // [capacity][kEvalRowDoubles]
    double *state;      // [kEvalStateDoubles]
    int32_t *improved;  // [1]
};

__device__ __forceinline__ double eval_butterfly(double v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ long long eval_butterfly(long long v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// the recorded slots of env e: [off, off + c), clipped to the buffers
__device__ __forceinline__ void eval_recorded(const EvalReduceArgs &A, int e, int *off, int *c)
{
    const int tgt = A.target[e], o = A.offset[e];
    int k = A.count[e];
    k = k < tgt ? k : tgt;
    if (o < 0 || o >= A.total) k = 0;
    else if (k > A.total - o) k = A.total - o;
    *off = o;
    *c = k;
}

__device__ __forceinline__ double eval_quiet_nan() { return __longlong_as_double(0x7FF8000000000000LL); }

__global__ void __launch_bounds__(64) k_eval_reduce(EvalReduceArgs A)
{
    const int lane = threadIdx.x;
    double s = 0.0;
    long long cnt = 0, len = 0, comp = 0, ne = 0, ne_cnt = 0;
    for (int e = lane; e < A.n; e += 64) {
        int off, c;
        eval_recorded(A, e, &off, &c);
        for (int k = 0; k < c; k++) {
            const int slot = off + k;
            s += A.ep_return[slot];
            cnt += 1;
            len += A.ep_length[slot];
            comp += A.ep_flags[slot] & 1;
            const int v = A.ep_n_elem[slot];
            if (v >= 0) {
                ne += v;
                ne_cnt += 1;
            }
        }
    }
    s = eval_butterfly(s);
    cnt = eval_butterfly(cnt);
    len = eval_butterfly(len);
    comp = eval_butterfly(comp);
    ne = eval_butterfly(ne);
    ne_cnt = eval_butterfly(ne_cnt);
    const double nan = eval_quiet_nan();
    const double mean = cnt > 0 ? s / (double)cnt : nan;
    double q = 0.0;
    if (cnt > 0) {
        for (int e = lane; e < A.n; e += 64) {
            int off, c;
            eval_recorded(A, e, &off, &c);
            for (int k = 0; k < c; k++) {
                const double d = A.ep_return[off + k] - mean;
                q += d * d;
            }
        }
    }
    q = eval_butterfly(q);
    if (lane != 0) return;
    const double best = A.state[0];
    const bool improved = cnt > 0 && mean > best;
    double *row = A.history + (size_t)A.row * kEvalRowDoubles;
    row[0] = A.num_timesteps;
    row[1] = mean;
    row[2] = cnt > 0 ? sqrt(q / (double)cnt) : nan;
    row[3] = cnt > 0 ? (double)len / (double)cnt : nan;
    row[4] = (double)cnt;
    row[5] = (double)A.short_envs[0];
    row[6] = cnt > 0 ? (double)comp / (double)cnt : nan;
    row[7] = ne_cnt > 0 ? (double)ne / (double)ne_cnt : nan;
    row[8] = improved ? 1.0 : 0.0;
    if (improved) {
        A.state[0] = mean;
        A.state[1] = (double)A.row;
    }
    A.state[2] = mean;
    A.state[3] = (double)(A.row + 1);
    A.improved[0] = improved ? 1 : 0;
}

struct KeepEntry {
    const float *src;
    long long dst_off, numel;
};

struct KeepTable {
    KeepEntry e[kKeepMaxEntries];
};

__global__ void __launch_bounds__(kKeepThreads) k_keep_best(float *dst, const int32_t *improved, KeepTable T)
{
    __shared__ int s_go;
    if (threadIdx.x == 0) s_go = improved[0];
    __syncthreads();
    if (s_go == 0) return;
    const KeepEntry E = T.e[blockIdx.y];
    const float *src = E.src;
    float *out = dst + E.dst_off;
    const long long n = E.numel;
    long long head = (long long)((4 - (((uintptr_t)out >> 2) & 3)) & 3);   // floats up to the destination's 16-byte boundary
    if (head > n) head = n;
    const bool vec = (((uintptr_t)(src + head)) & 15) == 0;
    const long long n_vec = vec ? (n - head) >> 2 : 0;
    const long long tail = head + 4 * n_vec;
    const long long tid = (long long)blockIdx.x * kKeepThreads + threadIdx.x, stride = (long long)gridDim.x * kKeepThreads;
    const float4 *src4 = reinterpret_cast<const float4 *>(src + head);
    float4 *out4 = reinterpret_cast<float4 *>(out + head);
    for (long long j = tid; j < n_vec; j += stride) out4[j] = src4[j];
    for (long long i = tid; i < head; i += stride) out[i] = src[i];
    for (long long i = tail + tid; i < n; i += stride) out[i] = src[i];
}

}  // namespace meshenv
