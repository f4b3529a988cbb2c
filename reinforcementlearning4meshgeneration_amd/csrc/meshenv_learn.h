// meshenv_learn.h -- the two kernels of the off-policy learn loop that are not a network (include/meshenv_offpolicy_learn.h,
// DESIGN.md section 24): SB3's OffPolicyAlgorithm._sample_action before learning_starts, and the Monitor's episode
// returns / lengths, both on the device so that collect -> store -> train -> refresh never waits for the host.
//
// k_uniform_actions.  One launch fills actions[T][n][3] (the Box) and buffer_actions[T][n][3] ([-1, 1)) of T vector steps:
//     unscaled = action_space.sample();  buffer_action = policy.scale_action(unscaled);  action = unscale(buffer_action)
// with the draw made in the scaled space.  Element (t, env, c): Philox4x32-10 keyed by seed at counter words (env,
// lo(counter + t), hi(counter + t), 4), the 64-bit sum carrying into the high word; component c takes output word c;
// u = (float)(word >> 8) * 2^-24 is exact and in [0, 1) (NOT philox_normal's + 0.5f map, which can round to 1);
// buffer = 2 u - 1 is exact; action = unscale_action(buffer, low, high), the expression of k_policy_forward.  Tag 4 is this
// kernel's own: 0 the rollout noise, 1 the replay draw, 2 the TD target's noise, 3 the actor gradient's.
//
// k_episode_stats.  The Monitor of T vector steps of n envs from the reward [T][n] float64, done and complete [T][n]
// histories, in ONE workgroup of 1024 threads:
//   phase 1  thread e, e + 1024, ... scans its env's column in step order: ret += reward[t][e] (the sequential float64 sum
//            from 0.0 that Python's sum(rewards) makes), len += 1; at a done it notes (ret, len) at the flat index t * n + e
//            of the workspace and resets the carry.  The carries persist across calls.
//   phase 2  the finished episodes go into the ring in SB3's order, flat index ascending: rank = the exclusive prefix sum of
//            the done flags (per trip of 1024 flags: ballot + popcount inside a wave, the 16 wave totals through LDS),
//            slot = (count + rank) % W.  Only the last W of a call are written, so every slot has one writer; the count
//            advances by all of them.
// No atomics, no cross-workgroup traffic: the order of every sum is fixed by the code.
#pragma once

#include "meshenv_actor.h"

namespace meshenv {

constexpr uint32_t kUniformPhiloxTag = 4u;

struct UniformArgs {
    int T, n;
    uint64_t seed, counter;
    float low[3], high[3];
    float *actions, *buffer_actions;   // [T][n][3]
};

__global__ void __launch_bounds__(256)
k_uniform_actions(UniformArgs A)
{
    const long long total = (long long)A.T * A.n, stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const int t = (int)(i / A.n), env = (int)(i - (long long)t * A.n);
        const uint64_t c = A.counter + (uint64_t)t;
        uint32_t r[4];
        philox4x32((uint32_t)env, (uint32_t)c, (uint32_t)(c >> 32), kUniformPhiloxTag, (uint32_t)A.seed, (uint32_t)(A.seed >> 32), r);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float u = (float)(r[k] >> 8) * (1.0f / 16777216.0f);
            const float b = 2.0f * u - 1.0f;
            A.buffer_actions[i * 3 + k] = b;
            A.actions[i * 3 + k] = unscale_action(b, A.low[k], A.high[k]);
        }
    }
}

constexpr int kEpThreads = 1024;

struct EpisodeArgs {
    int T, n, W;
    const double *reward;              // [T][n]
    const uint8_t *done, *complete;    // [T][n]
    double *carry_return;              // [n]
    int *carry_len;                    // [n]
    double *ring;                      // [W][3]: return, length, complete
    unsigned long long *count;         // episodes finished so far
    double *work_return;               // [T * n] workspace, written where done
    int *work_len;                     // [T * n]
};

__global__ void __launch_bounds__(kEpThreads)
k_episode_stats(EpisodeArgs A)
{
    __shared__ unsigned int wave_sum[kEpThreads / 64];
    __shared__ unsigned int trip_total;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long total = (long long)A.T * A.n;
    const unsigned long long count0 = *A.count;
    // phase 1: the columns
    unsigned int mine = 0;
    for (int e = tid; e < A.n; e += kEpThreads) {
        double ret = A.carry_return[e];
        int len = A.carry_len[e];
        for (int t = 0; t < A.T; t++) {
            const long long i = (long long)t * A.n + e;
            ret += A.reward[i];
            len += 1;
            if (A.done[i]) {
                A.work_return[i] = ret;
                A.work_len[i] = len;
                ret = 0.0;
                len = 0;
                mine += 1;
            }
        }
        A.carry_return[e] = ret;
        A.carry_len[e] = len;
    }
    // the number of episodes of this call: lanes, then waves, in index order (integers: any order gives the same)
    unsigned int s = mine;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
    if (lane == 0) wave_sum[wave] = s;
    __syncthreads();
    if (tid == 0) {
        unsigned int all = 0;
        for (int w = 0; w < kEpThreads / 64; w++) all += wave_sum[w];
        trip_total = all;
    }
    __syncthreads();   // (also: the workspace writes of phase 1 are visible to the workgroup)
    const unsigned long long n_done = trip_total;
    const unsigned long long first_kept = n_done > (unsigned long long)A.W ? n_done - (unsigned long long)A.W : 0ull;
    // phase 2: ranks in flat order, one trip of 1024 flags at a time
    unsigned long long before = 0;
    for (long long base = 0; base < total; base += kEpThreads) {
        const long long i = base + tid;
        const bool flag = i < total && A.done[i] != 0;
        const unsigned long long ballot = __ballot(flag);
        const unsigned int in_wave = (unsigned int)__popcll(ballot & ((1ull << lane) - 1ull));
        __syncthreads();   // the previous trip's readers of wave_sum are through
        if (lane == 0) wave_sum[wave] = (unsigned int)__popcll(ballot);
        __syncthreads();
        unsigned int ahead = 0, all = 0;
        for (int w = 0; w < kEpThreads / 64; w++) {
            const unsigned int v = wave_sum[w];
            if (w < wave) ahead += v;
            all += v;
        }
        const unsigned long long rank = before + ahead + in_wave;
        if (flag && rank >= first_kept) {
            double *slot = A.ring + 3 * ((count0 + rank) % (unsigned long long)A.W);
            slot[0] = A.work_return[i];
            slot[1] = (double)A.work_len[i];
            slot[2] = A.complete[i] ? 1.0 : 0.0;
        }
        before += all;
    }
    if (tid == 0) *A.count = count0 + n_done;
}

}  // namespace meshenv
