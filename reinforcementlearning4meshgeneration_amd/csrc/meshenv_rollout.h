// k_rollout_gather: the minibatches of SB3's RolloutBuffer.get for a whole epoch in one launch
// (include/meshenv_rollout.h).
//
// collect_rollout leaves six histories in [T][n] order (obs [T][n][18], buffer_actions [T][n][3], value, log_prob, advantages,
// returns [T][n]).  SB3's swap_and_flatten numbers their rows i = env * T + t, and one epoch visits them in the order of a
// permutation: minibatch k is rows perm[k B .. (k + 1) B).  The kernel writes ALL rows in permuted order into six field-major
// outputs, out_f[j] = f[perm[j] % T][perm[j] / T], so that every minibatch of the epoch is a contiguous slice of each output.
//
// The work is a copy of 25 floats per row.  The outputs are cut into chunks of kRgChunk = 1024 consecutive floats of ONE
// field, a workgroup of 256 threads per chunk: thread t writes floats t, t + 256, t + 512, t + 768 of the chunk, so a wave
// stores 64 consecutive floats and every output element is written by exactly one thread: no LDS, no atomics, and repeated
// launches give the same bits.  For the observations (and the actions) the chunk runs over the flattened (row, column) index,
// so a wave still stores 64 consecutive floats and reads pieces of 72-byte (12-byte) source rows.  V2 is the same copy of the
// observations in 8-byte pieces (a row is 9 of them); it needs both observation pointers 8-byte aligned.
//
// A perm[j] outside [0, rows) is never used as an address: the thread skips the read and writes NaN to row j of the field.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace meshenv {

constexpr int kRgChunk = 1024;      // output floats per workgroup: 256 threads x 4
constexpr int kRgThreads = 256;
constexpr int kRgObs = 18, kRgAct = 3, kRgScalars = 4;

struct RolloutGatherArgs {
    const float *obs, *act;             // [T][n][18], [T][n][3]
    const float *scalar[kRgScalars];    // value, log_prob, advantages, returns: [T][n]
    float *obs_out, *act_out;           // [rows][18], [rows][3]
    float *scalar_out[kRgScalars];      // [rows]
    const void *perm;                   // [rows] int32 or int64
    int32_t perm64;                     // 1: perm holds int64
    int32_t T, n, rows;                 // rows = T * n
    int32_t obs_blocks, act_blocks, scalar_blocks;   // workgroups per field: the grid is obs + act + 4 scalar
};

// The source row (t * n + env) of output row j, or -1 when perm[j] is not a row.
__device__ __forceinline__ int rg_source(const RolloutGatherArgs &A, int j)
{
    long long i = A.perm64 ? static_cast<const long long *>(A.perm)[j] : (long long)static_cast<const int32_t *>(A.perm)[j];
    if (i < 0 || i >= (long long)A.rows) return -1;
    const uint32_t u = (uint32_t)i, env = u / (uint32_t)A.T, t = u - env * (uint32_t)A.T;
    return (int)(t * (uint32_t)A.n + env);
}

// One chunk of a field of W floats per row, over the flattened (row, column) index.
template <int W>
__device__ __forceinline__ void rg_chunk(const RolloutGatherArgs &A, const float *__restrict__ src, float *__restrict__ dst, int chunk)
{
    const int total = A.rows * W;
    const int end = chunk * kRgChunk + kRgChunk < total ? chunk * kRgChunk + kRgChunk : total;
    for (int e = chunk * kRgChunk + (int)threadIdx.x; e < end; e += kRgThreads) {
        const int j = e / W, c = e - j * W;
        const int s = rg_source(A, j);
        dst[e] = s < 0 ? __builtin_nanf("") : src[s * W + c];
    }
}

// The observations in 8-byte pieces: 9 per row, 512 pieces (1024 floats) per chunk.
__device__ __forceinline__ void rg_chunk_obs2(const RolloutGatherArgs &A, int chunk)
{
    constexpr int P = kRgObs / 2;
    const int total = A.rows * P;
    const int first = chunk * (kRgChunk / 2);
    const int end = first + kRgChunk / 2 < total ? first + kRgChunk / 2 : total;
    const float2 *__restrict__ src = reinterpret_cast<const float2 *>(A.obs);
    float2 *__restrict__ dst = reinterpret_cast<float2 *>(A.obs_out);
    for (int e = first + (int)threadIdx.x; e < end; e += kRgThreads) {
        const int j = e / P, c = e - j * P;
        const int s = rg_source(A, j);
        float2 v;
        if (s < 0) v.x = v.y = __builtin_nanf("");
        else v = src[s * P + c];
        dst[e] = v;
    }
}

template <bool V2>
__global__ __launch_bounds__(kRgThreads) void k_rollout_gather(RolloutGatherArgs A)
{
    int b = (int)blockIdx.x;
    if (b < A.obs_blocks) {
        if (V2) rg_chunk_obs2(A, b);
        else rg_chunk<kRgObs>(A, A.obs, A.obs_out, b);
        return;
    }
    b -= A.obs_blocks;
    if (b < A.act_blocks) {
        rg_chunk<kRgAct>(A, A.act, A.act_out, b);
        return;
    }
    b -= A.act_blocks;
    const int f = b / A.scalar_blocks;      // < kRgScalars by the grid size
    // a chain of selects, not A.scalar[f]: a run-time index into a kernel argument would put the array into scratch
    const float *src = f == 0 ? A.scalar[0] : f == 1 ? A.scalar[1] : f == 2 ? A.scalar[2] : A.scalar[3];
    float *dst = f == 0 ? A.scalar_out[0] : f == 1 ? A.scalar_out[1] : f == 2 ? A.scalar_out[2] : A.scalar_out[3];
    rg_chunk<1>(A, src, dst, b - f * A.scalar_blocks);
}

}  // namespace meshenv
