// meshenv_replay.h -- the replay buffer of the off-policy algorithms (SAC, TD3) on the device: SB3 2.x's
// ReplayBuffer.add as OffPolicyAlgorithm._store_transition feeds it, and ReplayBuffer.sample / _get_samples
// (optimize_memory_usage=False).  Host restatement: tests/replay_ref.py.  Nothing here does arithmetic on a stored value
// except the three that SB3 does: rewards = (float)reward, the optional SAC action scaling
// 2.0f * ((a - low) / (high - low)) - 1.0f (float32, one rounding per operation: the build has -ffp-contract=off), and
// dones * (1 - timeouts) on the way out.  Everything else is copied bit for bit (NaN payloads, infinities, subnormals).
//
// Storage.  One caller-owned float32 array [rows][n_envs][kReplayR], one packed record per transition:
//
//   float  0..17  observation          (what the action was chosen on)
//         18..35  next observation     (the terminal observation where done, else the observation after the step)
//         36..38  action
//         39      reward               (float)reward
//         40      done                 0 / 1
//         41      timeout              done && !complete (TimeLimit.truncated), 0 when timeouts are not handled
//         42..    zero padding up to kReplayR
//
// SB3 keeps six arrays [rows, n, .]; a sampled transition is then six scattered reads of 4 to 72 bytes, and lanes that read
// from different rows run far below the rate of contiguous 128-byte segments.  A packed record is one aligned piece of
// kReplayR * 4 bytes read by kReplayR / 4 adjacent lanes with one 16-byte load each.  kReplayR is a compile-time constant:
// 48 (192-byte records, 42 payload floats + 6 of padding) is the default; -DMESHENV_REPLAY_R=64 builds the variant whose
// records are two aligned 128-byte lines.  On MI355X k_replay_add runs about 15 % faster with 48 (a quarter fewer bytes
// written), k_replay_sample shows no difference beyond run-to-run noise, and the store is a quarter smaller (numbers in
// DESIGN.md section 13).
// Offsets are size_t: rows * n_envs * kReplayR * 4 nears 2^32 at SB3's default buffer size and passes it beyond.
//
// Index draw.  Sample i of a batch at (seed, counter): w = philox4x32 (meshenv_actor.h) with counter words
// (i, counter lo, counter hi, kReplayDrawTag) and key (seed lo, seed hi);
//   row = __umulhi(w[0], size)      env = __umulhi(w[1], n_envs)
// i.e. the high half of the 64-bit product, which lies in [0, bound) and hits every index floor or ceil of 2^32 / bound
// times.  kReplayDrawTag = 1: the exploration noise (philox_normal) draws with 0 in that word, so a seed shared between the
// two never yields the same words.  Sample i depends on (seed, counter, i) alone, not on the batch size.
#pragma once

namespace meshenv {

#ifndef MESHENV_REPLAY_R
#define MESHENV_REPLAY_R 48
#endif

constexpr int kReplayR = MESHENV_REPLAY_R;          // floats per record
constexpr int kReplayPayload = 42;
constexpr int kRepNext = 18, kRepAct = 36, kRepReward = 39, kRepDone = 40, kRepTimeout = 41;
static_assert(kReplayR % 4 == 0 && kReplayR >= 44 && kReplayR <= 64, "a record is whole 16-byte pieces holding 42 floats");
constexpr int kReplayLanes = kReplayR / 4;          // adjacent lanes per record, one float4 each
constexpr int kReplayGroups = 16;                   // records a workgroup handles per pass
constexpr int kReplayThreads = kReplayLanes * kReplayGroups;   // 192 (R = 48) or 256 (R = 64)
constexpr uint32_t kReplayDrawTag = 1u;

struct ReplayAddArgs {
    int n, rows, T;
    int t0;                       // first step written: max(T - rows, 0), what T sequential adds leave
    int row0;                     // (pos + t0) % rows
    int scale, handle_timeouts;
    float lo0, lo1, lo2, hi0, hi1, hi2;
    const float *obs0;            // [n][18]
    const float *obs_after;       // [T][n][18]
    const float *tobs;            // [T][n][18]
    const float *actions;         // [T][n][3]
    const double *reward;         // [T][n]
    const uint8_t *done, *complete;
    float *store;                 // [rows][n][kReplayR]
};

// One record per group of kReplayLanes adjacent lanes; lane c builds floats 4c .. 4c + 3 and writes them with one 16-byte
// store, so a wave's stores cover whole records of neighbouring environments: contiguous in the store.  The loads are
// adjacent floats of the [n][18] / [n][3] inputs across a group and adjacent environments across groups.  A workgroup owns
// kReplayGroups environments (blockIdx.x) and the steps t0 + blockIdx.y, + gridDim.y, ...; t - t0 < rows, so no two
// (t, env) pairs of a launch share a record.
__global__ __launch_bounds__(kReplayThreads) void k_replay_add(ReplayAddArgs a)
{
    const int g = (int)threadIdx.x / kReplayLanes, c = (int)threadIdx.x % kReplayLanes;
    const int e = (int)blockIdx.x * kReplayGroups + g;
    if (e >= a.n) return;
    const size_t n = (size_t)a.n;
    for (int t = a.t0 + (int)blockIdx.y; t < a.T; t += (int)gridDim.y) {
        const size_t te = (size_t)t * n + (size_t)e;
        const bool d = a.done[te] != 0;
        const float *before = t == 0 ? a.obs0 + (size_t)e * kObsDim : a.obs_after + (te - n) * kObsDim;
        const float *next = (d ? a.tobs : a.obs_after) + te * kObsDim;
        const float *act = a.actions + te * 3;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int f = 4 * c + j;
            const float *src = f < kRepNext ? before + f : f < kRepAct ? next + (f - kRepNext) : act + (f - kRepAct);
            float x = f < kRepReward ? *src : 0.0f;
            if (a.scale) {
                const int k = f - kRepAct;     // 0..2 on an action float
                const bool is_act = k >= 0 && k < 3;
                const float lo = k == 0 ? a.lo0 : k == 1 ? a.lo1 : a.lo2, hi = k == 0 ? a.hi0 : k == 1 ? a.hi1 : a.hi2;
                const float s = 2.0f * ((x - lo) / (hi - lo)) - 1.0f;
                x = is_act ? s : x;
            }
            v[j] = x;
        }
        if (c == kRepReward / 4) v[kRepReward % 4] = (float)a.reward[te];
        if (c == kRepDone / 4) {
            v[kRepDone % 4] = d ? 1.0f : 0.0f;
            v[kRepTimeout % 4] = a.handle_timeouts && d && a.complete[te] == 0 ? 1.0f : 0.0f;
        }
        unsigned row = (unsigned)a.row0 + (unsigned)(t - a.t0);        // both below rows <= 2^31 - 1
        if (row >= (unsigned)a.rows) row -= (unsigned)a.rows;
        float4 *dst = reinterpret_cast<float4 *>(a.store + ((size_t)row * n + (size_t)e) * kReplayR) + c;
        *dst = make_float4(v[0], v[1], v[2], v[3]);
    }
}
static_assert(kRepDone / 4 == kRepTimeout / 4, "done and timeout sit in one 16-byte piece");

struct ReplaySampleArgs {
    int n, rows, size, B;
    uint64_t seed, counter;
    const float *store;
    const int32_t *rows_in, *envs_in;     // both or neither; given: no draw
    float *obs, *act, *next, *dones, *rew;  // [B][18], [B][3], [B][18], [B][1], [B][1]
    int32_t *rows_out, *envs_out;         // [B], each nullable
};

constexpr int kReplayInFlight = 4;                                  // records a lane group has in flight
constexpr int kReplaySamples = kReplayGroups * kReplayInFlight;     // samples per workgroup
constexpr int kReplayStride = kReplayR + 4;                         // LDS row stride: 16-byte aligned, rows staggered over the banks
static_assert(kReplayThreads >= kReplaySamples, "one thread per sample draws its indices");

// A workgroup gathers kReplaySamples consecutive samples: one thread per sample draws (or reads) its (row, env); every
// group of kReplayLanes lanes then issues kReplayInFlight 16-byte loads per lane, one record each, before it waits for
// any; the records go to an LDS tile, from which the five outputs are written as runs of consecutive floats (sample-major,
// as the outputs are laid out), so every wave's stores are contiguous.  A caller-supplied index outside [0, rows) x
// [0, n_envs) reads nothing: that sample's outputs are NaN and its echoed row is -1.
//
// BATCHES (k_replay_sample_batches): a.B = n_batches * batch is the flat sample count and the outputs are [n_batches][batch][.],
// i.e. flat over j = g * batch + i.  Sample i of batch g draws with the Philox words (i, lo(counter + g), hi(counter + g),
// kReplayDrawTag), the 64-bit sum wrapping modulo 2^64: the bits of k_replay_sample at counter + g.  A workgroup's
// kReplaySamples samples may lie in two or more batches.  No caller indices.
template <bool BATCHES>
__device__ __forceinline__ void replay_sample_body(const ReplaySampleArgs &a, int batch)
{
    __shared__ __align__(16) float tile[kReplaySamples][kReplayStride];
    __shared__ int srow[kReplaySamples], senv[kReplaySamples];
    const int tid = (int)threadIdx.x;
    const int s0 = (int)blockIdx.x * kReplaySamples;
    const int ns = min(kReplaySamples, a.B - s0);
    if (tid < ns) {
        const int s = s0 + tid;
        int row, env;
        if (!BATCHES && a.rows_in) {
            row = a.rows_in[s];
            env = a.envs_in[s];
            if ((unsigned)row >= (unsigned)a.rows || (unsigned)env >= (unsigned)a.n) row = -1, env = 0;
        } else {
            const int g = BATCHES ? s / batch : 0;
            const uint64_t counter = a.counter + (uint64_t)g;
            uint32_t w[4];
            philox4x32((uint32_t)(s - g * batch), (uint32_t)counter, (uint32_t)(counter >> 32), kReplayDrawTag, (uint32_t)a.seed,
                       (uint32_t)(a.seed >> 32), w);
            row = (int)__umulhi(w[0], (uint32_t)a.size);
            env = (int)__umulhi(w[1], (uint32_t)a.n);
        }
        srow[tid] = row;
        senv[tid] = env;
        if (a.rows_out) a.rows_out[s] = row;
        if (a.envs_out) a.envs_out[s] = env;
    }
    __syncthreads();
    const int g = tid / kReplayLanes, c = tid % kReplayLanes;
    const float qnan = __int_as_float(0x7FC00000);
    float4 v[kReplayInFlight];
#pragma unroll
    for (int k = 0; k < kReplayInFlight; k++) {
        const int i = g + k * kReplayGroups;
        v[k] = make_float4(qnan, qnan, qnan, qnan);
        if (i < ns && srow[i] >= 0) {
            const size_t rec = (size_t)srow[i] * (size_t)a.n + (size_t)senv[i];
            v[k] = *(reinterpret_cast<const float4 *>(a.store + rec * kReplayR) + c);
        }
    }
#pragma unroll
    for (int k = 0; k < kReplayInFlight; k++)
        *reinterpret_cast<float4 *>(&tile[g + k * kReplayGroups][4 * c]) = v[k];
    __syncthreads();
    const size_t base = (size_t)s0;
    for (int j = tid; j < ns * kObsDim; j += kReplayThreads) {
        const int i = j / kObsDim, f = j % kObsDim;
        a.obs[base * kObsDim + j] = tile[i][f];
        a.next[base * kObsDim + j] = tile[i][kRepNext + f];
    }
    for (int j = tid; j < ns * 3; j += kReplayThreads) a.act[base * 3 + j] = tile[j / 3][kRepAct + j % 3];
    if (tid < ns) {
        a.dones[base + tid] = tile[tid][kRepDone] * (1.0f - tile[tid][kRepTimeout]);
        a.rew[base + tid] = tile[tid][kRepReward];
    }
}

__global__ __launch_bounds__(kReplayThreads) void k_replay_sample(ReplaySampleArgs a) { replay_sample_body<false>(a, 1); }

// n_batches minibatches of `batch` samples in one launch (meshenv_replay_sample_batches)
__global__ __launch_bounds__(kReplayThreads) void k_replay_sample_batches(ReplaySampleArgs a, int batch)
{
    replay_sample_body<true>(a, batch);
}

}  // namespace meshenv
