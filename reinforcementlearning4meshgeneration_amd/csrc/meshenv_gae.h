// meshenv_gae.h -- generalised advantage estimation over a rollout's histories: SB3's
// RolloutBuffer.compute_returns_and_advantage (GAE, SB3 2.x) with the TimeLimit.truncated bootstrap of collect_rollouts
// (rewards += gamma * V(terminal obs)) in front, bit-identical to that float32 loop (examples/ppo_rollout.py::gae):
//
//   g = (float)gamma, gl = (float)(gamma * gae_lambda), last = 0
//   for t = T-1 .. 0:
//     r = (float)reward[t];  if terminal_value: r = r + g * terminal_value[t]
//     nnt = 1 - (done[t] ? 1 : 0);  next_v = t == T-1 ? last_value : value[t+1]
//     delta = (r + (g * next_v) * nnt) - value[t];  last = delta + (gl * nnt) * last
//     advantage[t] = last, returns[t] = last + value[t], buffer_reward[t] = r
//
// The build's -ffp-contract=off keeps every product and sum a separate rounding, as numpy and torch evaluate them; f32
// denormals are not flushed.  The chain is not re-associated (a scan across T would round differently).
//
// Layout.  Histories are [T][n] row-major.  A workgroup owns kGaeEnvs environments and walks time tiles of
// THREADS / kGaeEnvs * kGaeRowsPerThread rows from the last tile to the first.  Each thread owns one environment column and
// kGaeRowsPerThread rows of a tile: it loads them with coalesced loads along n, computes r, delta and gl * nnt elementwise
// into LDS, and the next tile's loads are issued before the chain of the current tile runs, so they are in flight while it
// does.  The chain itself (two dependent VALU per step) runs on kGaeEnvs lanes of wave 0 out of LDS; then all threads write
// advantage, returns and buffer_reward, coalesced.
//
// Two shapes (meshenv_gae picks by T): 256 threads (128-row tiles) up to T = 128, where a longer tile would leave rows idle, and 512
// threads (256-row tiles) beyond, where at 4096 envs one workgroup per CU streams the whole history and a tile twice as
// long doubles the bytes each chain hides (MI355X, T = 2048 x 4096 envs: 89 -> 68 us; 128 x 65 536: 42 us against 73).
#pragma once

namespace meshenv {

constexpr int kGaeEnvs = 16;           // environments per workgroup
constexpr int kGaeRowsPerThread = 8;
constexpr int kGaeShortT = 128;        // longest history of the 256-thread shape

struct GaeArgs {
    int T, n;
    float g, gl;                  // (float)gamma, (float)(gamma * gae_lambda)
    const double *reward;         // [T][n]
    const float *value;           // [T][n]
    const uint8_t *done;          // [T][n]
    const float *tvalue;          // [T][n] or nullptr
    const float *last_value;      // [n]
    float *adv;                   // [T][n]
    float *ret, *brew;            // [T][n], each nullable
};

struct GaeIn {
    double r;
    float v, vn, tv;
    uint8_t d;
};

template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_gae(GaeArgs a)
{
    constexpr int kGaeRowsPerPass = THREADS / kGaeEnvs;
    constexpr int kGaeTile = kGaeRowsPerPass * kGaeRowsPerThread;
    __shared__ float2 dc[kGaeTile][kGaeEnvs];   // (delta, gl * nnt)
    __shared__ float adv[kGaeTile][kGaeEnvs];
    // neighbouring env blocks share cache lines (16 floats = half a 128-B line, 16 bytes of done): keep them on one XCD's
    // L2 (workgroup i is dispatched to XCD i % 8)
    const int G = (int)gridDim.x, bid = (int)blockIdx.x;
    const int blk = G % 8 == 0 ? (bid % 8) * (G / 8) + bid / 8 : bid;
    const int le = (int)threadIdx.x % kGaeEnvs, lr = (int)threadIdx.x / kGaeEnvs;
    const int e = blk * kGaeEnvs + le;
    const bool env_ok = e < a.n;
    const size_t n = (size_t)a.n;
    const int T = a.T;

    auto load = [&](int tile, GaeIn (&in)[kGaeRowsPerThread]) {
#pragma unroll
        for (int j = 0; j < kGaeRowsPerThread; j++) {
            const int t = tile * kGaeTile + lr + j * kGaeRowsPerPass;
            if (env_ok && t < T) {
                const size_t o = (size_t)t * n + (size_t)e;
                in[j].r = a.reward[o];
                in[j].v = a.value[o];
                in[j].d = a.done[o];
                in[j].tv = a.tvalue ? a.tvalue[o] : 0.0f;
                in[j].vn = t + 1 < T ? a.value[o + n] : a.last_value[e];
            }
        }
    };

    float last = 0.0f;   // the chain's carry (threads < kGaeEnvs)
    // one tile: cur holds its inputs; the loads of the previous tile in time go to nxt before the chain runs
    auto step = [&](int tile, GaeIn (&cur)[kGaeRowsPerThread], GaeIn (&nxt)[kGaeRowsPerThread]) {
        const int t0 = tile * kGaeTile;
        const int rows = min(kGaeTile, T - t0);
        float rr[kGaeRowsPerThread];
#pragma unroll
        for (int j = 0; j < kGaeRowsPerThread; j++) {
            const int row = lr + j * kGaeRowsPerPass;
            rr[j] = 0.0f;
            if (env_ok && row < rows) {
                float r = (float)cur[j].r;
                if (a.tvalue) r = r + a.g * cur[j].tv;
                const float nnt = 1.0f - (cur[j].d ? 1.0f : 0.0f);
                const float delta = (r + (a.g * cur[j].vn) * nnt) - cur[j].v;
                dc[row][le] = make_float2(delta, a.gl * nnt);
                rr[j] = r;
            }
        }
        if (tile > 0) load(tile - 1, nxt);
        __syncthreads();
        if ((int)threadIdx.x < kGaeEnvs && env_ok) {
#pragma unroll 8
            for (int i = rows - 1; i >= 0; i--) {
                const float2 x = dc[i][le];
                last = x.x + x.y * last;
                adv[i][le] = last;
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kGaeRowsPerThread; j++) {
            const int row = lr + j * kGaeRowsPerPass;
            if (env_ok && row < rows) {
                const size_t o = (size_t)(t0 + row) * n + (size_t)e;
                const float A = adv[row][le];
                a.adv[o] = A;
                if (a.ret) a.ret[o] = A + cur[j].v;
                if (a.brew) a.brew[o] = rr[j];
            }
        }
    };

    GaeIn A[kGaeRowsPerThread], B[kGaeRowsPerThread];
    const int ntiles = (T + kGaeTile - 1) / kGaeTile;
    load(ntiles - 1, A);
    // two tiles per iteration with the buffers' roles swapped, so that no register copy waits on the loads in flight
    for (int tile = ntiles - 1; tile >= 0; tile -= 2) {
        step(tile, A, B);
        if (tile >= 1) step(tile - 1, B, A);
    }
}

}  // namespace meshenv
