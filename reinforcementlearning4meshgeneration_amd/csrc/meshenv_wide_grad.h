// meshenv_wide_grad.h -- the two gradient statements of DDPG at SB3's default widths [400, 300] (SB3 2.x's TD3.train, which
// DDPG inherits, with n_critics = 1; the reference's DDPG('MlpPolicy', env), rl/baselines/RL_Mesh.py:113-228):
//
//   critic   q = Q1(cat(obs, actions)), d = q - y, critic_loss = loss_scale * (S / B) with S = sum d^2,
//            dq = (2 loss_scale) * (d / B), then the masked backward through 300 -> 400 -> 21
//   actor    a = tanh(mu(obs)), actor_loss = -mean(Q1(cat(obs, a))); the critic backward from dq = 1 down to the three action
//            columns (no critic weight gradient), d_pre = (-((dQ/da) / B)) * (1 - a a), dz_2 = (a_2 > 0) sum_i d_pre[i] W_3[i],
//            then the actor's backward
//
// Why not k_critic_grad<TD3> / k_td3_actor_grad: they give wave w neurons [16 w, 16 w + 16) of every layer (256 neurons at
// most) and keep dW_2 in registers across row tiles; dW_2 is 300 x 400 = 120 000 floats here.  Two phases instead, with the
// per-row results in a workspace between them, and an ordered reduction:
//
// Phase A, rows (k_wgrad_critic_rows, k_wgrad_actor_rows).  One 16-wave workgroup per 16-row tile, grid ceil(B / 16).  A layer
// is a list of 16-neuron output tiles dealt to the waves as wide_layer does (wave w takes tiles w and w + 16: 25 tiles of
// layer 1, 19 of layer 2); the weights are read from the LIVE torch tensors ([out][in] row-major): the B operand of a forward
// product is 16 contiguous bytes of row n (wg_dense), da = dz W reads W by columns through buffer loads (wg_da).  Row tile 18's
// neurons 300..303 and the head's k = 300..303 exist in no tensor: they are read as zero (a lane predicate in wg_dense and in
// wg_da; no load leaves a tensor).  Activations live in LDS in natural order, row strides 404 and 308 (conflict-free for the 16
// rows of a quarter-wave, as in meshenv_wide.h), in ONE pair of buffers: a lane computes the same (row, neuron) elements of a
// layer's activation and of its dz, so the ReLU masks stay in registers and the actor statement runs the critic through the
// buffers the actor's forward has left (48 KB of LDS for either statement).  Per row the phase writes to the workspace
//   x0 [B16][32]    the input row: observation, action (critic statement), a 1 in column 21, zeros elsewhere
//   a1 [B16][416]   post-ReLU layer 1, a 1 in column 400, zeros to 415
//   a2 [B16][320]   post-ReLU layer 2, zeros in 300..303, a 1 in column 304, zeros to 319
//   dz1 [B16][400], dz2 [B16][304] (zeros in 300..303)
//   dh [B16][4]     the head terms: critic (dq, 0, 0, d^2), actor (d_pre[0..2], q)
// B16 = B rounded up to 16.  Every padded row is written as 0 (the columns of ones excepted) and every padded column as
// above in the same call: phase B never reads a float that this call has not written.
//
// Phase B, weights (k_wgrad_weights).  dW_l = dz_l^T a_{l-1} with the batch rows as the MFMA K dimension; the columns of ones
// make db_l a column of the same product (column 400 of a1: db_2; column 21 of x0: db_1; column 304 of a2: the head's bias
// gradient and, against column 3 of dh, S or the sum of q).  kWgJobs = 564 output tiles of 16 x 16: 19 x 26 (dz2, a1), 25 x 2
// (dz1, x0), 1 x 20 (dh, a2); one wave per tile and chunk of rows, four waves per workgroup, grid (141, chunks).  A chunk is
// T = max(4, ceil(tiles / 64)) row tiles (tiles = ceil(B / 16)): 64 rows up to B = 4096 (4 chunks, 564 workgroups at B = 256),
// at most 64 chunks.  Then k_wgrad_reduce adds the chunks' partial tiles in chunk order into the gradient buffer (torch
// layout) and finishes the loss.
//
// ACCUMULATION ORDER (tests/ddpg_grad_ref.py restates it; nothing below depends on where a row sits in a workgroup or on B
// except the chunk count):
//   forward layers     two accumulators, acc0 the even 16-groups of k ascending, acc1 the odd ones, four MFMA steps per group
//                      (k = 16 g + 4 (lane >> 4) + j), then (acc0 + acc1) + bias.  Layer 1: 2 groups, 4 + 1 + 1 = 6 roundings
//                      on the longest path; layer 2: 25 groups, 13 in acc0, 52 + 1 + 1 = 54; head: 19 groups, 40 + 1 + 1 = 42
//                      (the counts of meshenv_wide.h)
//   da_1 = dz_2 W_2    over n = 0..303 in 19 groups, acc0 even / acc1 odd, then acc0 + acc1: 40 + 1 = 41
//   dQ/da = dz_1 W_1   over n = 0..399 in 25 groups: 52 + 1 = 53
//   head dz_2 (actor)  d_pre[0] W_3[0][n], then two fmaf, i ascending: 3
//   batch sums         one accumulator per chunk: rows ascending, four per MFMA step, counted one rounding per row, at most
//                      min(16 T, B16); then chunk 0 + chunk 1 + ... in index order, chunks - 1 additions
//   loss               critic: loss_scale * (S / B); actor: -(S / B)
// No floating-point atomics: repeated calls give the same bits.
#pragma once

#include "meshenv_td3_actor_grad.h"
#include "meshenv_wide.h"

namespace meshenv {

constexpr int kWgObs = kCgObs, kWgIn = kTgtIn;
constexpr int kWgH1 = kWideH1, kWgH2 = kWideH2, kWgH2Pad = kWideH2Pad;   // 400, 300, 304
constexpr int kWgS1 = kWideS1, kWgS2 = kWideS2;                           // LDS row strides 404, 308
constexpr int kWgX0 = 32, kWgA1 = 416, kWgA2 = 320, kWgDh = 4;            // workspace row strides
constexpr int kWgRowFloats = kWgX0 + kWgA1 + kWgA2 + kWgH1 + kWgH2Pad + kWgDh;   // 1476 floats per row
constexpr int kWgMaxRows = 65536;
constexpr int kWgMaxChunks = 64, kWgMinChunkTiles = 4;
constexpr int kWgJobsW2 = kWideT2 * 26, kWgJobsW1 = kWideT1 * 2, kWgJobsHead = 20;
constexpr int kWgJobs = kWgJobsW2 + kWgJobsW1 + kWgJobsHead;             // 564
constexpr int kWgJobWaves = 4;
static_assert(kWgJobs % kWgJobWaves == 0, "the weight phase's grid has no idle wave");

// The gradient set of one [400, 300] network in torch layout, bind order: w1 [400][KIN], b1, w2 [300][400], b2, head [NOUT][300],
// head bias [NOUT]; padded to a multiple of 64 floats
template <int KIN, int NOUT>
struct WgLayout {
    static constexpr int b1 = kWgH1 * KIN;
    static constexpr int w2 = b1 + kWgH1;
    static constexpr int b2 = w2 + kWgH2 * kWgH1;
    static constexpr int w3 = b2 + kWgH2;
    static constexpr int b3 = w3 + NOUT * kWgH2;
    static constexpr int params = b3 + NOUT;
    static constexpr int stride = (params + 63) & ~63;
};
using WgActor = WgLayout<kWgObs, 3>;     // 128 803 gradients in 128 832 floats
using WgCritic = WgLayout<kWgIn, 1>;     // 129 401 gradients in 129 408 floats

struct WgNet {
    const float *w[3], *b[3];   // two hidden layers and the head (torch layout)
};

struct WgSpace {
    float *x0, *a1, *a2, *dz1, *dz2, *dh;   // [rows16][kWgX0 | kWgA1 | kWgA2 | 400 | 304 | 4]
};

// chunks of the weight phase: tiles per chunk and their count
__host__ __device__ inline int wg_chunk_tiles(int n)
{
    const int tiles = (n + kCgRows - 1) / kCgRows, t = (tiles + kWgMaxChunks - 1) / kWgMaxChunks;
    return t < kWgMinChunkTiles ? kWgMinChunkTiles : t;
}

// acc0 / acc1 += x W^T over G 16-groups of k (G odd: the last group goes to acc0) for the lane's row of W: off = n * K + 4 q,
// valid: false reads a zero row; the lanes of the last quarter-wave read zeros in the last group when TAIL (k = 16 G - 4 ..
// 16 G - 1 is past the row: K = 16 G - 4); xr = &x[e][4 q]
template <int G, bool TAIL>
__device__ __forceinline__ void wg_dense(const float *__restrict__ w, unsigned off, bool valid, int q, const float *xr, f32x4 &acc0,
                                         f32x4 &acc1)
{
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int g = 0; g < G; g++) {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(xr + 16 * g);
        const bool in = valid && !(TAIL && g == G - 1 && q == 3);
        const f32x4 b = in ? *reinterpret_cast<const f32x4 *>((w + 16 * g) + off) : zero;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (g & 1) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], acc1, 0, 0, 0);
            else acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], acc0, 0, 0, 0);
        }
    }
}

// da[row = 4 q + reg][k0] = sum_n dz[row][n] W[n][k0] over G 16-groups of n (acc0 even, acc1 odd, then their sum); W [N][K] is
// read by columns through buffer loads (one descriptor and one lane offset, as cg_da).  N = 16 G - 4 (TAIL): the rows
// 16 G - 4 .. 16 G - 1 of the last group do not exist; their lanes (the last quarter-wave) read the third quarter's rows
// instead and their B operand is 0, so no load leaves the tensor.  col: the lane's column, use: false makes the lane's B operand 0
template <int G, int N, int K>
__device__ __forceinline__ f32x4 wg_da(const float *w, const float *dz, int S, int e, int q, int col, bool use)
{
    constexpr bool TAIL = N < 16 * G;
    static_assert(N == 16 * G || N == 16 * G - 4, "whole 16-groups of rows, or one short quarter");
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    const float *xr = dz + e * S + 4 * q;
    const __amdgpu_buffer_rsrc_t wl = __builtin_amdgcn_make_buffer_rsrc((void *)w, 0, N * K * 4, kCgBufferFlags);
    const int voff = (4 * q * K + col) * 4;
    const int voff_tail = q == 3 ? (8 * K + col) * 4 : voff;   // the last quarter-wave re-reads the third quarter's rows
#pragma unroll
    for (int g = 0; g < G; g++) {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(xr + 16 * g);
        const bool last = TAIL && g == G - 1;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float l = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(wl, last ? voff_tail : voff, (16 * g + j) * K * 4, 0));
            const float b = (use && !(last && q == 3)) ? l : 0.0f;
            if (g & 1) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b, acc1, 0, 0, 0);
            else acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b, acc0, 0, 0, 0);
        }
    }
    f32x4 r;
#pragma unroll
    for (int reg = 0; reg < 4; reg++) r[reg] = acc0[reg] + acc1[reg];
    return r;
}

// v[reg] of neuron n0 (rows 4 q + reg) -> the LDS buffer (stride S), the workspace rows (stride WS; 0 for the rows past n)
// and out [n][H] (nullable; neurons below H, rows below n)
template <int H>
__device__ __forceinline__ void wg_store(float *buf, int S, float *ws, int WS, float *out, const f32x4 &v, int row0, int n, int q,
                                         int n0)
{
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
        const int row = 4 * q + reg, gr = row0 + row;
        buf[row * S + n0] = v[reg];
        ws[(unsigned)(gr * WS + n0)] = gr < n ? v[reg] : 0.0f;
        if (out && gr < n && n0 < H) out[(unsigned)(gr * H + n0)] = v[reg];
    }
}

// the columns past a workspace matrix's activations, by one wave: a 1 in column C, zeros in C + 1 .. C + 15
__device__ __forceinline__ void wg_ones(float *ws, int WS, int C, int row0, int lane)
{
    const int e = lane & 15, q = lane >> 4;
#pragma unroll
    for (int reg = 0; reg < 4; reg++) ws[(unsigned)((row0 + 4 * q + reg) * WS + C + e)] = e == 0 ? 1.0f : 0.0f;
}

// The two hidden layers of one network over the tile's rows: a_1 -> h1 (and ws1, out1), a_2 -> h2 (and ws2, out2); the
// lane's elements stay in v1 / v2 (tile `wave` in [0], `wave + 16` in [1]; zero where the wave has no second tile).  x0 must
// be staged behind a barrier; ends behind a barrier.  ws1 / ws2 nullable (the critic of the actor statement).
template <int KIN>
__device__ __forceinline__ void wg_forward(const WgNet &N, const float *x0, float *h1, float *h2, float *ws1, float *ws2, float *out1,
                                           float *out2, int row0, int n, int wave, int lane, f32x4 (&v1)[2], f32x4 (&v2)[2])
{
    const int e = lane & 15, q = lane >> 4;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int it = 0; it < 2; it++) {
        v1[it] = zero;
        const int tile = wave + 16 * it;
        if (tile >= kWideT1) continue;
        const int n0 = 16 * tile + e;
        v1[it] = cg_first_layer<KIN, kPolicyReLU>(N.w[0], N.b[0], x0, e, q, n0);
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int row = 4 * q + reg, gr = row0 + row;
            h1[row * kWgS1 + n0] = v1[it][reg];
            if (ws1) ws1[(unsigned)(gr * kWgA1 + n0)] = gr < n ? v1[it][reg] : 0.0f;
            if (out1 && gr < n) out1[(unsigned)(gr * kWgH1 + n0)] = v1[it][reg];
        }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 2; it++) {
        v2[it] = zero;
        const int tile = wave + 16 * it;
        if (tile >= kWideT2) continue;
        const int n0 = 16 * tile + e;
        const bool valid = n0 < kWgH2;
        const unsigned row = valid ? (unsigned)n0 : 0u;
        f32x4 acc0 = zero, acc1 = zero;
        wg_dense<kWideG2, false>(N.w[1], row * kWgH1 + 4 * q, valid, q, h1 + e * kWgS1 + 4 * q, acc0, acc1);
        const float b = valid ? N.b[1][row] : 0.0f;
#pragma unroll
        for (int reg = 0; reg < 4; reg++) v2[it][reg] = fmaxf((acc0[reg] + acc1[reg]) + b, 0.0f);
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int r = 4 * q + reg, gr = row0 + r;
            h2[r * kWgS2 + n0] = v2[it][reg];
            if (ws2) ws2[(unsigned)(gr * kWgA2 + n0)] = gr < n ? v2[it][reg] : 0.0f;
            if (out2 && gr < n && valid) out2[(unsigned)(gr * kWgH2 + n0)] = v2[it][reg];
        }
    }
    __syncthreads();
}

// The head over h2 for the wave that calls it: out[reg] = (acc0 + acc1) + bias of output e < NOUT, rows 4 q + reg
template <int NOUT>
__device__ __forceinline__ void wg_head(const WgNet &N, const float *h2, int lane, float (&out)[4])
{
    const int e = lane & 15, q = lane >> 4;
    const bool valid = e < NOUT;
    const unsigned hr = valid ? (unsigned)e : 0u;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    wg_dense<kWideGH, true>(N.w[2], hr * kWgH2 + 4 * q, valid, q, h2 + e * kWgS2 + 4 * q, acc0, acc1);
    const float bh = valid ? N.b[2][hr] : 0.0f;
#pragma unroll
    for (int reg = 0; reg < 4; reg++) out[reg] = (acc0[reg] + acc1[reg]) + bh;
}

// dz_2 of the lane's elements -> h2 and the workspace (nullable); then, behind barriers, da_1 = dz_2 W_2 and
// dz_1 = a_1 > 0 ? da_1 : 0 -> h1 (if KEEP1) and the workspace (nullable).  Every wave has finished reading h2 before the call.
template <bool KEEP1>
__device__ __forceinline__ void wg_backward(const float *w2, float *h1, float *h2, float *wsdz1, float *wsdz2, const f32x4 (&dz2)[2],
                                            const f32x4 (&v1)[2], int row0, int wave, int lane)
{
    const int e = lane & 15, q = lane >> 4;
#pragma unroll
    for (int it = 0; it < 2; it++) {
        const int tile = wave + 16 * it;
        if (tile >= kWideT2) continue;
        const int n0 = 16 * tile + e;
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int row = 4 * q + reg;
            h2[row * kWgS2 + n0] = dz2[it][reg];
            if (wsdz2) wsdz2[(unsigned)((row0 + row) * kWgH2Pad + n0)] = dz2[it][reg];
        }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 2; it++) {
        const int tile = wave + 16 * it;
        if (tile >= kWideT1) continue;
        const int n0 = 16 * tile + e;
        const f32x4 da = wg_da<kWideT2, kWgH2, kWgH1>(w2, h2, kWgS2, e, q, n0, true);
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int row = 4 * q + reg;
            const float dz = v1[it][reg] > 0.0f ? da[reg] : 0.0f;
            if (KEEP1) h1[row * kWgS1 + n0] = dz;   // (h1 was last read by the forward's layer 2, barriers ago)
            if (wsdz1) wsdz1[(unsigned)((row0 + row) * kWgH1 + n0)] = dz;
        }
    }
}

struct WgCriticArgs {
    int n;
    float two_scale;                       // 2 loss_scale
    const float *obs, *actions, *target;   // [n][18], [n][3], [n]
    WgNet c;
    WgSpace ws;
    float *q, *acts[2];                    // [n], [n][400], [n][300]; nullable
};

__global__ void __launch_bounds__(64 * kWideWaves)
k_wgrad_critic_rows(WgCriticArgs A)
{
    __shared__ __attribute__((aligned(16))) float x0[kCgRows * kCgInStride];
    __shared__ __attribute__((aligned(16))) float h1[kCgRows * kWgS1];
    __shared__ __attribute__((aligned(16))) float h2[kCgRows * kWgS2];
    __shared__ float s_dq[kCgRows];
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int e = lane & 15, q = lane >> 4, row0 = blockIdx.x * kCgRows;
    cg_stage<64 * kWideWaves, true>(x0, A.obs, A.actions, row0, A.n, t);
    __syncthreads();
    if (t < kCgRows * kWgX0) A.ws.x0[(unsigned)(row0 * kWgX0 + t)] = x0[(t >> 5) * kCgInStride + (t & 31)];
    if (wave == 15) wg_ones(A.ws.a1, kWgA1, kWgH1, row0, lane);
    if (wave == 14) wg_ones(A.ws.a2, kWgA2, kWgH2Pad, row0, lane);
    f32x4 v1[2], v2[2];
    wg_forward<kWgIn>(A.c, x0, h1, h2, A.ws.a1, A.ws.a2, A.acts[0], A.acts[1], row0, A.n, wave, lane, v1, v2);
    if (wave == 0) {
        float qv[4];
        wg_head<1>(A.c, h2, lane, qv);
        if (e == 0) {
            const float fn = (float)A.n;
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int row = 4 * q + reg, gr = row0 + row;
                const bool in = gr < A.n;
                const float d = in ? qv[reg] - A.target[gr] : 0.0f;
                const float dq = in ? A.two_scale * (d / fn) : 0.0f;
                s_dq[row] = dq;
                *reinterpret_cast<f32x4 *>(A.ws.dh + (unsigned)(gr * kWgDh)) = f32x4{dq, 0.0f, 0.0f, d * d};
                if (in && A.q) A.q[gr] = qv[reg];
            }
        }
    }
    __syncthreads();   // the head has read h2; s_dq
    f32x4 dz2[2];
#pragma unroll
    for (int it = 0; it < 2; it++) {
        const int n0 = 16 * (wave + 16 * it) + e;
        const float wo = n0 < kWgH2 ? A.c.w[2][n0] : 0.0f;
#pragma unroll
        for (int reg = 0; reg < 4; reg++) dz2[it][reg] = v2[it][reg] > 0.0f ? s_dq[4 * q + reg] * wo : 0.0f;
    }
    wg_backward<false>(A.c.w[1], h1, h2, A.ws.dz1, A.ws.dz2, dz2, v1, row0, wave, lane);
}

struct WgActorArgs {
    int n;
    const float *obs;                     // [n][18]
    WgNet a, c;                           // the actor, the critic
    WgSpace ws;
    float *actions, *q, *dq_da, *d_pre;   // [n][3] [n] [n][3] [n][3], every one nullable
    float *acts[2][2];                    // [actor, critic][layer]: [n][400], [n][300] post-ReLU activations, nullable
};

__global__ void __launch_bounds__(64 * kWideWaves)
k_wgrad_actor_rows(WgActorArgs A)
{
    __shared__ __attribute__((aligned(16))) float x0[kCgRows * kCgInStride];
    __shared__ __attribute__((aligned(16))) float h1[kCgRows * kWgS1];
    __shared__ __attribute__((aligned(16))) float h2[kCgRows * kWgS2];
    __shared__ float s_a[kCgRows * 4], s_d[kCgRows * 4], s_q[kCgRows];
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int e = lane & 15, q = lane >> 4, row0 = blockIdx.x * kCgRows;
    const float fn = (float)A.n;
    cg_stage<64 * kWideWaves, false>(x0, A.obs, nullptr, row0, A.n, t);
    __syncthreads();
    if (t < kCgRows * kWgX0) A.ws.x0[(unsigned)(row0 * kWgX0 + t)] = x0[(t >> 5) * kCgInStride + (t & 31)];
    if (wave == 15) wg_ones(A.ws.a1, kWgA1, kWgH1, row0, lane);
    if (wave == 14) wg_ones(A.ws.a2, kWgA2, kWgH2Pad, row0, lane);
    // ---- the actor's forward; its masks stay in a1 / a2
    f32x4 a1[2], a2[2];
    wg_forward<kWgObs>(A.a, x0, h1, h2, A.ws.a1, A.ws.a2, A.acts[0][0], A.acts[0][1], row0, A.n, wave, lane, a1, a2);
    if (wave == 0) {
        float pre[4];
        wg_head<3>(A.a, h2, lane, pre);
        if (e < 3) {
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int row = 4 * q + reg, gr = row0 + row;
                const bool in = gr < A.n;
                const float a = in ? tanhf(pre[reg]) : 0.0f;
                x0[row * kCgInStride + kWgObs + e] = a;   // (the workspace's x0 is written: it keeps the observation alone)
                s_a[row * 4 + e] = a;
                if (in && A.actions) A.actions[(unsigned)(gr * 3 + e)] = a;
            }
        }
    }
    __syncthreads();   // the action is in x0; the head has read h2
    // ---- the critic through the same buffers: forward, q, then dQ/da from dq = 1
    {
        f32x4 c1[2], c2[2];
        wg_forward<kWgIn>(A.c, x0, h1, h2, nullptr, nullptr, A.acts[1][0], A.acts[1][1], row0, A.n, wave, lane, c1, c2);
        if (wave == 0) {
            float qv[4];
            wg_head<1>(A.c, h2, lane, qv);
            if (e == 0) {
#pragma unroll
                for (int reg = 0; reg < 4; reg++) {
                    const int row = 4 * q + reg, gr = row0 + row;
                    s_q[row] = gr < A.n ? qv[reg] : 0.0f;
                    if (gr < A.n && A.q) A.q[gr] = qv[reg];
                }
            }
        }
        __syncthreads();   // the head has read h2
        f32x4 dz2[2];
#pragma unroll
        for (int it = 0; it < 2; it++) {
            const int n0 = 16 * (wave + 16 * it) + e;
            const float wo = n0 < kWgH2 ? A.c.w[2][n0] : 0.0f;
#pragma unroll
            for (int reg = 0; reg < 4; reg++) dz2[it][reg] = c2[it][reg] > 0.0f ? wo : 0.0f;
        }
        wg_backward<true>(A.c.w[1], h1, h2, nullptr, nullptr, dz2, c1, row0, wave, lane);
    }
    __syncthreads();   // dz_1 of the critic is in h1
    if (wave == 0) {   // dQ/da[row][k] = sum_n dz_1[row][n] W^q_1[n][18 + k], then the head gradient
        const bool use = e < 3;
        const f32x4 dq = wg_da<kWideT1, kWgH1, kWgIn>(A.c.w[0], h1, kWgS1, e, q, kWgObs + (use ? e : 0), use);
        if (e < 4) {
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int row = 4 * q + reg, gr = row0 + row;
                const bool in = gr < A.n;
                float d;
                if (use) {
                    const float a = s_a[row * 4 + e];
                    d = in ? (-(dq[reg] / fn)) * (1.0f - a * a) : 0.0f;
                    if (in && A.dq_da) A.dq_da[(unsigned)(gr * 3 + e)] = dq[reg];
                    if (in && A.d_pre) A.d_pre[(unsigned)(gr * 3 + e)] = d;
                } else {
                    d = s_q[row];
                }
                s_d[row * 4 + e] = d;
                A.ws.dh[(unsigned)(gr * kWgDh + e)] = d;
            }
        }
    }
    __syncthreads();   // d_pre; every wave is past the critic's h2
    // ---- the actor's backward
    f32x4 dz2[2];
#pragma unroll
    for (int it = 0; it < 2; it++) {
        const int n0 = 16 * (wave + 16 * it) + e;
        const bool valid = n0 < kWgH2;
        float w3[3];
#pragma unroll
        for (int i = 0; i < 3; i++) w3[i] = valid ? A.a.w[2][i * kWgH2 + n0] : 0.0f;
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const float *d = s_d + (4 * q + reg) * 4;
            float v = d[0] * w3[0];
            v = fmaf(d[1], w3[1], v);
            v = fmaf(d[2], w3[2], v);
            dz2[it][reg] = a2[it][reg] > 0.0f ? v : 0.0f;
        }
    }
    wg_backward<false>(A.a.w[1], h1, h2, A.ws.dz1, A.ws.dz2, dz2, a1, row0, wave, lane);
}

// Phase B: wave `job` of chunk blockIdx.y: the 16 x 16 tile sum_rows dz[row][16 nt + i] act[row][16 kt + j] over the chunk's
// rows -> partial [chunk][job][lane][4] (D[i = 4 q + reg][j = e])
__global__ void __launch_bounds__(64 * kWgJobWaves)
k_wgrad_weights(WgSpace ws, int rows16, int chunk_rows, float *__restrict__ partial)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int e = lane & 15, q = lane >> 4;
    const int job = blockIdx.x * kWgJobWaves + wave;
    const float *dz, *act;
    int sd, sa;
    bool use = true;
    if (job < kWgJobsW2) {
        const int nt = job / 26, kt = job - 26 * nt;
        dz = ws.dz2 + 16 * nt; sd = kWgH2Pad; act = ws.a1 + 16 * kt; sa = kWgA1;
    } else if (job < kWgJobsW2 + kWgJobsW1) {
        const int j = job - kWgJobsW2, nt = j >> 1, kt = j & 1;
        dz = ws.dz1 + 16 * nt; sd = kWgH1; act = ws.x0 + 16 * kt; sa = kWgX0;
    } else {
        const int kt = job - kWgJobsW2 - kWgJobsW1;
        dz = ws.dh; sd = kWgDh; act = ws.a2 + 16 * kt; sa = kWgA2;
        use = e < kWgDh;
    }
    const int r0 = blockIdx.y * chunk_rows, r1 = min(r0 + chunk_rows, rows16);
    const int ed = use ? e : 0;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int r = r0; r < r1; r += kCgRows) {   // a row tile: four MFMA steps of four rows, rows ascending
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const unsigned row = (unsigned)(r + 4 * s + q);
            const float l = dz[row * sd + ed];
            const float a = use ? l : 0.0f;
            const float b = act[row * sa + e];
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
        }
    }
    *reinterpret_cast<f32x4 *>(partial + ((size_t)blockIdx.y * kWgJobs + job) * 256 + lane * 4) = acc;
}

// The chunks' partial tiles added in chunk order into grad (torch layout of WgLayout<KIN, NOUT>); element (i = 3, column 304)
// of the head's product is S: loss = scale * (S / B), scale = loss_scale (critic) or -1 (actor)
template <int KIN, int NOUT>
__global__ void __launch_bounds__(256)
k_wgrad_reduce(const float *__restrict__ partial, int chunks, int n, float scale, float *__restrict__ grad, float *__restrict__ loss)
{
    using L = WgLayout<KIN, NOUT>;
    const int job = blockIdx.x, r = threadIdx.x, i = r >> 4, j = r & 15;
    const float *p = partial + (size_t)job * 256 + (((i >> 2) * 16 + j) * 4 + (i & 3));
    float s = p[0];
#pragma unroll 4
    for (int c = 1; c < chunks; c++) s = s + p[(size_t)c * kWgJobs * 256];
    if (job < kWgJobsW2) {
        const int nt = job / 26, kt = job - 26 * nt, nn = 16 * nt + i, k = 16 * kt + j;
        if (nn >= kWgH2) return;
        if (k < kWgH1) grad[L::w2 + nn * kWgH1 + k] = s;
        else if (k == kWgH1) grad[L::b2 + nn] = s;
    } else if (job < kWgJobsW2 + kWgJobsW1) {
        const int jj = job - kWgJobsW2, nn = 16 * (jj >> 1) + i, k = 16 * (jj & 1) + j;
        if (k < KIN) grad[nn * KIN + k] = s;
        else if (k == kCgOnes) grad[L::b1 + nn] = s;
    } else {
        const int k = 16 * (job - kWgJobsW2 - kWgJobsW1) + j;
        if (i < NOUT) {
            if (k < kWgH2) grad[L::w3 + i * kWgH2 + k] = s;
            else if (k == kWgH2Pad) grad[L::b3 + i] = s;
        } else if (i == 3 && k == kWgH2Pad) {
            loss[0] = scale * (s / (float)n);
        }
    }
}

}  // namespace meshenv
