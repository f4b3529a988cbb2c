// meshenv_wide.h -- the forward engine of DDPG's networks: a ReLU MLP with two hidden layers of widths (400, 300), SB3's
// default net_arch of TD3Policy, which the reference's DDPG('MlpPolicy', env) uses for the actor and for the critic
// (rl/baselines/RL_Mesh.py:113-228, v2/src/mesh_rl/algorithms/sb3_algos.py:31-43).  Two kernels on it:
//   k_wide_policy   the deterministic kind of meshenv_policy.h at [400, 300]: s = tanh(mu(latent)), with noise
//                   s = clamp(s + sigma * eps, -1, 1); buffer_action = s, action = low + 0.5 (s + 1)(high - low)
//   k_wide_target   DDPG's TD target (SB3's TD3.train block with n_critics = 1), actor then Q1 in one launch:
//                   a = clamp(tanh(mu(next_obs)) + clamp(policy_noise * eps, -noise_clip, noise_clip), -1, 1)
//                   target = reward + (1 - done) * gamma * Q1(next_obs ++ a)
//
// Why not k_policy_forward<H>: that kernel gives one wavefront 16 neurons of EVERY layer and keeps the wave's weights in
// registers, which ends at 16 waves x 16 = 256 neurons.  Here a layer is a list of 16-neuron output tiles that the waves
// of the workgroup take in turn, and a tile's weights are streamed through registers group by group.
//
// Tiles (v_mfma_f32_16x16x4_f32: exact f32, 16 rows = MFMA M; a K group is 16 inputs = four MFMAs):
//   layer 1   K = 32  (18 observations, or 21 = cat(obs, action), zero-padded)   2 groups   25 tiles (400 neurons)
//   layer 2   K = 400                                                            25 groups   19 tiles (300 neurons + 4 padding)
//   head      K = 304 (300 + 4 padding)                                          19 groups    1 tile  (mu0..2 or q, 13+ padding)
// Weights are packed [tile][group][lane 64][4] in the per-lane B-operand order of pack_matrix_element (meshenv_pack.h);
// whatever no source tensor covers (neurons 300..303 of layer 2 and their bias, k = 300..303 of the head, the head's unused
// columns) is the zero of the buffer's one memset, so the padded activations are relu(0 + 0) = 0.  Bias blocks are padded
// to the tile count (400, 304, 16): no lane reads past one.
//
// Tile-to-wave table.  A workgroup has kWideWaves = 16 wavefronts (1024 threads, the launch limit) and kWideMT row tiles
// (R = 16 kWideMT rows).  Wave w takes
//   layer 1   tiles w and w + 16        (waves 0..8 two tiles, 9..15 one)
//   layer 2   tiles w and w + 16        (waves 0..2 two tiles, 3..15 one); waves sit round-robin on the four SIMDs, so the
//                                       matrix pipes carry 5, 5, 5 and 4 tiles
//   head      wave m < kWideMT takes row tile m
// and computes its tile for all kWideMT row tiles from ONE load of each B operand (the weights of a group are read once
// per workgroup, not once per 16 rows).
//
// Accumulation order (the tests' bound is derived from it, tests/ddpg_ref.py).  Per output element, two accumulators:
// acc0 takes the even k-groups 0, 2, 4, ... in ascending order, acc1 the odd ones; inside a group the four MFMAs run
// j = 0..3 (k = 4 (4 g + j) + (lane >> 4)).  Then (acc0 + acc1) + bias.  With G groups acc0 holds ceil(G / 2) of them:
//   layer 1: G = 2,  4 * 1 fused steps + 1 join + 1 bias =  6
//   layer 2: G = 25, 4 * 13             + 1      + 1      = 54
//   head:    G = 19, 4 * 10             + 1      + 1      = 42
// The order does not depend on kWideMT, on the row's position in the workgroup or on n: a row's result is the same bits
// in every launch.
//
// LDS (dynamic): x0 [R][36] (the input rows, K = 32 layout of meshenv_policy.h), h1 [R][404], h2 [R][308] in the k-permuted
// layout (position (k & 3) * (K / 4) + (k >> 2); strides 404 and 308 = 20 and 52 mod 64: the 16 lanes of a ds_read_b128
// start on 16 distinct multiples of four banks), eps [R][4]: 48 128 bytes at R = 16, 96 256 at R = 32, 144 384 at R = 48.
// R = 64 would need 192 512 bytes; a CU has 163 840.  R = 16 is the measured choice (32 and 48 rows
// re-read fewer weights but are slower up to 4096 rows and no different at 65 536); MESHENV_WIDE_MT builds the others.
#pragma once

#include "meshenv_policy.h"

namespace meshenv {

#ifndef MESHENV_WIDE_MT
#define MESHENV_WIDE_MT 1
#endif

constexpr int kWideH1 = 400, kWideH2 = 300;
constexpr int kWideT1 = 25, kWideT2 = 19;         // output tiles of layers 1 and 2
constexpr int kWideG2 = 25, kWideGH = 19;         // K groups of layer 2 and of the head
constexpr int kWideH2Pad = 16 * kWideT2;          // 304
constexpr int kWideS1 = kWideH1 + 4, kWideS2 = kWideH2Pad + 4;   // LDS row strides
constexpr int kWideWaves = 16;
constexpr int kWideMT = MESHENV_WIDE_MT;          // row tiles per workgroup
constexpr int kWideRows = 16 * kWideMT;
constexpr int kWideLdsFloats = kWideRows * (kPolInStride + kWideS1 + kWideS2 + 4);
static_assert(kWideMT >= 1 && kWideLdsFloats * sizeof(float) <= 160 * 1024, "the activations of R rows must fit a CU's 160 KiB of LDS");

struct WideNet {
    const float *w1p, *b1;  // [25][2][64][4], [400]
    const float *w2p, *b2;  // [19][25][64][4], [304]
    const float *whp, *bh;  // [19][64][4], [16]
};

// acc[m] = the 16 x 16 tile of row tile m over G k-groups (the accumulation order of the header); wp: the tile's packed
// weights [G][64][4]; x: LDS rows of stride xs in the permuted layout of a 16 G-input layer
template <int G, int MT>
__device__ __forceinline__ void wide_tile(const float *__restrict__ wp, const float *x, int xs, int lane, f32x4 (&acc)[MT])
{
    const int e = lane & 15, q = lane >> 4;
    f32x4 a0[MT], a1[MT];
#pragma unroll
    for (int m = 0; m < MT; m++) a0[m] = a1[m] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float *xr = x + e * xs + q * (4 * G);
    const f32x4 *w = reinterpret_cast<const f32x4 *>(wp) + lane;
#pragma unroll
    for (int g = 0; g < G; g++) {
        const f32x4 b = w[g * 64];
#pragma unroll
        for (int m = 0; m < MT; m++) {
            const f32x4 a = *reinterpret_cast<const f32x4 *>(xr + m * 16 * xs + 4 * g);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (g & 1) a1[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], a1[m], 0, 0, 0);
                else a0[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], a0[m], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int m = 0; m < MT; m++) acc[m] = a0[m] + a1[m];
}

// One hidden layer: the waves take the NT tiles in turn; y = relu(W x + b) into the permuted layout of a KN-input layer
// (row stride ys).  D[row = 4 (lane >> 4) + reg][col = lane & 15].
template <int G, int NT, int KN, int MT>
__device__ __forceinline__ void wide_layer(const float *__restrict__ wp, const float *__restrict__ bias, const float *x, int xs,
                                           float *y, int ys, int wave, int lane)
{
    const int e = lane & 15, q = lane >> 4;
    for (int tile = wave; tile < NT; tile += kWideWaves) {
        f32x4 acc[MT];
        wide_tile<G, MT>(wp + (size_t)tile * G * 256, x, xs, lane, acc);
        const int n0 = 16 * tile + e;
        const float b0 = bias[n0];
        const int p0 = (n0 & 3) * (KN / 4) + (n0 >> 2);
#pragma unroll
        for (int m = 0; m < MT; m++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) y[(16 * m + 4 * q + reg) * ys + p0] = fmaxf(acc[m][reg] + b0, 0.0f);
    }
}

// One network over the workgroup's rows.  x0: the input rows (K = 32 layout, stride kPolInStride); h1, h2: the activation
// buffers.  Every thread calls it: the first barrier waits for x0 and for the previous network's head.  Wave m < MT, lane
// (col e, rows 4 q + reg) receives out[reg] = head[16 m + 4 q + reg][e] + bias; the other waves' out is unspecified.
template <int MT>
__device__ __forceinline__ void wide_forward(const WideNet &N, const float *x0, float *h1, float *h2, int wave, int lane, float out[4])
{
    __syncthreads();
    wide_layer<2, kWideT1, kWideH1, MT>(N.w1p, N.b1, x0, kPolInStride, h1, kWideS1, wave, lane);
    __syncthreads();
    wide_layer<kWideG2, kWideT2, kWideH2Pad, MT>(N.w2p, N.b2, h1, kWideS1, h2, kWideS2, wave, lane);
    __syncthreads();
    if (wave >= MT) return;
    f32x4 acc[1];
    wide_tile<kWideGH, 1>(N.whp, h2 + wave * 16 * kWideS2, kWideS2, lane, acc);
    const float bh = N.bh[lane & 15];
#pragma unroll
    for (int reg = 0; reg < 4; reg++) out[reg] = acc[0][reg] + bh;
}

struct WideLds {
    float *x0, *h1, *h2, *eps;
};

__device__ __forceinline__ WideLds wide_lds(float *lds)
{
    WideLds L;
    L.x0 = lds;
    L.h1 = L.x0 + kWideRows * kPolInStride;
    L.h2 = L.h1 + kWideRows * kWideS1;
    L.eps = L.h2 + kWideRows * kWideS2;
    return L;
}

// rows row0 .. row0 + R - 1 of in[n][18] into x0 (zero past column 17 and past row n)
__device__ __forceinline__ void wide_stage(float *x0, const float *__restrict__ in, int n, int row0, int t)
{
    for (int i = t; i < kWideRows * kPolInPad; i += 64 * kWideWaves) {
        const int e = i >> 5, k = i & 31, r = row0 + e;
        x0[e * kPolInStride + (k & 3) * (kPolInPad / 4) + (k >> 2)] = (k < 18 && r < n) ? in[(size_t)r * 18 + k] : 0.0f;
    }
}

// PolicyArgs as k_policy_forward's deterministic kind reads them; aux: sigma, low, high at 0, 3, 6
__global__ void __launch_bounds__(64 * kWideWaves)
k_wide_policy(WideNet N, const float *__restrict__ aux, PolicyArgs A)
{
    extern __shared__ __attribute__((aligned(16))) float wide_smem[];
    const WideLds L = wide_lds(wide_smem);
    const int t = threadIdx.x, env0 = blockIdx.x * kWideRows;
    const int lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const bool noisy = A.noise || A.sample;
    if (noisy) {
        for (int i = t; i < kWideRows * 3; i += 64 * kWideWaves) {
            const int row = i / 3, c = i - 3 * row, env = env0 + row;
            float eps = 0.0f;
            if (env < A.n) eps = A.sample ? philox_normal<0u>(A.seed, A.counter, (uint32_t)env, c) : A.noise[(size_t)env * 3 + c];
            L.eps[row * 4 + c] = eps;
        }
    }
    wide_stage(L.x0, A.obs, A.n, env0, t);
    float head[4];
    wide_forward<kWideMT>(N, L.x0, L.h1, L.h2, wave, lane, head);
    const int e = lane & 15, q = lane >> 4;
    if (wave >= kWideMT || e >= 3) return;
    const float sigma = aux[e], low = aux[3 + e], high = aux[6 + e];
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
        const int row = 16 * wave + 4 * q + reg, env = env0 + row;
        if (env >= A.n) continue;
        const float eps = noisy ? L.eps[row * 4 + e] : 0.0f;
        float s = tanhf(head[reg]);
        if (noisy) s = fminf(fmaxf(s + sigma * eps, -1.0f), 1.0f);
        if (A.actions) A.actions[(size_t)env * 3 + e] = unscale_action(s, low, high);
        if (A.buffer_actions) A.buffer_actions[(size_t)env * 3 + e] = s;
        if (A.eps_out && noisy) A.eps_out[(size_t)env * 3 + e] = eps;
    }
}

// TargetArgs as k_td_target<kTargetTD3> reads them (next_log_prob and q2 are refused by the host)
struct WideTargetArgs {
    int n;
    const float *next_obs, *rewards, *dones, *noise;
    int sample;
    uint64_t seed, counter;
    float gamma, policy_noise, noise_clip;
    float *target, *next_actions, *q1, *eps_out;
};

__global__ void __launch_bounds__(64 * kWideWaves)
k_wide_target(WideNet actor, WideNet critic, WideTargetArgs A)
{
    extern __shared__ __attribute__((aligned(16))) float wide_smem[];
    const WideLds L = wide_lds(wide_smem);
    const int t = threadIdx.x, row0 = blockIdx.x * kWideRows;
    const int lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const bool noisy = A.noise || A.sample;
    for (int i = t; i < kWideRows * 3; i += 64 * kWideWaves) {
        const int row = i / 3, c = i - 3 * row, r = row0 + row;
        float eps = 0.0f;
        if (noisy && r < A.n) eps = A.sample ? philox_normal<2u>(A.seed, A.counter, (uint32_t)r, c) : A.noise[(size_t)r * 3 + c];
        L.eps[row * 4 + c] = eps;
    }
    // next observations -> x0; columns 18..20 receive the action below, the rest is zero
    wide_stage(L.x0, A.next_obs, A.n, row0, t);
    const int e = lane & 15, q = lane >> 4;
    float head[4];
    wide_forward<kWideMT>(actor, L.x0, L.h1, L.h2, wave, lane, head);
    if (wave < kWideMT && e < 3) {   // every wave is past layer 1: x0 is free to take the action
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int row = 16 * wave + 4 * q + reg, r = row0 + row;
            const float eps = L.eps[row * 4 + e];
            const float nz = fminf(fmaxf(A.policy_noise * eps, -A.noise_clip), A.noise_clip);
            const float a = fminf(fmaxf(tanhf(head[reg]) + nz, -1.0f), 1.0f);
            const int k = 18 + e;
            L.x0[row * kPolInStride + (k & 3) * (kPolInPad / 4) + (k >> 2)] = r < A.n ? a : 0.0f;
            if (r >= A.n) continue;
            if (A.next_actions) A.next_actions[(size_t)r * 3 + e] = a;
            if (A.eps_out) A.eps_out[(size_t)r * 3 + e] = eps;
        }
    }
    if (!A.target && !A.q1) return;   // (uniform: no barrier is left waiting)
    float qv[4];
    wide_forward<kWideMT>(critic, L.x0, L.h1, L.h2, wave, lane, qv);
    if (wave >= kWideMT || e != 0) return;
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
        const int r = row0 + 16 * wave + 4 * q + reg;
        if (r >= A.n) continue;
        if (A.q1) A.q1[r] = qv[reg];
        if (A.target) A.target[r] = A.rewards[r] + ((1.0f - A.dones[r]) * A.gamma) * qv[reg];
    }
}

}  // namespace meshenv
