// meshenv_policy.h -- fused forward of the PPO / A2C / TD3 / DDPG-style MLP policies (the rollout side of the on-policy
// and deterministic-actor algorithms the reference trains with, rl/baselines/RL_Mesh.py:113-228).
//
// One kernel, k_policy_forward<H, ACT, KIND>, for a two-hidden-layer MLP of width H (64, 128 or 256) with ReLU or Tanh:
//   KIND = kPolicyActorCritic   (SB3 ActorCriticPolicy: PPO, A2C) a pi tower and a vf tower on the same observation;
//        mean = action_net(latent_pi), std = exp(log_std), buffer_action = mean + std * eps,
//        action = clamp(buffer_action, low, high), log_prob = sum_k Normal(mean_k, std_k).log_prob(buffer_action_k),
//        value = value_net(latent_vf)
//   KIND = kPolicyDeterministic (SB3 TD3Policy / DDPG: actor.mu) one tower; scaled = tanh(mu(latent)),
//        with noise scaled = clamp(scaled + sigma * eps, -1, 1) (NormalActionNoise); buffer_action = scaled,
//        action = low + 0.5 * (scaled + 1) * (high - low)
// eps is an explicit [n][3] input, the in-kernel Philox normal of meshenv_actor.h (same (seed, counter, env) keying as the
// SAC actor), or 0 (deterministic).
//
// Layout.  Same MFMA tiling as meshenv_actor.h (v_mfma_f32_16x16x4_f32: exact f32, 16 environments = MFMA M per
// workgroup), but a tower per WORKGROUP: blockIdx.y selects the tower (0 = pi / actor, 1 = vf), and a workgroup has H / 16
// wavefronts, wave w owning neurons [16 w, 16 w + 16) of both hidden layers as one 16x16 output tile.  The two towers of an
// actor-critic policy thus run side by side in one launch without sharing registers: at H = 256 a wave holds its 64-float
// layer-2 slice plus the 8-float layer-1 slice, inside the 128 registers that four waves per SIMD allow.  Layer weights are
// packed on the host in the per-lane B-operand order ([tile][K/16][lane][4], element j of lane l in group g =
// W[n = 16 tile + (l & 15)][k = 4 (4 g + j) + (l >> 4)]) and requested before the first layer runs; the head tile (one
// 16-wide tile: columns mean0..2 or value) one layer ahead of its use where the registers allow (H <= 128), after layer 2
// otherwise.  Activations go through LDS in the k-permuted layout of meshenv_actor.h (position (k & 3) * (K / 4) + (k >> 2),
// row stride K + 4 floats: conflict-free ds_read_b128).
//
// Bootstrap pass (vf workgroups only, tdone != nullptr): tvalue[e] = V(tobs[e]) where tdone[e] && !tcomplete[e], else 0 --
// the value of a truncated episode's terminal observation.  A workgroup none of whose 16 envs needs it skips the pass.
// Value-only launches (tower0 = 1) start the grid at the vf tower.
#pragma once

#include "meshenv_actor.h"

namespace meshenv {

enum { kPolicyActorCritic = 0, kPolicyDeterministic = 1 };
enum { kPolicyReLU = 0, kPolicyTanh = 1 };

constexpr int kPolEnvs = 16;      // environments per workgroup = MFMA M
constexpr int kPolInPad = 32;     // layer-1 K: 18 observations padded to a multiple of 16
constexpr int kPolInStride = 36;  // LDS row stride of the input rows (36 mod 64 = 36: 16 rows x 16 B on distinct banks)

struct PolicyTower {
    const float *w1p, *b1;  // [H/16][2][64][4], [H]
    const float *w2p, *b2;  // [H/16][H/16][64][4], [H]
    const float *whp, *bh;  // head tile [H/16][64][4], [16]
};

struct PolicyWeights {
    PolicyTower pi, vf;     // vf unused by the deterministic kind
    const float *aux;       // [9]: log_std (actor-critic) or sigma (deterministic), low, high
};

struct PolicyArgs {
    int n;
    int tower0;             // tower of blockIdx.y == 0 (1: value-only launch)
    const float *obs;       // [n][18]
    const float *noise;     // [n][3] or nullptr
    int sample;             // in-kernel Philox noise keyed by (seed, counter, env)
    uint64_t seed, counter;
    float *actions, *buffer_actions, *log_prob, *value, *eps_out;   // every one nullable
    const float *tobs;      // bootstrap pass: [n][18] terminal observations
    const uint8_t *tdone, *tcomplete;
    float *tvalue;          // [n]
};

template <int ACT>
__device__ __forceinline__ float policy_act(float x)
{
    return ACT == kPolicyTanh ? tanhf(x) : fmaxf(x, 0.0f);
}

// y = act(W x + b) for the wave's 16 neurons; x: LDS rows of stride xs in the permuted layout of a 16 G-input layer,
// y: the permuted layout of the next (H-input) layer, row stride H + 4
template <int G, int H, int ACT>
__device__ __forceinline__ void policy_layer(const LayerRegs<G> &r, const float *__restrict__ bias, const float *x, int xs,
                                             float *y, int wave, int lane)
{
    const int e = lane & 15, q = lane >> 4;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    const float *xr = x + e * xs + q * (4 * G);
#pragma unroll
    for (int g = 0; g < G; g += 2) {
        const f32x4 a0 = *reinterpret_cast<const f32x4 *>(xr + 4 * g);
        const f32x4 a1 = *reinterpret_cast<const f32x4 *>(xr + 4 * g + 4);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[j], r.w[g][j], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[j], r.w[g + 1][j], acc1, 0, 0, 0);
        }
    }
    // D[row = 4 (lane >> 4) + reg][col = lane & 15]
    const int n0 = 16 * wave + e;
    const float b0 = bias[n0];
    const int p0 = (n0 & 3) * (H / 4) + (n0 >> 2);
#pragma unroll
    for (int reg = 0; reg < 4; reg++) y[(4 * q + reg) * (H + 4) + p0] = policy_act<ACT>((acc0[reg] + acc1[reg]) + b0);
}

// One pass of a tower over the 16 envs env0 .. env0 + 15 (every thread of the workgroup calls it: it contains barriers).
// boot: the bootstrap pass (rows of envs that need no terminal value are zero, outputs go to tvalue).
template <int H, int ACT, int KIND>
__device__ __forceinline__ void policy_pass(const PolicyTower &T, const float *__restrict__ aux, const PolicyArgs &A, int tower,
                                            bool boot, int env0, float *x0, float *h1, float *h2, float *eps_lds, int t)
{
    constexpr int G2 = H / 16;
    constexpr bool kHeadAhead = H <= 128;
    const int lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    LayerRegs<2> r1;
    LayerRegs<G2> r2;
    LayerRegs<G2> wh;
    load_layer<2>(r1, T.w1p, wave, lane);
    load_layer<G2>(r2, T.w2p, wave, lane);
    const float *in = boot ? A.tobs : A.obs;
    const bool noisy = !boot && tower == 0 && (A.noise || A.sample);
    if (noisy) {   // exploration noise, drawn while the weights are in flight
        for (int i = t; i < kPolEnvs * 3; i += 64 * G2) {
            const int row = i / 3, c = i - 3 * row, env = env0 + row;
            float eps = 0.0f;
            if (env < A.n) eps = A.sample ? philox_normal<0u>(A.seed, A.counter, (uint32_t)env, c) : A.noise[(size_t)env * 3 + c];
            eps_lds[row * 4 + c] = eps;
        }
    }
    for (int i = t; i < kPolEnvs * kPolInPad; i += 64 * G2) {
        const int e = i >> 5, k = i & 31, env = env0 + e;
        bool use = k < 18 && env < A.n;
        if (use && boot) use = A.tdone[env] && !A.tcomplete[env];
        x0[e * kPolInStride + (k & 3) * (kPolInPad / 4) + (k >> 2)] = use ? in[(size_t)env * 18 + k] : 0.0f;
    }
    __syncthreads();
    policy_layer<2, H, ACT>(r1, T.b1, x0, kPolInStride, h1, wave, lane);
    if (kHeadAhead && wave == 0) load_layer<G2>(wh, T.whp, 0, lane);
    __syncthreads();
    policy_layer<G2, H, ACT>(r2, T.b2, h1, H + 4, h2, wave, lane);
    if (!kHeadAhead && wave == 0) load_layer<G2>(wh, T.whp, 0, lane);
    __syncthreads();
    if (wave != 0) return;
    const int e = lane & 15, q = lane >> 4;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    const float *xr = h2 + e * (H + 4) + q * (4 * G2);
#pragma unroll
    for (int g = 0; g < G2; g += 2) {
        const f32x4 a0 = *reinterpret_cast<const f32x4 *>(xr + 4 * g);
        const f32x4 a1 = *reinterpret_cast<const f32x4 *>(xr + 4 * g + 4);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[j], wh.w[g][j], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[j], wh.w[g + 1][j], acc1, 0, 0, 0);
        }
    }
    const float bh = T.bh[e];
    const int c = e < 3 ? e : 0;
    if (tower == 1) {   // value head: column 0
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int env = env0 + 4 * q + reg;
            if (e != 0 || env >= A.n) continue;
            const float v = (acc0[reg] + acc1[reg]) + bh;
            if (!boot) {
                if (A.value) A.value[env] = v;
            } else if (A.tdone[env] && !A.tcomplete[env]) {
                A.tvalue[env] = v;
            }
        }
        return;
    }
    const float scale = aux[c], low = aux[3 + c], high = aux[6 + c];
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
        const int row = 4 * q + reg, env = env0 + row;
        const float mean = (acc0[reg] + acc1[reg]) + bh;
        const float eps = noisy && e < 3 ? eps_lds[row * 4 + c] : 0.0f;
        float ba, act, lp = 0.0f;
        if (KIND == kPolicyActorCritic) {
            const float std = expf(scale);   // torch: log_std.exp()
            ba = mean + std * eps;
            act = fminf(fmaxf(ba, low), high);
            const float d = ba - mean;       // torch.distributions.Normal.log_prob
            lp = -(d * d) / (2.0f * (std * std)) - logf(std) - 0.91893853320467274f;
        } else {
            float s = tanhf(mean);
            if (noisy) s = fminf(fmaxf(s + scale * eps, -1.0f), 1.0f);
            ba = s;
            act = unscale_action(s, low, high);
        }
        // sum over the three action components (lanes e, e + 1, e + 2 of the row), in torch's order
        const float lp1 = __shfl(lp, lane + 1, 64), lp2 = __shfl(lp, lane + 2, 64);
        if (e >= 3 || env >= A.n) continue;
        if (A.actions) A.actions[(size_t)env * 3 + e] = act;
        if (A.buffer_actions) A.buffer_actions[(size_t)env * 3 + e] = ba;
        if (A.eps_out && noisy) A.eps_out[(size_t)env * 3 + e] = eps;
        if (KIND == kPolicyActorCritic && e == 0 && A.log_prob) A.log_prob[env] = (lp + lp1) + lp2;
    }
}

template <int H, int ACT, int KIND>
__global__ void __launch_bounds__(64 * (H / 16))
k_policy_forward(PolicyWeights W, PolicyArgs A)
{
    __shared__ __attribute__((aligned(16))) float x0[kPolEnvs * kPolInStride];
    __shared__ __attribute__((aligned(16))) float h1[kPolEnvs * (H + 4)];
    __shared__ __attribute__((aligned(16))) float h2[kPolEnvs * (H + 4)];
    __shared__ __attribute__((aligned(16))) float eps_lds[kPolEnvs * 4];
    const int t = threadIdx.x, env0 = blockIdx.x * kPolEnvs;
    const int tower = KIND == kPolicyActorCritic ? (int)blockIdx.y + A.tower0 : 0;
    const PolicyTower T = tower == 0 ? W.pi : W.vf;
    policy_pass<H, ACT, KIND>(T, W.aux, A, tower, false, env0, x0, h1, h2, eps_lds, t);
    if (KIND != kPolicyActorCritic || tower != 1 || !A.tdone) return;
    // bootstrap pass: terminal values of the truncated episodes among the workgroup's envs
    __syncthreads();   // wave 0's head has read h2
    int need = 0;
    if (t < kPolEnvs && env0 + t < A.n) {
        const int env = env0 + t;
        need = A.tdone[env] && !A.tcomplete[env];
        if (!need) A.tvalue[env] = 0.0f;
    }
    if (__syncthreads_or(need)) policy_pass<H, ACT, KIND>(T, W.aux, A, 1, true, env0, x0, h1, h2, eps_lds, t);
}

}  // namespace meshenv
