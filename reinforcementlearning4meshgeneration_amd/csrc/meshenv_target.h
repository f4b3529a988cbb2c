// meshenv_target.h -- the TD target of SAC and TD3 in one launch (the `with th.no_grad():` block of SB3 2.x's SAC.train /
// TD3.train that follows replay_buffer.sample, for the networks the reference trains: rl/baselines/RL_Mesh.py:179-222, SAC
// ReLU [128, 128, 128], TD3 ReLU [256, 256]).
//
//   SAC  mean, log_std = actor(next_obs), log_std clamped to [-20, 2]; g = mean + exp(log_std) * eps; a = tanh(g);
//        log_prob = sum_k Normal(mean_k, std_k).log_prob(g_k) - sum_k log(1 - a_k^2 + 1e-6)
//        q = min(Q1(next_obs ++ a), Q2(next_obs ++ a)) - ent_coef * log_prob
//   TD3  a = clamp(tanh(mu(next_obs)) + clamp(policy_noise * eps, -noise_clip, noise_clip), -1, 1)
//        q = min(Q1(next_obs ++ a), Q2(next_obs ++ a))
//   target = reward + (1 - done) * gamma * q          (float32, SB3's order of operations)
//
// k_td_target<KIND>.  The MFMA tiling of meshenv_policy.h (v_mfma_f32_16x16x4_f32: exact f32; 16 samples = MFMA M per
// workgroup; H / 16 wavefronts, wave w owning neurons [16 w, 16 w + 16) of every hidden layer; activations through LDS in
// the k-permuted layout, weights in the per-lane B-operand order).  The three networks run ONE AFTER THE OTHER in the same
// waves: actor, then Q1, then Q2.  The critics' input row is the actor's input row with the action written into columns
// 18..20 (cat(obs, action), 21 inputs padded to 32), so the observation is staged once.  Each tower requests its first two
// layers' weights before the barrier that ends the previous tower, so that they are in flight while wave 0 finishes the
// previous head; a third layer (SAC) is requested one layer ahead.  Wave 0 runs every head (one 16-wide tile: columns
// mu0..2, log_std0..2 / mu0..2 / q) and keeps log_prob, q1 and q2 of its rows in registers until the final elementwise step.
//
// eps: an explicit [B][3] input, 0 (neither given), or Philox4x32-10 keyed by seed at counter words (sample index, counter
// lo, counter hi, 2).  Tag 2 is this kernel's own: the rollout noise (meshenv_actor.h) uses 0, the replay draw
// (meshenv_replay.h) 1, so the same (seed, counter) given to all three does not reuse a stream.
//
// k_target_pack (meshenv_pack.h): the weights come from LIVE device tensors in torch.nn.Linear layout.  One launch copies all
// of them (and log_ent_coef) into the handle's buffer in the kernel's layout.
#pragma once

#include "meshenv_pack.h"
#include "meshenv_policy.h"

namespace meshenv {

enum { kTargetSAC = 0, kTargetTD3 = 1, kTargetDDPG = 2 };   // DDPG: k_wide_target, meshenv_wide.h

constexpr int kTgtRows = 16;      // samples per workgroup = MFMA M
constexpr int kTgtIn = 21;        // critic inputs: 18 observations ++ 3 actions (padded to kPolInPad = 32)
constexpr uint32_t kTgtPhiloxTag = 2u;

struct TargetTower {
    const float *w1p, *b1;  // [H/16][2][64][4], [H]
    const float *w2p, *b2;  // [H/16][H/16][64][4], [H]
    const float *w3p, *b3;  // SAC only
    const float *whp, *bh;  // head tile [H/16][64][4], [16]
};

struct TargetWeights {
    TargetTower actor, q1, q2;
    const float *log_ent_coef;   // the packed copy of SAC's learned log_ent_coef, or nullptr (fixed ent_coef)
};

struct TargetArgs {
    int n;
    const float *next_obs;       // [n][18]
    const float *rewards, *dones;  // [n] (required with target)
    const float *noise;          // [n][3] or nullptr
    int sample;                  // in-kernel Philox noise
    uint64_t seed, counter;
    float gamma, ent_coef, policy_noise, noise_clip;
    float *target, *next_actions, *next_log_prob, *q1, *q2, *eps_out;   // every one nullable
};

// One network over the workgroup's 16 rows: NL ReLU layers of width H, then the head tile on wave 0, whose lane (col e, rows
// 4 q + reg) receives out[reg] = head[row][e] + bias (other waves: unspecified).  x0: the input rows (K = 32 layout, stride
// kPolInStride); ha, hb: activation buffers of stride H + 4.  Every thread calls it: the first barrier waits for x0 and for
// the previous tower's head.
template <int H, int NL>
__device__ __forceinline__ void target_tower(const TargetTower &T, const float *x0, float *ha, float *hb, int wave, int lane,
                                             float out[4])
{
    constexpr int G = H / 16;
    constexpr bool kHeadAhead = H <= 128;
    LayerRegs<2> r1;
    LayerRegs<G> r2, r3, wh;
    load_layer<2>(r1, T.w1p, wave, lane);
    load_layer<G>(r2, T.w2p, wave, lane);
    __syncthreads();
    policy_layer<2, H, kPolicyReLU>(r1, T.b1, x0, kPolInStride, ha, wave, lane);
    if (NL == 3) load_layer<G>(r3, T.w3p, wave, lane);
    else if (kHeadAhead && wave == 0) load_layer<G>(wh, T.whp, 0, lane);
    __syncthreads();
    policy_layer<G, H, kPolicyReLU>(r2, T.b2, ha, H + 4, hb, wave, lane);
    if ((NL == 3 || !kHeadAhead) && wave == 0) load_layer<G>(wh, T.whp, 0, lane);
    __syncthreads();
    const float *last = hb;
    if (NL == 3) {
        policy_layer<G, H, kPolicyReLU>(r3, T.b3, hb, H + 4, ha, wave, lane);
        __syncthreads();
        last = ha;
    }
    if (wave != 0) return;
    const int e = lane & 15, q = lane >> 4;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    const float *xr = last + e * (H + 4) + q * (4 * G);
#pragma unroll
    for (int g = 0; g < G; g += 2) {
        const f32x4 a0 = *reinterpret_cast<const f32x4 *>(xr + 4 * g);
        const f32x4 a1 = *reinterpret_cast<const f32x4 *>(xr + 4 * g + 4);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[j], wh.w[g][j], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[j], wh.w[g + 1][j], acc1, 0, 0, 0);
        }
    }
    const float bh = T.bh[e];
#pragma unroll
    for (int reg = 0; reg < 4; reg++) out[reg] = (acc0[reg] + acc1[reg]) + bh;
}

template <int KIND>
__global__ void __launch_bounds__(KIND == kTargetSAC ? 512 : 1024)
k_td_target(TargetWeights W, TargetArgs A)
{
    constexpr int H = KIND == kTargetSAC ? 128 : 256, NL = KIND == kTargetSAC ? 3 : 2;
    __shared__ __attribute__((aligned(16))) float x0[kTgtRows * kPolInStride];
    __shared__ __attribute__((aligned(16))) float ha[kTgtRows * (H + 4)];
    __shared__ __attribute__((aligned(16))) float hb[kTgtRows * (H + 4)];
    __shared__ __attribute__((aligned(16))) float eps_lds[kTgtRows * 4];
    const int t = threadIdx.x, row0 = blockIdx.x * kTgtRows;
    const int lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const bool noisy = A.noise || A.sample;
    if (t < kTgtRows * 3) {
        const int row = t / 3, c = t - 3 * row, r = row0 + row;
        float eps = 0.0f;
        if (noisy && r < A.n) eps = A.sample ? philox_normal<kTgtPhiloxTag>(A.seed, A.counter, (uint32_t)r, c) : A.noise[(size_t)r * 3 + c];
        eps_lds[row * 4 + c] = eps;
    }
    // next observations -> x0 in the K = 32 layout; columns 18..20 receive the action below, the rest is zero
    for (int i = t; i < kTgtRows * kPolInPad; i += 64 * (H / 16)) {
        const int e = i >> 5, k = i & 31, r = row0 + e;
        const float v = (k < 18 && r < A.n) ? A.next_obs[(size_t)r * 18 + k] : 0.0f;
        x0[e * kPolInStride + (k & 3) * (kPolInPad / 4) + (k >> 2)] = v;
    }
    const int e = lane & 15, q = lane >> 4;
    float head[4], lp[4] = {0.f, 0.f, 0.f, 0.f};
    target_tower<H, NL>(W.actor, x0, ha, hb, wave, lane, head);
    if (wave == 0) {
        const int c = e < 3 ? e : 0;
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int row = 4 * q + reg, r = row0 + row;
            const float mean = head[reg];
            const float eps = eps_lds[row * 4 + c];
            float a;
            if (KIND == kTargetSAC) {
                const float ls_raw = __shfl(mean, lane + 3, 64);   // column 3 + a holds log_std_a
                const float ls = fminf(fmaxf(ls_raw, -20.0f), 2.0f);
                const float std = expf(ls);
                const float g = mean + std * eps;
                a = tanhf(g);
                const float d = g - mean;       // torch.distributions.Normal.log_prob
                const float lpc = -(d * d) / (2.0f * (std * std)) - logf(std) - 0.91893853320467274f;
                const float sq = logf((1.0f - a * a) + 1e-6f);   // SquashedDiagGaussianDistribution, epsilon 1e-6
                const float lpc1 = __shfl(lpc, lane + 1, 64), lpc2 = __shfl(lpc, lane + 2, 64);
                const float sq1 = __shfl(sq, lane + 1, 64), sq2 = __shfl(sq, lane + 2, 64);
                lp[reg] = ((lpc + lpc1) + lpc2) - ((sq + sq1) + sq2);
                if (e == 0 && r < A.n && A.next_log_prob) A.next_log_prob[r] = lp[reg];
            } else {
                const float nz = fminf(fmaxf(A.policy_noise * eps, -A.noise_clip), A.noise_clip);
                a = fminf(fmaxf(tanhf(mean) + nz, -1.0f), 1.0f);
            }
            if (e >= 3) continue;
            const int k = 18 + e;
            x0[row * kPolInStride + (k & 3) * (kPolInPad / 4) + (k >> 2)] = r < A.n ? a : 0.0f;
            if (r >= A.n) continue;
            if (A.next_actions) A.next_actions[(size_t)r * 3 + e] = a;
            if (A.eps_out) A.eps_out[(size_t)r * 3 + e] = eps;
        }
    }
    float qa[4], qb[4];
    target_tower<H, NL>(W.q1, x0, ha, hb, wave, lane, qa);
    target_tower<H, NL>(W.q2, x0, ha, hb, wave, lane, qb);
    if (wave != 0 || e != 0) return;
    float ent = 0.0f;
    if (KIND == kTargetSAC) ent = W.log_ent_coef ? expf(W.log_ent_coef[0]) : A.ent_coef;
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
        const int r = row0 + 4 * q + reg;
        if (r >= A.n) continue;
        if (A.q1) A.q1[r] = qa[reg];
        if (A.q2) A.q2[r] = qb[reg];
        if (!A.target) continue;
        float nq = fminf(qa[reg], qb[reg]);
        if (KIND == kTargetSAC) nq = nq - ent * lp[reg];
        A.target[r] = A.rewards[r] + ((1.0f - A.dones[r]) * A.gamma) * nq;
    }
}

}  // namespace meshenv
