// meshenv_td3_actor_grad.h -- the actor loss of TD3 / DDPG and its gradients (SB3 2.x's TD3.train, the statements that run
// every policy_delay steps:
//
//   actor_loss = -self.critic.q1_forward(replay_data.observations, self.actor(replay_data.observations)).mean()
//   self.actor.optimizer.zero_grad(); actor_loss.backward()
//
// for the networks the reference trains: rl/baselines/RL_Mesh.py:206-222, actor ReLU [256, 256] with a Linear(256, 3) + Tanh
// head on 18 observations, critic q_networks[0] ReLU [256, 256] on cat(obs, action) = 21).  Two launches: k_td3_actor_grad
// writes one partial gradient set per workgroup, k_td3_actor_grad_reduce sums the sets in index order into the gradient
// buffer (torch's [out][in] / [out] layout) and finishes the loss.  The critic is only differentiated with respect to the
// action: its parameters receive no gradient.
//
// k_td3_actor_grad.  The tiling of k_critic_grad<TD3>: 16 samples per tile, 1024 threads, wave w owning neurons [16 w,
// 16 w + 16) of every hidden layer, v_mfma_f32_16x16x4_f32 throughout, weights read from the LIVE torch tensors, activations
// in LDS with row stride H + 4.  blockIdx.x is the workgroup of a tile set (it walks the tiles blockIdx.x, blockIdx.x + nwg,
// ... with its accumulators in registers), blockIdx.y the half: dW_2 is 65 536 floats, 64 accumulator registers per lane, so
// as in k_critic_grad<TD3> (kCgSplitTD3) two workgroups per tile set each do the whole forward and critic pass and accumulate
// half the columns of dW_2; half 0 writes everything else.  Per tile:
//
//   actor     a_l = relu(W_l a_{l-1} + b_l), l = 1, 2, both kept in LDS; a_0 = cg_stage's input row (18
//             observations, columns 18..20 for the action, a_0[21] = 1; the actor's weights of columns >= 18 are read as 0)
//   head      wave 0, one 16-wide tile of which columns 0..2 are used: pre = W_3 a_2 + b_3, a = tanhf(pre) (k_td_target<TD3>'s
//             call); a goes into columns 18..20 of the input row, 0 for rows past B
//   critic    c_1 = relu(W^q_1 a_0 + b^q_1), c_2 likewise, THROUGH ONE LDS BUFFER: a lane computes the same (row, neuron)
//             elements of c_1, c_2, dz_2 and dz_1, so c_2 is formed in registers and written over c_1 once every wave has
//             read it, and the sign of c_1 stays in a register as the mask of dz_1.  q = w^q_out c_2 + b^q_out on wave 0.
//             Backward from dq = 1: dz_2 = c_2 > 0 ? w^q_out : 0, dz_1 = c_1 > 0 ? dz_2 W^q_2 : 0, and on wave 0
//             dQ/da = dz_1 W^q_1[:, 18..20].  No weight gradient.
//   head grad wave 0: d_pre = (-((dQ/da) / B)) * (1 - a a), autograd's order (tanh's backward is grad * (1 - out * out));
//             exactly 0 for rows past B
//   actor     backward from a head gradient through cg_da of meshenv_grad_tile.h, the head being 3 wide: thread t < 768 owns
//             dW_3[t / 256][t % 256] += d_pre[row][i] a_2[row][n] (fmaf, rows in order), threads 768..770 db_3 (plain adds),
//             thread 771 the sum of q; dz_2 = a_2 > 0 ? sum_i d_pre[i] W_3[i][n] : 0 (one product and two fmaf, i in order);
//             then dW_2 (this half's columns), db_2, da_1 = dz_2 W_2, dz_1 = a_1 > 0 ? da_1 : 0, dW_1, db_1.
//
// Reduction order of a gradient element and of the sum of q (tests/td3_actor_grad_ref.py derives its bounds from it): one
// fma / add chain over the rows of the workgroup's tiles, 16 T roundings for T = ceil(tiles / nwg), then nwg - 1 additions
// over the partial sets in index order; nwg as in meshenv_critic_grad.h.  actor_loss = -(S / B).  No floating-point
// atomics: two calls on the same inputs give the same bits.
#pragma once

#include "meshenv_critic_grad.h"

namespace meshenv {

constexpr int kTaObs = kCgObs; // actor inputs
constexpr int kTaParts = 4;    // optional per-sample outputs: actions q1 dq_da d_pre

// The gradient set, torch layout, in TD3ActorGradSpec's parameter order: w1 [H][18], b1 [H], w2 [H][H], b2 [H], w3 [3][H],
// b3 [3]; padded to a multiple of 64 floats.  A partial set carries the sum of q after it.
struct TaLayout {
    static constexpr int H = 256;
    static constexpr int b1 = H * kTaObs;
    static constexpr int w2 = b1 + H;
    static constexpr int b2 = w2 + H * H;
    static constexpr int w3 = b2 + H;
    static constexpr int b3 = w3 + 3 * H;
    static constexpr int params = b3 + 3;
    static constexpr int stride = (params + 63) & ~63;
    static constexpr int set = stride + 64;
};

struct TaArgs {
    int n, nwg;
    const float *obs;              // [n][18]
    const float *w[3], *b[3];      // the actor: two hidden layers and the head (torch layout)
    CgCritic c;                    // the first critic: w[0..1] hidden, w[2] the output layer
    float *partial;                // [nwg][TaLayout::set]
    float *actions, *q, *dq_da, *d_pre;   // [n][3] [n] [n][3] [n][3], every one nullable
    float *acts[2][2];             // [actor, critic][layer]: [n][H] post-ReLU activations, nullable
};

__global__ void __launch_bounds__(1024)
k_td3_actor_grad(TaArgs A)
{
    constexpr int H = TaLayout::H, G = H / 16, S = H + 4, NT = 1024;
    constexpr int GH = G / kCgSplitTD3;   // input tiles of dW_2 per workgroup
    using L = TaLayout;
    __shared__ __attribute__((aligned(16))) float x0[kCgRows * kCgInStride];
    __shared__ __attribute__((aligned(16))) float aa[2][kCgRows * S];   // the actor's activations, then its dz
    __shared__ __attribute__((aligned(16))) float ca[kCgRows * S];      // the critic: c_1, c_2, dz_2, dz_1 in turn
    __shared__ float s_a[kCgRows * 4], dh[kCgRows * 4];                 // a and d_pre, columns 0..2
    __shared__ float s_q[kCgRows];
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);   // the lane's own indices: per tile, below
    const int half = blockIdx.y;
    const bool first = half == 0;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 dw1[2] = {zero, zero};
    f32x4 dw2[GH], db2 = zero;
#pragma unroll
    for (int kt = 0; kt < GH; kt++) dw2[kt] = zero;
    float hacc = 0.0f;   // t < 768: dW_3[t / H][t % H]; 768..770: db_3; 771: the sum of q
    const int tiles = (A.n + kCgRows - 1) / kCgRows;
    const float fn = (float)A.n;

    for (int tile = blockIdx.x; tile < tiles; tile += A.nwg) {
        const int row0 = tile * kCgRows;
        // The lane's indices are formed in every tile, behind a barrier the optimiser cannot see through: hoisted out of
        // the loop, the addresses derived from them (some fifty registers) would be live across it next to the
        // accumulators and spill.  This rests on how the optimiser hoists today: after a compiler upgrade run
        // tools/resource_usage.sh again (profiles/td3_actor_grad_resource_usage.txt: 104 VGPRs, no scratch).
        int tt = threadIdx.x;
        asm volatile("" : "+v"(tt));
        const int t = tt, lane = t & 63, e = lane & 15, q = lane >> 4, n0 = 16 * wave + e;
        cg_stage<NT, false>(x0, A.obs, nullptr, row0, A.n, t);
        __syncthreads();
        // ---- actor forward and its head (wave 0)
        {
            f32x4 v = cg_first_layer<kTaObs, kPolicyReLU>(A.w[0], A.b[0], x0, e, q, n0);
            cg_store<H>(aa[0], first ? A.acts[0][0] : nullptr, v, row0, A.n, q, n0);
            __syncthreads();
            v = cg_hidden_layer<H, kPolicyReLU>(A.w[1], A.b[1], aa[0], e, q, n0);
            cg_store<H>(aa[1], first ? A.acts[0][1] : nullptr, v, row0, A.n, q, n0);
            __syncthreads();
        }
        if (wave == 0) {
            f32x4 acc0 = zero, acc1 = zero;
            const int hr = e < 3 ? e : 0;
            cg_dense<G>(A.w[2], (unsigned)(hr * H + 4 * q), e < 3, aa[1] + e * S + 4 * q, acc0, acc1);
            if (e < 3) {
                const float bh = A.b[2][hr];
#pragma unroll
                for (int reg = 0; reg < 4; reg++) {
                    const int row = 4 * q + reg, r = row0 + row;
                    const bool in = r < A.n;
                    const float a = in ? tanhf((acc0[reg] + acc1[reg]) + bh) : 0.0f;
                    x0[row * kCgInStride + kTaObs + e] = a;
                    s_a[row * 4 + e] = a;
                    if (in && first && A.actions) A.actions[(unsigned)(r * 3 + e)] = a;
                }
            }
        }
        __syncthreads();
        // ---- the critic through one buffer: forward, q, then dQ/da from dq = 1
        {
            f32x4 v = cg_first_layer<kTgtIn, kPolicyReLU>(A.c.w[0], A.c.b[0], x0, e, q, n0);
            bool m1[4];
#pragma unroll
            for (int reg = 0; reg < 4; reg++) m1[reg] = v[reg] > 0.0f;
            cg_store<H>(ca, first ? A.acts[1][0] : nullptr, v, row0, A.n, q, n0);
            __syncthreads();
            v = cg_hidden_layer<H, kPolicyReLU>(A.c.w[1], A.c.b[1], ca, e, q, n0);
            const float wo = A.c.w[2][(unsigned)n0];
            __syncthreads();   // every wave has read c_1
            cg_store<H>(ca, first ? A.acts[1][1] : nullptr, v, row0, A.n, q, n0);
            __syncthreads();
            if (wave == 0) {
                f32x4 acc0 = zero, acc1 = zero;
                cg_dense<G>(A.c.w[2], (unsigned)(4 * q), e == 0, ca + e * S + 4 * q, acc0, acc1);
                if (e == 0) {
                    const float bh = A.c.b[2][0];
#pragma unroll
                    for (int reg = 0; reg < 4; reg++) {
                        const int row = 4 * q + reg, gr = row0 + row;
                        const float qv = (acc0[reg] + acc1[reg]) + bh;
                        s_q[row] = gr < A.n ? qv : 0.0f;
                        if (gr < A.n && first && A.q) A.q[(unsigned)gr] = qv;
                    }
                }
            }
            __syncthreads();   // wave 0 has read c_2
#pragma unroll
            for (int reg = 0; reg < 4; reg++) ca[(4 * q + reg) * S + n0] = v[reg] > 0.0f ? wo : 0.0f;   // dz_2
            __syncthreads();
            const f32x4 da = cg_da<H>(A.c.w[1], ca, e, q, n0);
            __syncthreads();   // every wave has read dz_2
#pragma unroll
            for (int reg = 0; reg < 4; reg++) ca[(4 * q + reg) * S + n0] = m1[reg] ? da[reg] : 0.0f;    // dz_1
            __syncthreads();
        }
        if (wave == 0) {   // dQ/da[row][k] = sum_n dz_1[row][n] W^q_1[n][18 + k], then the head gradient
            f32x4 acc0 = zero, acc1 = zero;
            const float *xr = ca + e * S + 4 * q;
            // buffer loads as in cg_da: lanes e >= 3 read column 18 and drop it
            const __amdgpu_buffer_rsrc_t w1 = __builtin_amdgcn_make_buffer_rsrc((void *)A.c.w[0], 0, H * kTgtIn * 4, kCgBufferFlags);
            const int voff = (4 * q * kTgtIn + kTaObs + (e < 3 ? e : 0)) * 4;
#pragma unroll
            for (int g = 0; g < G; g += 2) {
                const f32x4 a0 = *reinterpret_cast<const f32x4 *>(xr + 16 * g);
                const f32x4 a1 = *reinterpret_cast<const f32x4 *>(xr + 16 * g + 16);
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const float l0 = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(w1, voff, (16 * g + j) * kTgtIn * 4, 0));
                    const float l1 = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(w1, voff, (16 * g + 16 + j) * kTgtIn * 4, 0));
                    const float b0 = e < 3 ? l0 : 0.0f, b1 = e < 3 ? l1 : 0.0f;
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[j], b0, acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[j], b1, acc1, 0, 0, 0);
                }
            }
            if (e < 3) {
#pragma unroll
                for (int reg = 0; reg < 4; reg++) {
                    const int row = 4 * q + reg, r = row0 + row;
                    const bool in = r < A.n;
                    const float dq = acc0[reg] + acc1[reg];
                    const float a = s_a[row * 4 + e];
                    const float d = in ? (-(dq / fn)) * (1.0f - a * a) : 0.0f;
                    dh[row * 4 + e] = d;
                    if (in && first) {
                        if (A.dq_da) A.dq_da[(unsigned)(r * 3 + e)] = dq;
                        if (A.d_pre) A.d_pre[(unsigned)(r * 3 + e)] = d;
                    }
                }
            }
        }
        __syncthreads();
        // ---- head weight and bias gradients from a_2, the sum of q
        if (t < 3 * H) {
            const int i = t >> 8, n = t & (H - 1);
#pragma unroll
            for (int row = 0; row < kCgRows; row++) hacc = fmaf(dh[row * 4 + i], aa[1][row * S + n], hacc);
        } else if (t < 3 * H + 3) {
#pragma unroll
            for (int row = 0; row < kCgRows; row++) hacc = hacc + dh[row * 4 + (t - 3 * H)];
        } else if (t == 3 * H + 3) {
#pragma unroll
            for (int row = 0; row < kCgRows; row++) hacc = hacc + s_q[row];
        }
        __syncthreads();   // every thread has read a_2
        {   // dz_2 = a_2 > 0 ? sum_i d_pre[i] W_3[i][n] : 0 over a_2
            const int n = t & (H - 1), r4 = 4 * (t >> 8);
            float w3[3];
#pragma unroll
            for (int i = 0; i < 3; i++) w3[i] = A.w[2][(unsigned)(i * H + n)];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float *d = dh + (r4 + r) * 4;
                float v = d[0] * w3[0];
                v = fmaf(d[1], w3[1], v);
                v = fmaf(d[2], w3[2], v);
                float *p = aa[1] + (r4 + r) * S + n;
                *p = *p > 0.0f ? v : 0.0f;
            }
        }
        __syncthreads();
        // ---- layer 2: dW_2 (this half's columns), db_2, da_1
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const int row = 4 * q + s;
            const float a = aa[1][row * S + n0];   // A[i = e][k = q]: dz_2[row][n]
#pragma unroll
            for (int kt = 0; kt < GH; kt++)
                dw2[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, aa[0][row * S + 16 * (half * GH + kt) + e], dw2[kt], 0, 0, 0);
            db2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, 1.0f, db2, 0, 0, 0);
        }
        {
            const f32x4 da = cg_da<H>(A.w[1], aa[1], e, q, n0);
            __syncthreads();   // every wave has read a_1 (dW_2) and dz_2
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                float *p = aa[0] + (4 * q + reg) * S + n0;
                *p = *p > 0.0f ? da[reg] : 0.0f;
            }
        }
        __syncthreads();
        // ---- layer 1: dW_1 and, against the column of ones, db_1
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const int row = 4 * q + s;
            const float a = aa[0][row * S + n0];
#pragma unroll
            for (int kt = 0; kt < 2; kt++)
                dw1[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, x0[row * kCgInStride + 16 * kt + e], dw1[kt], 0, 0, 0);
        }
        __syncthreads();   // x0, aa, ca, dh and s_q are free for the next tile
    }

    const int t = threadIdx.x, e = t & 15, q = (t & 63) >> 4;
    // ---- the workgroup's partial set, torch layout; D[i = 4 q + reg][j = e]: neuron 16 wave + 4 q + reg, input 16 kt + e
    float *P = A.partial + (size_t)blockIdx.x * L::set;
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
        const int n = 16 * wave + 4 * q + reg;
#pragma unroll
        for (int kt = 0; kt < GH; kt++) P[L::w2 + n * H + 16 * (half * GH + kt) + e] = dw2[kt][reg];
        if (!first) continue;
        if (e == 0) P[L::b2 + n] = db2[reg];
        cg_put_dw1<kTaObs>(P, L::b1, dw1, reg, n, e);
    }
    if (!first) return;   // everything but its columns of dW_2 is the first workgroup's to write
    if (t < 3 * H + 3) P[L::w3 + t] = hacc;   // w3 [3][H] and b3 [3] are adjacent
    else if (t == 3 * H + 3) P[L::stride] = hacc;
}

// grad[i] = partial[0][i] + partial[1][i] + ... in index order; with S the sums of q added the same way: actor_loss = -(S / B)
__global__ void __launch_bounds__(256)
k_td3_actor_grad_reduce(const float *__restrict__ partial, int nwg, int n, float *__restrict__ grad, float *__restrict__ loss)
{
    using L = TaLayout;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < L::params) {
        float s[1];
        cg_sum_sets<1, true>(partial, nwg, L::set, i, s);
        grad[i] = s[0];
    }
    if (i == 0) {
        float s[1];
        cg_sum_sets<1, false>(partial, nwg, L::set, L::stride, s);
        loss[0] = -(s[0] / (float)n);
    }
}

}  // namespace meshenv
