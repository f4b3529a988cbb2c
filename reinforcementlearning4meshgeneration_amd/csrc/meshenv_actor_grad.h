// meshenv_actor_grad.h -- the actor loss and the entropy-coefficient loss of SAC and their gradients (SB3 2.x's SAC.train,
// the statements that follow the critic update:
//
//   actions_pi, log_prob = self.actor.action_log_prob(replay_data.observations)
//   ent_coef = th.exp(self.log_ent_coef.detach())
//   ent_coef_loss = -(self.log_ent_coef * (log_prob + self.target_entropy).detach()).mean()
//   q_values_pi = th.cat(self.critic(replay_data.observations, actions_pi), dim=1)
//   min_qf_pi, _ = th.min(q_values_pi, dim=1, keepdim=True)
//   actor_loss = (ent_coef * log_prob - min_qf_pi).mean()
//   self.actor.optimizer.zero_grad(); actor_loss.backward()
//
// for the networks the reference trains: rl/baselines/RL_Mesh.py:179-205, actor ReLU [128, 128, 128] with mu / log_std
// heads, twin critics ReLU [128, 128, 128] on cat(obs, action) = 21).  Two launches: k_actor_grad writes one partial
// gradient set per workgroup, k_actor_grad_reduce sums the sets in index order into the gradient buffer (torch's [out][in] /
// [out] layout) and finishes the two losses and log_ent_coef.grad.  The critics are only differentiated with respect to
// the action: their parameters receive no gradient (SB3 zeroes what autograd leaves there before the next critic step).
//
// k_actor_grad.  The tiling of meshenv_critic_grad.h: 16 samples per tile, 8 wavefronts, wave w owning neurons [16 w,
// 16 w + 16) of every hidden layer, v_mfma_f32_16x16x4_f32 throughout, weights read from the LIVE torch tensors, every
// activation in LDS with row stride H + 4.  Workgroup g walks the tiles g, g + nwg, ... with its accumulators in registers.
// Per tile:
//
//   actor     a_l = relu(W_l a_{l-1} + b_l), all three kept in LDS; a_0 = cg_stage's input row (18 observations,
//             columns 18..20 for the action, a_0[21] = 1; the actor's weights of columns >= 18 are read as 0)
//   heads     wave 0, one 16-wide tile: columns 0..2 mu, 3..5 log_std; then k_td_target<SAC>'s elementwise tail in SB3's
//             order: ls = clamp(raw, -20, 2); std = expf(ls); g = mu + std eps; a = tanhf(g); the Normal log-prob from
//             d = g - mu; log((1 - a a) + 1e-6f); a goes into columns 18..20 of the input row
//   critic c  (c = 1, 2, one after the other through the same three LDS buffers) forward, q_c on wave 0; backward from
//             dq = 1: dz_3 = a_3 > 0 ? w_out : 0, da_{l-1} = dz_l W_l masked by a_{l-1} > 0, and on wave 0
//             dQ_c/da = dz_1 W_1[:, 18..20].  No weight gradient.
//   select    wave 0: q1 <= q2 takes critic 1 (torch.min's choice on a tie).  With alpha = expf(log_ent_coef) (or the fixed
//             coefficient), s = 1 - a a, t = (2 a) s / (s + 1e-6f), dLa = -((dQ_sel/da) / B), se = std eps:
//                 d_mu      = (alpha / B) t + dLa s
//                 d_log_std = raw in [-20, 2] ? (alpha / B) (-1 + t se) + (dLa s) se : 0
//             the closed form of what autograd computes: the two eps^2 terms of the Normal log-prob (through g and through
//             the variance) cancel analytically and are not evaluated; what is left of it is -1 per component from
//             -log(std).  Rows past B get 0.  Loss terms alpha log_prob - min(q1, q2) and log_prob + target_entropy.
//   actor     backward from a head gradient through cg_da of meshenv_grad_tile.h, the head being 6 wide: dW_head += d_head^T a_3 (one
//             accumulator tile per wave, rows 6..15 zero) and db_head against a column of ones; dz_3 = a_3 > 0 ?
//             sum_i d_head[i] W_head[i][n] : 0 (one product and five fmaf, i in order); then dW_l, db_l, da_{l-1} for
//             l = 3, 2, 1.
//
// Reduction order of a gradient element and of the two loss sums (tests/actor_grad_ref.py derives its bounds from it): one
// fma / add chain over the rows of the workgroup's tiles, 16 T roundings for T = ceil(tiles / nwg), then nwg - 1 additions
// over the partial sets in index order; nwg as in meshenv_critic_grad.h.  No floating-point atomics: two calls on the same
// inputs give the same bits.
//
// eps: an explicit [B][3] input, 0 (neither given), or Philox4x32-10 keyed by seed at counter words (sample index, counter
// lo, counter hi, 3): tag 3 is this kernel's own (rollout noise 0, replay draw 1, TD target 2).
#pragma once

#include "meshenv_critic_grad.h"

namespace meshenv {

constexpr uint32_t kAgPhiloxTag = 3u;
constexpr int kAgObs = kCgObs;      // actor inputs
constexpr int kAgHeadStride = 16;   // LDS row stride of d_head (6 columns used, the rest stay 0)
constexpr int kAgParts = 7;         // optional per-sample outputs: actions log_prob q1 q2 dq_da d_mu d_log_std

// The gradient set, torch layout, in ActorGradSpec's parameter order: w1 [H][18], b1, w2 [H][H], b2, w3, b3, mu_w [3][H],
// mu_b [3], log_std_w [3][H], log_std_b [3], then log_ent_coef.grad [1]; padded to a multiple of 64 floats.  A partial set
// carries the two loss sums after it.
struct AgLayout {
    static constexpr int H = 128;
    static constexpr int b1 = H * kAgObs;
    static constexpr int hidden0 = b1 + H;
    static constexpr int hidden_stride = H * H + H;
    static constexpr int mu_w = hidden0 + 2 * hidden_stride;
    static constexpr int mu_b = mu_w + 3 * H;
    static constexpr int ls_w = mu_b + 3;
    static constexpr int ls_b = ls_w + 3 * H;
    static constexpr int ent = ls_b + 3;
    static constexpr int params = ent + 1;
    static constexpr int stride = (params + 63) & ~63;
    static constexpr int set = stride + 64;
    __host__ __device__ static constexpr int hw(int l) { return hidden0 + (l - 1) * hidden_stride; }   // l = 1, 2
    __host__ __device__ static constexpr int hb(int l) { return hw(l) + H * H; }
};

struct AgActor {
    const float *w[3], *b[3];                 // hidden layers (torch layout)
    const float *mu_w, *mu_b, *ls_w, *ls_b;   // [3][H], [3]
};

struct AgArgs {
    int n, nwg;
    const float *obs;            // [n][18]
    const float *noise;          // [n][3] or nullptr
    int sample;                  // in-kernel Philox noise
    uint64_t seed, counter;
    AgActor a;
    CgCritic c[2];
    const float *log_ent_coef;   // the live [1] tensor, or nullptr (fixed ent_coef)
    float ent_coef, target_entropy;
    float *partial;              // [nwg][AgLayout::set]
    float *actions, *log_prob, *q[2], *dq_da, *d_mu, *d_ls;   // [n][3] [n] [n] [n] [n][3] [n][3] [n][3], every one nullable
    float *eps_out;              // [n][3], nullable: the eps used
    float *acts[3][3];           // [actor, critic 1, critic 2][layer]: [n][H] post-ReLU activations, nullable
};

// Three ReLU layers over the tile's 16 rows: act[l] = relu(W_l act[l - 1] + b_l), act[-1] = x0 (KIN valid columns; the rest
// of W_1's K = 32 is read as 0).  Every thread calls it; x0 is complete at entry (a barrier has passed), act[2] at exit.
template <int KIN>
__device__ __forceinline__ void ag_forward(const float *const *w, const float *const *b, const float *x0, float (*act)[kCgRows * 132],
                                           float *const *out, int row0, int n, int e, int q, int n0)
{
    constexpr int H = 128, G = H / 16, S = H + 4;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int l = 0; l < 3; l++) {
        // the epilogue stays inline: through cg_bias_act / cg_store k_actor_grad's SGPR spill count changes (55 -> 53)
        f32x4 acc0 = zero, acc1 = zero;
        if (l == 0) cg_first<KIN>(w[0], x0, e, q, n0, acc0, acc1);
        else cg_dense<G>(w[l], (unsigned)(n0 * H + 4 * q), true, act[l - 1] + e * S + 4 * q, acc0, acc1);
        const float bias = b[l][(unsigned)n0];
        float *o = out[l];
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {   // D[row = 4 q + reg][col = e]
            const int row = 4 * q + reg;
            const float v = fmaxf((acc0[reg] + acc1[reg]) + bias, 0.0f);
            act[l][row * S + n0] = v;
            if (o && row0 + row < n) o[(unsigned)((row0 + row) * H + n0)] = v;
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(512)
k_actor_grad(AgArgs A)
{
    constexpr int H = 128, G = H / 16, S = H + 4, NT = 512;
    using L = AgLayout;
    __shared__ __attribute__((aligned(16))) float x0[kCgRows * kCgInStride];
    __shared__ __attribute__((aligned(16))) float aa[3][kCgRows * S];   // the actor's activations, then its dz
    __shared__ __attribute__((aligned(16))) float ca[3][kCgRows * S];   // one critic's activations, then its dz
    __shared__ float dh[kCgRows * kAgHeadStride];                       // d_head: columns 0..2 d_mu, 3..5 d_log_std
    __shared__ float eps_l[kCgRows * 4], s_a[kCgRows * 4], s_se[kCgRows * 4], s_mk[kCgRows * 4];
    __shared__ float dqa[2][kCgRows * 4];                               // dQ_c/da
    __shared__ float s_lp[kCgRows], s_q[2][kCgRows], l1[kCgRows], l2[kCgRows];
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int e = lane & 15, q = lane >> 4;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 dw1[2] = {zero, zero};
    f32x4 dwl[2][G], dbl[2] = {zero, zero};
#pragma unroll
    for (int l = 0; l < 2; l++)
#pragma unroll
        for (int kt = 0; kt < G; kt++) dwl[l][kt] = zero;
    f32x4 dwh = zero, dbh = zero;   // head: rows 4 q + reg of d_head against the wave's 16 inputs / against ones
    float loss1 = 0.0f, loss2 = 0.0f;   // t == 0
    const int n0 = 16 * wave + e;
    const int tiles = (A.n + kCgRows - 1) / kCgRows;
    const float fn = (float)A.n;
    const bool noisy = A.noise || A.sample;
    if (t < kCgRows * kAgHeadStride) dh[t] = 0.0f;

    for (int tile = blockIdx.x; tile < tiles; tile += A.nwg) {
        const int row0 = tile * kCgRows;
        if (t < kCgRows * 3) {
            const int row = t / 3, c = t - 3 * row, r = row0 + row;
            float eps = 0.0f;
            if (noisy && r < A.n) eps = A.sample ? philox_normal<kAgPhiloxTag>(A.seed, A.counter, (uint32_t)r, c) : A.noise[(unsigned)(r * 3 + c)];
            eps_l[row * 4 + c] = eps;
            if (A.eps_out && r < A.n) A.eps_out[(unsigned)(r * 3 + c)] = eps;
        }
        cg_stage<NT, false>(x0, A.obs, nullptr, row0, A.n, t);
        __syncthreads();
        // ---- actor forward, heads and the elementwise tail (wave 0)
        ag_forward<kAgObs>(A.a.w, A.a.b, x0, aa, A.acts[0], row0, A.n, e, q, n0);
        if (wave == 0) {
            f32x4 acc0 = zero, acc1 = zero;
            const float *wh = e < 3 ? A.a.mu_w : A.a.ls_w;
            const int hr = e < 3 ? e : (e < 6 ? e - 3 : 0);
            cg_dense<G>(wh, (unsigned)(hr * H + 4 * q), e < 6, aa[2] + e * S + 4 * q, acc0, acc1);
            const float bh = e < 6 ? (e < 3 ? A.a.mu_b : A.a.ls_b)[hr] : 0.0f;
            const int c = e < 3 ? e : 0;
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int row = 4 * q + reg, r = row0 + row;
                const float mean = (acc0[reg] + acc1[reg]) + bh;
                const float eps = eps_l[row * 4 + c];
                const float ls_raw = __shfl(mean, lane + 3, 64);   // column 3 + a holds log_std_a
                const float ls = fminf(fmaxf(ls_raw, -20.0f), 2.0f);
                const float std = expf(ls);
                const float se = std * eps;
                const float g = mean + se;
                const float a = tanhf(g);
                const float d = g - mean;       // torch.distributions.Normal.log_prob
                const float lpc = -(d * d) / (2.0f * (std * std)) - logf(std) - 0.91893853320467274f;
                const float sq = logf((1.0f - a * a) + 1e-6f);   // SquashedDiagGaussianDistribution, epsilon 1e-6
                const float lpc1 = __shfl(lpc, lane + 1, 64), lpc2 = __shfl(lpc, lane + 2, 64);
                const float sq1 = __shfl(sq, lane + 1, 64), sq2 = __shfl(sq, lane + 2, 64);
                const float lp = ((lpc + lpc1) + lpc2) - ((sq + sq1) + sq2);
                if (e == 0) {
                    s_lp[row] = lp;
                    if (r < A.n && A.log_prob) A.log_prob[(unsigned)r] = lp;
                }
                if (e >= 3) continue;
                const bool in = r < A.n;
                x0[row * kCgInStride + kAgObs + e] = in ? a : 0.0f;
                s_a[row * 4 + e] = in ? a : 0.0f;
                s_se[row * 4 + e] = se;
                s_mk[row * 4 + e] = (ls_raw >= -20.0f && ls_raw <= 2.0f) ? 1.0f : 0.0f;   // torch's clamp gradient
                if (in && A.actions) A.actions[(unsigned)(r * 3 + e)] = a;
            }
        }
        __syncthreads();
        // ---- the critics, one after the other: forward, q, then dQ/da from dq = 1
#pragma unroll 1
        for (int c = 0; c < 2; c++) {
            const CgCritic &C = A.c[c];
            ag_forward<kTgtIn>(C.w, C.b, x0, ca, A.acts[1 + c], row0, A.n, e, q, n0);
            if (wave == 0) {
                f32x4 acc0 = zero, acc1 = zero;
                cg_dense<G>(C.w[3], (unsigned)(4 * q), e == 0, ca[2] + e * S + 4 * q, acc0, acc1);
                const float bh = C.b[3][0];
                if (e == 0) {
#pragma unroll
                    for (int reg = 0; reg < 4; reg++) {
                        const int row = 4 * q + reg, gr = row0 + row;
                        const float qv = (acc0[reg] + acc1[reg]) + bh;
                        s_q[c][row] = qv;
                        if (gr < A.n && A.q[c]) A.q[c][(unsigned)gr] = qv;
                    }
                }
            }
            {   // dz_3 = a_3 > 0 ? w_out : 0 over a_3 (only this thread reads the element it writes)
                const int n = t & (H - 1), r4 = 4 * (t >> 7);
                const float wo = C.w[3][(unsigned)n];
                __syncthreads();   // wave 0 has read a_3
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    float *p = ca[2] + (r4 + r) * S + n;
                    *p = *p > 0.0f ? wo : 0.0f;
                }
            }
            __syncthreads();
#pragma unroll
            for (int l = 2; l >= 1; l--) {
                const f32x4 da = cg_da<H>(C.w[l], ca[l], e, q, n0);
#pragma unroll
                for (int reg = 0; reg < 4; reg++) {
                    float *p = ca[l - 1] + (4 * q + reg) * S + n0;
                    *p = *p > 0.0f ? da[reg] : 0.0f;
                }
                __syncthreads();
            }
            if (wave == 0) {   // dQ/da[row][k] = sum_n dz_1[row][n] W_1[n][18 + k]
                f32x4 acc0 = zero, acc1 = zero;
                const float *xr = ca[0] + e * S + 4 * q;
                const float *w1 = C.w[0];
                const unsigned off = (unsigned)(4 * q * kTgtIn + kAgObs + (e < 3 ? e : 0));
#pragma unroll
                for (int g = 0; g < G; g += 2) {
                    const f32x4 a0 = *reinterpret_cast<const f32x4 *>(xr + 16 * g);
                    const f32x4 a1 = *reinterpret_cast<const f32x4 *>(xr + 16 * g + 16);
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const float b0 = e < 3 ? (w1 + (16 * g + j) * kTgtIn)[off] : 0.0f;
                        const float b1 = e < 3 ? (w1 + (16 * g + 16 + j) * kTgtIn)[off] : 0.0f;
                        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[j], b0, acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[j], b1, acc1, 0, 0, 0);
                    }
                }
                if (e < 3) {
#pragma unroll
                    for (int reg = 0; reg < 4; reg++) dqa[c][(4 * q + reg) * 4 + e] = acc0[reg] + acc1[reg];
                }
            }
            __syncthreads();   // ca is free for the next critic; dqa is visible
        }
        // ---- the row's critic, the head gradients and the loss terms (wave 0)
        if (wave == 0 && e < 3) {
            const float alpha = A.log_ent_coef ? expf(A.log_ent_coef[0]) : A.ent_coef;
            const float ab = alpha / fn;
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int row = 4 * q + reg, r = row0 + row;
                const bool in = r < A.n;
                const float q1 = s_q[0][row], q2 = s_q[1][row];
                const int sel = q1 <= q2 ? 0 : 1;   // torch.min returns the first of equal values
                const float dq = dqa[sel][row * 4 + e];
                const float a = s_a[row * 4 + e], se = s_se[row * 4 + e];
                const float s = 1.0f - a * a;
                const float tt = ((2.0f * a) * s) / (s + 1e-6f);
                const float dla = -(dq / fn);
                float dmu = ab * tt + dla * s;
                float dls = ab * (-1.0f + tt * se) + (dla * s) * se;
                if (s_mk[row * 4 + e] == 0.0f) dls = 0.0f;
                if (!in) dmu = dls = 0.0f;
                dh[row * kAgHeadStride + e] = dmu;
                dh[row * kAgHeadStride + 3 + e] = dls;
                if (in) {
                    if (A.dq_da) A.dq_da[(unsigned)(r * 3 + e)] = dq;
                    if (A.d_mu) A.d_mu[(unsigned)(r * 3 + e)] = dmu;
                    if (A.d_ls) A.d_ls[(unsigned)(r * 3 + e)] = dls;
                }
                if (e == 0) {
                    const float lp = s_lp[row];
                    l1[row] = in ? alpha * lp - (sel ? q2 : q1) : 0.0f;
                    l2[row] = in ? lp + A.target_entropy : 0.0f;
                }
            }
        }
        __syncthreads();
        // ---- head weight and bias gradients from a_3
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const int row = 4 * q + s;
            const float a = dh[row * kAgHeadStride + e];   // A[i = e][k = q]: d_head[row][e]
            dwh = __builtin_amdgcn_mfma_f32_16x16x4f32(a, aa[2][row * S + n0], dwh, 0, 0, 0);
            dbh = __builtin_amdgcn_mfma_f32_16x16x4f32(a, 1.0f, dbh, 0, 0, 0);
        }
        if (t == 0) {
#pragma unroll
            for (int row = 0; row < kCgRows; row++) {
                loss1 = loss1 + l1[row];
                loss2 = loss2 + l2[row];
            }
        }
        __syncthreads();   // every wave has read a_3
        {   // dz_3 = a_3 > 0 ? sum_i d_head[i] W_head[i][n] : 0 over a_3
            const int n = t & (H - 1), r4 = 4 * (t >> 7);
            float wm[3], wl[3];
#pragma unroll
            for (int i = 0; i < 3; i++) {
                wm[i] = A.a.mu_w[(unsigned)(i * H + n)];
                wl[i] = A.a.ls_w[(unsigned)(i * H + n)];
            }
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float *d = dh + (r4 + r) * kAgHeadStride;
                float v = d[0] * wm[0];
                v = fmaf(d[1], wm[1], v);
                v = fmaf(d[2], wm[2], v);
                v = fmaf(d[3], wl[0], v);
                v = fmaf(d[4], wl[1], v);
                v = fmaf(d[5], wl[2], v);
                float *p = aa[2] + (r4 + r) * S + n;
                *p = *p > 0.0f ? v : 0.0f;
            }
        }
        __syncthreads();
        // ---- hidden layers, last to first
#pragma unroll
        for (int l = 2; l >= 0; l--) {
#pragma unroll
            for (int s = 0; s < 4; s++) {
                const int row = 4 * q + s;
                const float a = aa[l][row * S + n0];   // A[i = e][k = q]: dz[row][n]
                if (l == 0) {
#pragma unroll
                    for (int kt = 0; kt < 2; kt++)
                        dw1[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, x0[row * kCgInStride + 16 * kt + e], dw1[kt], 0, 0, 0);
                } else {
#pragma unroll
                    for (int kt = 0; kt < G; kt++)
                        dwl[l - 1][kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, aa[l - 1][row * S + 16 * kt + e], dwl[l - 1][kt], 0, 0, 0);
                    dbl[l - 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, 1.0f, dbl[l - 1], 0, 0, 0);
                }
            }
            if (l == 0) {
                __syncthreads();   // x0, aa and dh are free for the next tile
                break;
            }
            const f32x4 da = cg_da<H>(A.a.w[l], aa[l], e, q, n0);
            __syncthreads();   // every wave has read a_{l-1} (dW_l) and dz_l
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                float *p = aa[l - 1] + (4 * q + reg) * S + n0;
                *p = *p > 0.0f ? da[reg] : 0.0f;
            }
            __syncthreads();
        }
    }

    // ---- the workgroup's partial set, torch layout; D[i = 4 q + reg][j = e]
    float *P = A.partial + (size_t)blockIdx.x * L::set;
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
        const int n = 16 * wave + 4 * q + reg;   // neuron of the hidden layers' tiles
#pragma unroll
        for (int l = 1; l < 3; l++) {
#pragma unroll
            for (int kt = 0; kt < G; kt++) P[L::hw(l) + n * H + 16 * kt + e] = dwl[l - 1][kt][reg];
            if (e == 0) P[L::hb(l) + n] = dbl[l - 1][reg];
        }
        cg_put_dw1<kAgObs>(P, L::b1, dw1, reg, n, e);
        const int i = 4 * q + reg;               // row of the head tile: 0..2 mu, 3..5 log_std
        if (i < 6) {
            const int hr = i < 3 ? i : i - 3;
            P[(i < 3 ? L::mu_w : L::ls_w) + hr * H + n0] = dwh[reg];
            if (wave == 0 && e == 0) P[(i < 3 ? L::mu_b : L::ls_b) + hr] = dbh[reg];
        }
    }
    if (t == 0) {
        P[L::stride] = loss1;
        P[L::stride + 1] = loss2;
    }
}

// grad[i] = partial[0][i] + partial[1][i] + ... in index order; with S_1, S_2 the loss sums added the same way:
// actor_loss = S_1 / B; m = S_2 / B; log_ent_coef.grad = -m; ent_coef_loss = -(log_ent_coef m)
__global__ void __launch_bounds__(256)
k_actor_grad_reduce(const float *__restrict__ partial, int nwg, int n, const float *__restrict__ log_ent_coef, float *__restrict__ grad,
                    float *__restrict__ loss)
{
    using L = AgLayout;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < L::ent) {
        float s[1];
        cg_sum_sets<1, true>(partial, nwg, L::set, i, s);
        grad[i] = s[0];
    }
    if (i == 0) {
        float s[2];
        cg_sum_sets<2, false>(partial, nwg, L::set, L::stride, s);
        loss[0] = s[0] / (float)n;
        if (log_ent_coef) {
            const float m = s[1] / (float)n;
            grad[L::ent] = -m;
            loss[1] = -(log_ent_coef[0] * m);
        }
    }
}

}  // namespace meshenv
