// meshenv_ppo_grad.h -- the loss of PPO and A2C and its gradients (SB3 2.x's PPO.train / A2C.train, one minibatch of B rows:
//
//   values, log_prob, entropy = policy.evaluate_actions(obs, actions)        # DiagGaussian, state-independent log_std [3]
//   if normalize_advantage and B > 1: adv = (adv - adv.mean()) / (adv.std() + 1e-8)
//   ratio = exp(log_prob - old_log_prob)
//   policy_loss  = -min(adv * ratio, adv * clamp(ratio, 1 - clip_range, 1 + clip_range)).mean()      # A2C: -(adv * log_prob).mean()
//   value_loss   = mse_loss(returns, values);  entropy_loss = -mean(entropy)
//   loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss
//   loss.backward(); clip_grad_norm_(policy.parameters(), max_grad_norm)
//
// for the actor-critic MLP policies the reference trains with: rl/baselines/RL_Mesh.py:113-177, PPO ReLU [128, 128] x 2, and
// SB3's default A2C Tanh [64, 64]).  (The live tensors reach a loaded FusedPolicy's packed buffer through k_target_pack of
// meshenv_pack.h: meshenv_policy_bind fills its PackTable, meshenv_policy_refresh launches it.)
// At most four launches: k_ppo_adv_stats (when normalising), k_ppo_grad<H, ACT>, k_ppo_grad_reduce, k_ppo_grad_clip (with a
// max_grad_norm).
//
// k_ppo_grad<H, ACT>, H = 64 or 128, ReLU or Tanh.  blockIdx.y is the tower (0 = pi, 1 = vf), as in k_policy_forward: the loss
// couples the towers through scalars only, so each is a forward and a backward from its own head gradient.  The tiling of
// k_critic_grad: 16 rows per tile, H / 16 wavefronts, wave w owning neurons [16 w, 16 w + 16) of both hidden layers,
// v_mfma_f32_16x16x4_f32 throughout, weights read from the LIVE [out][in] tensors (cg_dense forward, buffer loads for
// da = dz W), activations in LDS with row stride H + 4; blockIdx.x walks the tiles blockIdx.x, blockIdx.x + nwg, ... with its
// accumulators in registers.  Per tile:
//
//   forward   a_l = act(W_l a_{l-1} + b_l), l = 1, 2, both kept in LDS; a_0 = 18 observations padded to 32, a_0[21] = 1
//   pi head   wave 0, columns 0..2 of one 16-wide tile: mean = W_h a_2 + b_h; std = expf(log_std), d = action - mean,
//             lp_i = -(d d) / (2 (std std)) - logf(std) - 0.9189385f, log_prob = (lp_0 + lp_1) + lp_2 (k_policy_forward's order);
//             adv' = (adv - mean_adv) * inv_std_adv when normalising; log_ratio = log_prob - old_log_prob, ratio = expf(log_ratio),
//             p1 = adv' ratio, p2 = adv' min(max(ratio, lo), hi), the surrogate term min(p1, p2);
//             c = dL/dlog_prob = passes ? -(p1 / B) : 0   (A2C: the term adv' log_prob, c = -(adv' / B));
//             d_mean_i = (c d_i) / var_i, the row's d_log_std_i term c ((d_i d_i) / var_i - 1); exactly 0 for rows past B
//   vf head   wave 0, column 0: v = W_h a_2 + b_h, diff = v - returns, d_v = (vf_coef (2 diff)) / B, the term diff diff
//   backward  head weights: thread t owns one element of dW_h (fmaf, rows in order), further threads db_h and the row sums;
//             dz_2 = act'(a_2) sum_i d_head[i] W_h[i][n] (one product, and two fmaf for the pi tower) over a_2; dW_2, db_2
//             (MFMA, K = the 16 rows), da_1 = dz_2 W_2, dz_1 = act'(a_1) da_1 over a_1, dW_1 and, against the column of ones,
//             db_1.  act'(a) is a > 0 for ReLU and 1 - a a for Tanh, from the kept activation.
//
// The "passes" predicate is autograd's.  Inside [lo, hi] = [1 - clip_range, 1 + clip_range], INCLUSIVE, clamp passes its
// gradient and the two products are equal: minimum halves the gradient between them and both halves arrive at ratio, so the
// row gets the full gradient.  Outside, p2 is constant in ratio and the gradient flows only when p1 < p2, the unclamped product
// being the smaller one (p1 == p2 outside the range needs adv' ratio == adv' clamp(ratio), a zero gradient either way):
//
//   passes = (lo <= ratio && ratio <= hi) || p1 < p2
//
// Reduction order of a gradient element and of the four row sums (tests/ppo_grad_ref.py derives its bounds from it): one fma /
// add chain over the rows of the workgroup's tiles, 16 T roundings for T = ceil(tiles / nwg), then nwg - 1 additions over the
// partial sets in index order by k_ppo_grad_reduce; nwg as in meshenv_critic_grad.h.  No floating-point atomics: two calls on
// the same inputs give the same bits.
#pragma once

#include "meshenv_critic_grad.h"

namespace meshenv {

constexpr int kPgObs = kCgObs;   // inputs of both towers
constexpr int kPgTensors = 13;   // pi w1 b1 w2 b2 wh bh, vf likewise, log_std
constexpr int kPgSums = 4;       // row sums behind a partial set: surrogate, squared value error, kl term, clipped rows
constexpr int kPgParts = 5;      // optional per-row outputs: log_prob ratio values advantages pass
constexpr int kPgOut = 8;        // loss policy_loss value_loss entropy_loss approx_kl clip_fraction grad_norm (one spare)
constexpr int kPgStatThreads = 1024;

// The gradient set, torch layout, in PPOGradSpec's order; padded to a multiple of 64 floats.  A partial set carries the four
// row sums after it.
template <int H>
struct PgLayout {
    static constexpr int b1 = H * kPgObs;
    static constexpr int w2 = b1 + H;
    static constexpr int b2 = w2 + H * H;
    static constexpr int wh = b2 + H;
    static constexpr int vf = wh + 3 * H + 3;          // the vf tower's first float: behind the pi head [3][H] and its bias [3]
    static constexpr int log_std = vf + wh + H + 1;    // behind the value head [1][H] and its bias [1]
    static constexpr int params = log_std + 3;
    static constexpr int stride = (params + 63) & ~63;
    static constexpr int set = stride + 64;
};

// first float of each of the 13 tensors, and the end of the last, for a width known at run time
__host__ __device__ inline void pg_offsets(int H, int off[kPgTensors + 1])
{
    int at = 0;
    for (int tower = 0; tower < 2; tower++) {
        const int n_out = tower == 0 ? 3 : 1;
        const int sizes[6] = {H * kPgObs, H, H * H, H, n_out * H, n_out};
        for (int i = 0; i < 6; i++) {
            off[6 * tower + i] = at;
            at += sizes[i];
        }
    }
    off[12] = at;
    off[13] = at + 3;
}

struct PgTower {
    const float *w[3], *b[3];   // two hidden layers and the head (torch layout)
};

struct PgArgs {
    int n, nwg;
    int a2c, normalize;
    const float *obs, *actions, *old_log_prob, *adv, *returns;   // [n][18] [n][3] [n] [n] [n]
    const float *stats;          // [2]: the mean of adv and 1 / (std + 1e-8), read when normalize
    float lo, hi, clip, vf_coef;
    PgTower t[2];
    const float *log_std;        // [3]
    float *partial;              // [nwg][PgLayout::set]
    float *log_prob, *ratio, *values, *advn, *pass;   // [n] each, every one nullable
    float *acts[2][2];           // [tower][layer]: [n][H] kept activations, nullable
};

// a' of the backward pass from the kept activation a: g act'(a)
template <int ACT>
__device__ __forceinline__ float pg_back(float a, float g)
{
    return ACT == kPolicyTanh ? g * (1.0f - a * a) : (a > 0.0f ? g : 0.0f);
}

template <int H, int ACT>
__global__ void __launch_bounds__(4 * H)
k_ppo_grad(PgArgs A)
{
    constexpr int G = H / 16, S = H + 4, NT = 4 * H;
    using L = PgLayout<H>;
    __shared__ __attribute__((aligned(16))) float x0[kCgRows * kCgInStride];
    __shared__ __attribute__((aligned(16))) float aa[2][kCgRows * S];   // a_1 and a_2, then dz_1 and dz_2
    __shared__ float dh[kCgRows * 4];   // the head gradient: columns 0..2 (pi), 0 (vf)
    __shared__ float st[kCgRows * 8];   // the row's terms: pi 0..2 d_log_std, 3 surrogate, 4 kl, 5 clipped; vf 0 squared error
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int e = lane & 15, q = lane >> 4, n0 = 16 * wave + e;
    const int tower = blockIdx.y;
    const bool pi = tower == 0;
    const PgTower &T = A.t[tower];
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 dw1[2] = {zero, zero};
    f32x4 dw2[G], db2 = zero;
#pragma unroll
    for (int kt = 0; kt < G; kt++) dw2[kt] = zero;
    float hacc = 0.0f;   // pi: t < 3 H dW_h[t / H][t % H], then 3 db_h, 3 d_log_std, surrogate, kl, clipped; vf: H dW_h, db_h, squared error
    const int tiles = (A.n + kCgRows - 1) / kCgRows;
    const float fn = (float)A.n;

    for (int tile = blockIdx.x; tile < tiles; tile += A.nwg) {
        const int row0 = tile * kCgRows;
        cg_stage<NT, false>(x0, A.obs, nullptr, row0, A.n, t);
        __syncthreads();
        // ---- forward
        cg_store<H>(aa[0], A.acts[tower][0], cg_first_layer<kPgObs, ACT>(T.w[0], T.b[0], x0, e, q, n0), row0, A.n, q, n0);
        __syncthreads();
        cg_store<H>(aa[1], A.acts[tower][1], cg_hidden_layer<H, ACT>(T.w[1], T.b[1], aa[0], e, q, n0), row0, A.n, q, n0);
        __syncthreads();
        // ---- the head and its gradient (wave 0)
        if (wave == 0) {
            const int n_out = pi ? 3 : 1;
            const int hr = e < n_out ? e : 0;
            f32x4 acc0 = zero, acc1 = zero;
            cg_dense<G>(T.w[2], (unsigned)(hr * H + 4 * q), e < n_out, aa[1] + e * S + 4 * q, acc0, acc1);
            const float bh = T.b[2][hr];
            if (pi) {
                const float std = expf(A.log_std[hr]);   // torch: log_std.exp()
                const float var = std * std, lstd = logf(std);
                const float am = A.normalize ? A.stats[0] : 0.0f, as = A.normalize ? A.stats[1] : 1.0f;
#pragma unroll
                for (int reg = 0; reg < 4; reg++) {
                    const int row = 4 * q + reg, gr = row0 + row;
                    const bool in = gr < A.n;
                    const float mean = (acc0[reg] + acc1[reg]) + bh;
                    const float act = in && e < 3 ? A.actions[(unsigned)(gr * 3 + e)] : mean;
                    const float d = act - mean;          // torch.distributions.Normal.log_prob
                    const float dd = d * d;
                    const float lp = -dd / (2.0f * var) - lstd - 0.91893853320467274f;
                    // the three components sit in lanes 0..2 of the row's quarter-wave; torch's order of the sum
                    const float lp0 = __shfl(lp, lane & 48, 64), lp1 = __shfl(lp, (lane & 48) + 1, 64), lp2 = __shfl(lp, (lane & 48) + 2, 64);
                    const float logp = (lp0 + lp1) + lp2;
                    float adv = 0.0f, ratio = 1.0f, c = 0.0f, sur = 0.0f, kl = 0.0f, cf = 0.0f, pass = 1.0f;
                    if (in) {
                        adv = A.adv[(unsigned)gr];
                        if (A.normalize) adv = (adv - am) * as;
                        if (A.a2c) {
                            sur = adv * logp;
                            c = -(adv / fn);
                        } else {
                            const float lr = logp - A.old_log_prob[(unsigned)gr];
                            ratio = expf(lr);
                            const float p1 = adv * ratio, p2 = adv * fminf(fmaxf(ratio, A.lo), A.hi);
                            sur = fminf(p1, p2);
                            const bool passes = (ratio >= A.lo && ratio <= A.hi) || p1 < p2;   // autograd's: see the top
                            c = passes ? -(p1 / fn) : 0.0f;
                            kl = (ratio - 1.0f) - lr;
                            cf = fabsf(ratio - 1.0f) > A.clip ? 1.0f : 0.0f;
                            pass = passes ? 1.0f : 0.0f;
                        }
                    }
                    if (e < 3) {
                        dh[row * 4 + e] = (c * d) / var;
                        st[row * 8 + e] = c * (dd / var - 1.0f);
                    } else if (e == 3) {
                        st[row * 8 + 3] = sur;
                        st[row * 8 + 4] = kl;
                        st[row * 8 + 5] = cf;
                        if (in) {
                            if (A.log_prob) A.log_prob[(unsigned)gr] = logp;
                            if (A.ratio) A.ratio[(unsigned)gr] = ratio;
                            if (A.advn) A.advn[(unsigned)gr] = adv;
                            if (A.pass) A.pass[(unsigned)gr] = pass;
                        }
                    }
                }
            } else if (e == 0) {
#pragma unroll
                for (int reg = 0; reg < 4; reg++) {
                    const int row = 4 * q + reg, gr = row0 + row;
                    float dv = 0.0f, sq = 0.0f;
                    if (gr < A.n) {
                        const float v = (acc0[reg] + acc1[reg]) + bh;
                        const float diff = v - A.returns[(unsigned)gr];
                        dv = (A.vf_coef * (2.0f * diff)) / fn;
                        sq = diff * diff;
                        if (A.values) A.values[(unsigned)gr] = v;
                    }
                    dh[row * 4] = dv;
                    st[row * 8] = sq;
                }
            }
        }
        __syncthreads();
        // ---- head weight and bias gradients from a_2, the row sums
        if (pi) {
            if (t < 3 * H) {
                const int i = t / H, n = t & (H - 1);
#pragma unroll
                for (int row = 0; row < kCgRows; row++) hacc = fmaf(dh[row * 4 + i], aa[1][row * S + n], hacc);
            } else if (t < 3 * H + 3) {
#pragma unroll
                for (int row = 0; row < kCgRows; row++) hacc = hacc + dh[row * 4 + (t - 3 * H)];
            } else if (t < 3 * H + 9) {
#pragma unroll
                for (int row = 0; row < kCgRows; row++) hacc = hacc + st[row * 8 + (t - 3 * H - 3)];
            }
        } else {
            if (t < H) {
#pragma unroll
                for (int row = 0; row < kCgRows; row++) hacc = fmaf(dh[row * 4], aa[1][row * S + t], hacc);
            } else if (t == H) {
#pragma unroll
                for (int row = 0; row < kCgRows; row++) hacc = hacc + dh[row * 4];
            } else if (t == H + 1) {
#pragma unroll
                for (int row = 0; row < kCgRows; row++) hacc = hacc + st[row * 8];
            }
        }
        __syncthreads();   // every thread has read a_2
        {   // dz_2 = act'(a_2) sum_i d_head[i] W_h[i][n] over a_2
            const int n = t & (H - 1), r4 = 4 * (t / H);
            const float w0 = T.w[2][(unsigned)n];
            const float w1 = pi ? T.w[2][(unsigned)(H + n)] : 0.0f, w2 = pi ? T.w[2][(unsigned)(2 * H + n)] : 0.0f;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float *d = dh + (r4 + r) * 4;
                float v = d[0] * w0;
                if (pi) {
                    v = fmaf(d[1], w1, v);
                    v = fmaf(d[2], w2, v);
                }
                float *p = aa[1] + (r4 + r) * S + n;
                *p = pg_back<ACT>(*p, v);
            }
        }
        __syncthreads();
        // ---- layer 2: dW_2, db_2, da_1
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const int row = 4 * q + s;
            const float a = aa[1][row * S + n0];   // A[i = e][k = q]: dz_2[row][n]
#pragma unroll
            for (int kt = 0; kt < G; kt++) dw2[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, aa[0][row * S + 16 * kt + e], dw2[kt], 0, 0, 0);
            db2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, 1.0f, db2, 0, 0, 0);
        }
        {
            const f32x4 da = cg_da<H>(T.w[1], aa[1], e, q, n0);
            __syncthreads();   // every wave has read a_1 (dW_2) and dz_2
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                float *p = aa[0] + (4 * q + reg) * S + n0;
                *p = pg_back<ACT>(*p, da[reg]);
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
        __syncthreads();   // x0, aa, dh and st are free for the next tile
    }

    // ---- the workgroup's partial set, torch layout; D[i = 4 q + reg][j = e]: neuron 16 wave + 4 q + reg, input 16 kt + e
    float *set = A.partial + (size_t)blockIdx.x * L::set;
    float *P = set + (pi ? 0 : L::vf);
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
        const int n = 16 * wave + 4 * q + reg;
#pragma unroll
        for (int kt = 0; kt < G; kt++) P[L::w2 + n * H + 16 * kt + e] = dw2[kt][reg];
        if (e == 0) P[L::b2 + n] = db2[reg];
        cg_put_dw1<kPgObs>(P, L::b1, dw1, reg, n, e);
    }
    if (pi) {
        if (t < 3 * H + 3) P[L::wh + t] = hacc;                         // wh [3][H] and bh [3] are adjacent
        else if (t < 3 * H + 6) set[L::log_std + (t - 3 * H - 3)] = hacc;
        else if (t == 3 * H + 6) set[L::stride + 0] = hacc;             // surrogate
        else if (t == 3 * H + 7) set[L::stride + 2] = hacc;             // kl
        else if (t == 3 * H + 8) set[L::stride + 3] = hacc;             // clipped rows
    } else {
        if (t < H + 1) P[L::wh + t] = hacc;                             // wh [1][H] and bh [1] are adjacent
        else if (t == H + 1) set[L::stride + 1] = hacc;                 // squared value error
    }
}

// grad[i] = partial[0][i] + partial[1][i] + ... in index order, minus ent_coef for log_std (entropy = sum_i (0.5 + 0.5 log(2 pi)
// + log_std_i) whatever the row); the four row sums the same way, then out[0..5] = loss, policy_loss = -(S_0 / B), value_loss =
// S_1 / B, entropy_loss, approx_kl = S_2 / B, clip_fraction = S_3 / B.  out[6] (grad_norm) is k_ppo_grad_clip's; NaN without it.
__global__ void __launch_bounds__(256)
k_ppo_grad_reduce(const float *__restrict__ partial, int nwg, int set, int stride, int params, int n, float ent_coef, float vf_coef,
                  const float *__restrict__ log_std, int clipped, float *__restrict__ grad, float *__restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < params) {
        float s[1];
        cg_sum_sets<1, true>(partial, nwg, set, i, s);
        if (i >= params - 3) s[0] = s[0] - ent_coef;
        grad[i] = s[0];
    }
    if (i == 0) {
        float s[kPgSums];
        cg_sum_sets<kPgSums, false>(partial, nwg, set, stride, s);
        const float fn = (float)n, c = 1.4189385332046727f;   // 0.5 + 0.5 log(2 pi)
        const float policy_loss = -(s[0] / fn), value_loss = s[1] / fn;
        const float entropy_loss = -(((c + log_std[0]) + (c + log_std[1])) + (c + log_std[2]));
        out[0] = (policy_loss + ent_coef * entropy_loss) + vf_coef * value_loss;
        out[1] = policy_loss;
        out[2] = value_loss;
        out[3] = entropy_loss;
        out[4] = s[2] / fn;
        out[5] = s[3] / fn;
        if (!clipped) out[6] = __builtin_nanf("");
    }
}

// One workgroup in a fixed order: every thread adds its elements t, t + 1024, ... in order, then a binary tree over the 1024
// partial sums in LDS.  Returns the sum to every thread.
__device__ __forceinline__ float pg_block_sum(float s, float *red, int t)
{
    red[t] = s;
    __syncthreads();
    for (int w = kPgStatThreads / 2; w > 0; w >>= 1) {
        if (t < w) red[t] = red[t] + red[t + w];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

// stats[0] = mean(adv), stats[1] = 1 / (std + 1e-8) with torch's unbiased std: two passes, the mean, then the centred
// squares over n - 1 (n > 1: the host does not normalise one row)
__global__ void __launch_bounds__(kPgStatThreads)
k_ppo_adv_stats(const float *__restrict__ adv, int n, float *__restrict__ stats)
{
    __shared__ float red[kPgStatThreads];
    const int t = threadIdx.x;
    float s = 0.0f;
    for (int i = t; i < n; i += kPgStatThreads) s = s + adv[i];
    const float mean = pg_block_sum(s, red, t) / (float)n;
    s = 0.0f;
    for (int i = t; i < n; i += kPgStatThreads) {
        const float d = adv[i] - mean;
        s = s + d * d;
    }
    const float var = pg_block_sum(s, red, t) / (float)(n - 1);
    if (t == 0) {
        stats[0] = mean;
        stats[1] = 1.0f / (sqrtf(var) + 1e-8f);
    }
}

// torch's clip_grad_norm_ on the 13 gradients of the flat buffer, one workgroup in a fixed order: per tensor the sum of squares
// (pg_block_sum) and its root, total_norm = the root of the sum of the 13 squared norms in tensor order, coef =
// min(max_norm / (total_norm + 1e-6), 1), every gradient multiplied by coef (by 1.0 too, as torch does: exact).  out[6] =
// total_norm before clipping.
__global__ void __launch_bounds__(kPgStatThreads)
k_ppo_grad_clip(float *__restrict__ grad, int H, float max_norm, float *__restrict__ out)
{
    __shared__ float red[kPgStatThreads];
    const int t = threadIdx.x;
    int off[kPgTensors + 1];
    pg_offsets(H, off);
    float total = 0.0f;
    for (int k = 0; k < kPgTensors; k++) {
        float s = 0.0f;
        for (int i = off[k] + t; i < off[k + 1]; i += kPgStatThreads) {
            const float g = grad[i];
            s = s + g * g;
        }
        const float norm = sqrtf(pg_block_sum(s, red, t));
        total = total + norm * norm;
    }
    const float total_norm = sqrtf(total);
    const float coef = fminf(max_norm / (total_norm + 1e-6f), 1.0f);
    for (int i = t; i < off[kPgTensors]; i += kPgStatThreads) grad[i] = grad[i] * coef;
    if (t == 0) out[6] = total_norm;
}

}  // namespace meshenv
