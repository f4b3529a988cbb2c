// meshenv_critic_grad.h -- the critic loss of SAC and TD3 and its gradients (SB3 2.x's SAC.train / TD3.train:
//
//   current_q_values = self.critic(replay_data.observations, replay_data.actions)
//   critic_loss = 0.5 * sum(F.mse_loss(current_q, target_q_values) for current_q in current_q_values)
//   self.critic.optimizer.zero_grad(); critic_loss.backward()
//
// for the twin critics the reference trains: rl/baselines/RL_Mesh.py:179-222, SAC ReLU [128, 128, 128], TD3 ReLU [256, 256],
// input cat(obs, action) = 21).  Two launches: k_critic_grad<KIND> writes one partial gradient set per workgroup,
// k_critic_grad_reduce sums the sets in index order into the gradient buffer (torch's [out][in] / [out] layout).
//
// k_critic_grad<KIND>.  blockIdx.y is the critic, blockIdx.x the workgroup of that critic; a workgroup walks the 16-sample
// tiles blockIdx.x, blockIdx.x + nwg, ... and has H / 16 wavefronts, wave w owning neurons [16 w, 16 w + 16) of every hidden
// layer (the tiling of meshenv_target.h).  The weights are read from the LIVE torch tensors as they are: with the MFMA step
// (group g, j) of lane (e = lane & 15, q = lane >> 4) taking k = 16 g + 4 q + j, the B operand of the forward is 16
// contiguous bytes of row n = 16 w + e of W, and the A operand 16 contiguous bytes of row e of the activations in LDS in
// their natural order (row stride H + 4 floats: the 16 rows of a quarter-wave on distinct banks).  Per tile:
//
//   forward   a_l = relu(W_l a_{l-1} + b_l), a_0 = cat(obs, action) padded to 32 with a_0[21] = 1 (the weights of the
//             padding are read as 0), every a_l kept in LDS; q = W_h a_L + b_h on wave 0 (v_mfma_f32_16x16x4_f32 throughout:
//             exact f32, two accumulators over even / odd 16-groups of k)
//   dq        = (q - y) / B, 0 for rows past B; the loss term (q - y)^2
//   head      dW_h[n] += dq[row] a_L[row][n] (fmaf, rows in order), db_h += dq[row]; dz_L = a_L > 0 ? dq W_h[n] : 0,
//             written over a_L
//   layer l   dW_l += dz_l^T a_{l-1}: M = the wave's 16 neurons, N = 16 inputs per accumulator tile, K = the 16 rows
//             (MFMA step s of lane quarter q takes row 4 q + s: conflict-free LDS reads); the accumulators stay in
//             registers over all tiles of the workgroup.  db_l is the same product against a column of ones: column 21 of
//             a_0 for the first layer, one more accumulator tile for the others.
//             da_{l-1} = dz_l W_l for the wave's 16 columns (k over the H neurons, two accumulators as in the forward; W_l
//             read by columns, 64 bytes per row and quarter-wave); dz_{l-1} = a_{l-1} > 0 ? da_{l-1} : 0 written over
//             a_{l-1} once every wave has read it.  The first layer needs no da.
//
// Reduction order of a gradient element (tests/critic_grad_ref.py derives its bound from it): one fma chain over the rows
// of the workgroup's tiles, 16 T roundings for T = ceil(tiles / nwg) tiles, then nwg - 1 additions over the partial sets in
// index order.  nwg = min(tiles, 64) up to 512 tiles, 128 beyond (kCgMaxGroups); no floating-point atomics anywhere, so two
// calls on the same inputs give the same bits.
//
// The per-tile pieces (staging, cg_first, cg_dense, cg_da, the dW_1 write-out, the sum over the partial sets) are the shared
// helpers of meshenv_grad_tile.h.
#pragma once

#include "meshenv_grad_tile.h"

namespace meshenv {

constexpr int kCgMaxLayers = 4;   // hidden layers + head
constexpr int kCgSplitTD3 = 2;    // TD3: workgroups per critic and tile set, each accumulating half the columns of dW_2

// One gradient set: per critic w1 [H][21], b1 [H], then w_l [H][H], b_l [H] per further hidden layer, wh [H], bh [1], padded
// to a multiple of 64 floats; the partial sets carry the two loss sums after the second critic.
template <int H, int NL>
struct CgLayout {
    static constexpr int b1 = H * kTgtIn;
    static constexpr int hidden0 = b1 + H;
    static constexpr int hidden_stride = H * H + H;
    static constexpr int wh = hidden0 + (NL - 1) * hidden_stride;
    static constexpr int bh = wh + H;
    static constexpr int params = bh + 1;
    static constexpr int stride = (params + 63) & ~63;
    static constexpr int grads = 2 * stride;
    static constexpr int set = grads + 64;
    __host__ __device__ static constexpr int hw(int l) { return hidden0 + (l - 1) * hidden_stride; }   // l = 1 .. NL - 1
    __host__ __device__ static constexpr int hb(int l) { return hw(l) + H * H; }
};

struct CgCritic {
    const float *w[kCgMaxLayers], *b[kCgMaxLayers];   // hidden layers 0 .. NL - 1, then the head at NL (torch layout)
};

struct CgArgs {
    int n, nwg;
    const float *obs, *actions, *target;   // [n][18], [n][3], [n]
    CgCritic c[2];
    float *partial;                        // [nwg][CgLayout::set]
    float *q[2];                           // [n], nullable
    float *acts[2][kCgMaxLayers - 1];      // [n][H] post-ReLU activations per hidden layer, nullable
};

template <int KIND>
__global__ void __launch_bounds__(KIND == kTargetSAC ? 512 : 1024)
k_critic_grad(CgArgs A)
{
    constexpr int H = KIND == kTargetSAC ? 128 : 256, NL = KIND == kTargetSAC ? 3 : 2;
    constexpr int G = H / 16, S = H + 4, NT = 64 * G;
    constexpr int KS = KIND == kTargetSAC ? 1 : kCgSplitTD3, GH = G / KS;   // input tiles of a hidden dW per workgroup
    using L = CgLayout<H, NL>;
    __shared__ __attribute__((aligned(16))) float x0[kCgRows * kCgInStride];
    __shared__ __attribute__((aligned(16))) float act[NL][kCgRows * S];
    __shared__ float dq[kCgRows], d2[kCgRows];
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int e = lane & 15, q = lane >> 4;
    const int c = blockIdx.y / KS, half = blockIdx.y % KS;
    const CgCritic &C = A.c[c];
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 dw1[2] = {zero, zero};
    f32x4 dwl[NL - 1][GH], dbl[NL - 1];
#pragma unroll
    for (int l = 0; l < NL - 1; l++) {
        dbl[l] = zero;
#pragma unroll
        for (int kt = 0; kt < GH; kt++) dwl[l][kt] = zero;
    }
    float dwo = 0.0f, dbo = 0.0f, loss = 0.0f;   // head weight of neuron t (t < H); head bias and loss sum (t == H)
    const int n0 = 16 * wave + e;
    const int tiles = (A.n + kCgRows - 1) / kCgRows;
    const float fn = (float)A.n;

    for (int tile = blockIdx.x; tile < tiles; tile += A.nwg) {
        const int row0 = tile * kCgRows;
        cg_stage<NT, true>(x0, A.obs, A.actions, row0, A.n, t);
        __syncthreads();
        // ---- forward
#pragma unroll
        for (int l = 0; l < NL; l++) {
            // the epilogue stays inline: through cg_bias_act / cg_store this kernel allocates more VGPRs (168 -> 170, 124 -> 128)
            f32x4 acc0 = zero, acc1 = zero;
            if (l == 0) cg_first<kTgtIn>(C.w[0], x0, e, q, n0, acc0, acc1);
            else cg_dense<G>(C.w[l], (unsigned)(n0 * H + 4 * q), true, act[l - 1] + e * S + 4 * q, acc0, acc1);
            const float b = C.b[l][(unsigned)n0];
            float *out = A.acts[c][l];
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {   // D[row = 4 q + reg][col = e]
                const int row = 4 * q + reg;
                const float v = fmaxf((acc0[reg] + acc1[reg]) + b, 0.0f);
                act[l][row * S + n0] = v;
                if (out && half == 0 && row0 + row < A.n) out[(unsigned)((row0 + row) * H + n0)] = v;
            }
            __syncthreads();
        }
        // ---- head, dq and the loss terms (wave 0)
        if (wave == 0) {
            f32x4 acc0 = zero, acc1 = zero;
            cg_dense<G>(C.w[NL], (unsigned)(4 * q), e == 0, act[NL - 1] + e * S + 4 * q, acc0, acc1);
            const float bh = C.b[NL][0];
            if (e == 0) {
#pragma unroll
                for (int reg = 0; reg < 4; reg++) {
                    const int row = 4 * q + reg, gr = row0 + row;
                    float d = 0.0f, dd = 0.0f;
                    if (gr < A.n) {
                        const float qv = (acc0[reg] + acc1[reg]) + bh;
                        const float diff = qv - A.target[(unsigned)gr];
                        dd = diff * diff;
                        d = diff / fn;
                        if (A.q[c] && half == 0) A.q[c][(unsigned)gr] = qv;
                    }
                    dq[row] = d;
                    d2[row] = dd;
                }
            }
        }
        __syncthreads();
        // ---- head gradients; dz of the last hidden layer over its activations
        if (t < H) {
            const float wh = C.w[NL][(unsigned)t];
            float *col = act[NL - 1] + t;
#pragma unroll
            for (int row = 0; row < kCgRows; row++) {
                const float a = col[row * S], d = dq[row];
                dwo = fmaf(d, a, dwo);
                col[row * S] = a > 0.0f ? d * wh : 0.0f;
            }
        } else if (t == H) {
#pragma unroll
            for (int row = 0; row < kCgRows; row++) {
                dbo = dbo + dq[row];
                loss = loss + d2[row];
            }
        }
        __syncthreads();
        // ---- hidden layers, last to first
#pragma unroll
        for (int l = NL - 1; l >= 0; l--) {
#pragma unroll
            for (int s = 0; s < 4; s++) {
                const int row = 4 * q + s;
                const float a = act[l][row * S + n0];   // A[i = e][k = q]: dz[row][n]
                if (l == 0) {
#pragma unroll
                    for (int kt = 0; kt < 2; kt++)
                        dw1[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, x0[row * kCgInStride + 16 * kt + e], dw1[kt], 0, 0, 0);
                } else {
#pragma unroll
                    for (int kt = 0; kt < GH; kt++)
                        dwl[l - 1][kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, act[l - 1][row * S + 16 * (half * GH + kt) + e],
                                                                              dwl[l - 1][kt], 0, 0, 0);
                    dbl[l - 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, 1.0f, dbl[l - 1], 0, 0, 0);
                }
            }
            if (l == 0) {
                __syncthreads();   // x0 and act[0] are free for the next tile
                break;
            }
            const f32x4 da = cg_da<H>(C.w[l], act[l], e, q, n0);   // da_{l-1}[row][k = n0] = sum_n dz_l[row][n] W_l[n][k]
            __syncthreads();   // every wave has read a_{l-1} (dW_l) and dz_l
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                float *p = act[l - 1] + (4 * q + reg) * S + n0;
                *p = *p > 0.0f ? da[reg] : 0.0f;
            }
            __syncthreads();
        }
    }

    // ---- the workgroup's partial set, torch layout; D[i = 4 q + reg][j = e]: neuron 16 wave + 4 q + reg, input 16 kt + e
    float *P = A.partial + (size_t)blockIdx.x * L::set + (size_t)c * L::stride;
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
        const int n = 16 * wave + 4 * q + reg;
#pragma unroll
        for (int l = 1; l < NL; l++) {
#pragma unroll
            for (int kt = 0; kt < GH; kt++) P[L::hw(l) + n * H + 16 * (half * GH + kt) + e] = dwl[l - 1][kt][reg];
            if (e == 0 && half == 0) P[L::hb(l) + n] = dbl[l - 1][reg];
        }
        if (half != 0) continue;
        cg_put_dw1<kTgtIn>(P, L::b1, dw1, reg, n, e);
    }
    if (half != 0) return;   // everything but its columns of the hidden dW is the first workgroup's to write
    if (t < H) P[L::wh + t] = dwo;
    else if (t == H) {
        P[L::bh] = dbo;
        A.partial[(size_t)blockIdx.x * L::set + L::grads + c] = loss;
    }
}

// grad[i] = partial[0][i] + partial[1][i] + ... in index order; loss = 0.5 (S_1 / B + S_2 / B) with S_c summed the same way
__global__ void __launch_bounds__(256)
k_critic_grad_reduce(const float *__restrict__ partial, int nwg, int set, int grads, int n, float *__restrict__ grad,
                     float *__restrict__ loss)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < grads) {
        float s[1];
        cg_sum_sets<1, true>(partial, nwg, set, i, s);
        grad[i] = s[0];
    }
    if (i == 0 && loss) {
        float s[2];
        cg_sum_sets<2, false>(partial, nwg, set, grads, s);
        loss[0] = 0.5f * (s[0] / (float)n + s[1] / (float)n);
    }
}

}  // namespace meshenv
