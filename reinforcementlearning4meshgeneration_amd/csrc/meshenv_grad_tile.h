// meshenv_grad_tile.h -- the 16-row tile primitives of the gradient kernels (k_critic_grad, k_actor_grad, k_td3_actor_grad,
// k_ppo_grad and their *_reduce kernels): one definition each of what every one of them does per tile.
//
// The tiling they share.  A workgroup has H / 16 wavefronts and handles 16 samples (rows) per tile; wave w owns neurons
// [16 w, 16 w + 16) of every hidden layer, lane (e = lane & 15, q = lane >> 4) its neuron n0 = 16 w + e.  Everything is
// v_mfma_f32_16x16x4_f32 (exact f32) with two accumulators over the even / odd 16-groups of k, summed at the end: MFMA step
// (group g, j) of the lane takes k = 16 g + 4 q + j, and register reg of the result is D[row = 4 q + reg][col = e].  The
// weights are read from the LIVE torch tensors ([out][in] row-major).  Activations live in LDS in their natural order, row
// stride H + 4 floats (the 16 rows of a quarter-wave on distinct banks); the input rows x0 have K = 32 columns at stride
// kCgInStride: the observation, columns 18..20 for the action where there is one, a 1 in column kCgOnes (against which the
// first layer's weight gradient product yields its bias gradient), zeros elsewhere and in the rows past n.
//
// Every helper is inlined into its kernel; none contains a barrier.
#pragma once

#include "meshenv_target.h"

namespace meshenv {

constexpr int kCgRows = 16;       // samples per tile = MFMA K of the weight gradient
constexpr int kCgObs = 18;        // observation columns of the input rows
constexpr int kCgInStride = 36;   // LDS row stride of the input rows (21 inputs padded to 32)
constexpr int kCgOnes = 21;       // the column of ones in the input rows: the first layer's bias gradient
constexpr int kCgMaxGroups = 128; // workgroups per network; the workspace holds that many partial sets
constexpr int kCgBufferFlags = 0x00020000;   // word 3 of a raw 32-bit buffer descriptor on gfx9

// x0 <- the 16 input rows of the tile at row0, by NT threads (t = threadIdx.x): obs [n][18], with ACTIONS columns 18..20 from
// actions [n][3] (otherwise they stay 0 and actions is not read), the ones column, zeros past n
template <int NT, bool ACTIONS>
__device__ __forceinline__ void cg_stage(float *x0, const float *obs, const float *actions, int row0, int n, int t)
{
    for (int i = t; i < kCgRows * 32; i += NT) {
        const int r = i >> 5, k = i & 31, gr = row0 + r;
        float v = 0.0f;
        if (k == kCgOnes) v = 1.0f;
        else if (gr < n && k < kCgObs) v = obs[(unsigned)(gr * kCgObs + k)];
        else if (ACTIONS && gr < n && k < kTgtIn) v = actions[(unsigned)(gr * 3 + (k - kCgObs))];
        x0[r * kCgInStride + k] = v;
    }
}

// acc0 / acc1 += x W^T over K = 16 G inputs for the lane's neuron n: w = W (uniform), off = n * K + 4 q (one 32-bit lane
// offset against a scalar base per load), valid: false reads a zero row; xr = &x[e][4 q]
template <int G>
__device__ __forceinline__ void cg_dense(const float *__restrict__ w, unsigned off, bool valid, const float *xr, f32x4 &acc0,
                                         f32x4 &acc1)
{
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int g = 0; g < G; g += 2) {
        const f32x4 a0 = *reinterpret_cast<const f32x4 *>(xr + 16 * g);
        const f32x4 a1 = *reinterpret_cast<const f32x4 *>(xr + 16 * g + 16);
        const f32x4 b0 = valid ? *reinterpret_cast<const f32x4 *>((w + 16 * g) + off) : zero;
        const f32x4 b1 = valid ? *reinterpret_cast<const f32x4 *>((w + 16 * g + 16) + off) : zero;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[j], b0[j], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[j], b1[j], acc1, 0, 0, 0);
        }
    }
}

// acc0 / acc1 += x0 W_1^T for the lane's neuron n0: W_1 [H][KIN], of whose K = 32 the columns >= KIN (the padding and the
// column of ones) are read as 0
template <int KIN>
__device__ __forceinline__ void cg_first(const float *w1, const float *x0, int e, int q, int n0, f32x4 &acc0, f32x4 &acc1)
{
    const unsigned o1 = (unsigned)(n0 * KIN + 4 * q);
    const float *xr = x0 + e * kCgInStride + 4 * q;
    const f32x4 a0 = *reinterpret_cast<const f32x4 *>(xr), a1 = *reinterpret_cast<const f32x4 *>(xr + 16);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const float b0 = (w1 + j)[o1];                                      // k = 4 q + j < 16
        const float b1 = 16 + 4 * q + j < KIN ? (w1 + 16 + j)[o1] : 0.0f;   // the padding and the column of ones
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[j], b0, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[j], b1, acc1, 0, 0, 0);
    }
}

// act((acc0 + acc1) + bias[n0]) for rows 4 q + reg: the epilogue of a hidden layer (ReLU is fmaxf(x, 0.0f))
template <int ACT>
__device__ __forceinline__ f32x4 cg_bias_act(const f32x4 &acc0, const f32x4 &acc1, const float *bias, int n0)
{
    const float b = bias[(unsigned)n0];
    f32x4 r;
#pragma unroll
    for (int reg = 0; reg < 4; reg++) r[reg] = policy_act<ACT>((acc0[reg] + acc1[reg]) + b);
    return r;
}

// act(W_1 x0 + b_1) of the lane's neuron n0 for rows 4 q + reg
template <int KIN, int ACT>
__device__ __forceinline__ f32x4 cg_first_layer(const float *w1, const float *b1, const float *x0, int e, int q, int n0)
{
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    cg_first<KIN>(w1, x0, e, q, n0, acc0, acc1);
    return cg_bias_act<ACT>(acc0, acc1, b1, n0);
}

// act(W x + b) of the lane's neuron n0 for rows 4 q + reg; x: 16 rows of H activations in LDS
template <int H, int ACT>
__device__ __forceinline__ f32x4 cg_hidden_layer(const float *w, const float *b, const float *x, int e, int q, int n0)
{
    constexpr int G = H / 16, S = H + 4;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    cg_dense<G>(w, (unsigned)(n0 * H + 4 * q), true, x + e * S + 4 * q, acc0, acc1);
    return cg_bias_act<ACT>(acc0, acc1, b, n0);
}

// v[reg] -> buf[row = 4 q + reg][n0], and to out [n][H] (nullable) for the rows below n
template <int H>
__device__ __forceinline__ void cg_store(float *buf, float *out, const f32x4 &v, int row0, int n, int q, int n0)
{
    constexpr int S = H + 4;
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {   // D[row = 4 q + reg][col = e]
        const int row = 4 * q + reg;
        buf[row * S + n0] = v[reg];
        if (out && row0 + row < n) out[(unsigned)((row0 + row) * H + n0)] = v[reg];
    }
}

// da[row = 4 q + reg][k = n0] = sum_n dz[row][n] W[n][k] for the wave's 16 columns: two accumulators over even / odd
// 16-groups of n; W [H][H] read by columns, 64 bytes per row and quarter-wave, through buffer loads: one descriptor and one
// lane offset for all 4 G of them (a flat address per load would cost two registers each); reads past the H x H matrix
// cannot happen and would return 0
template <int H>
__device__ __forceinline__ f32x4 cg_da(const float *w, const float *dz, int e, int q, int n0)
{
    constexpr int G = H / 16, S = H + 4;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    const float *xr = dz + e * S + 4 * q;
    const __amdgpu_buffer_rsrc_t wl = __builtin_amdgcn_make_buffer_rsrc((void *)w, 0, H * H * 4, kCgBufferFlags);
    const int voff = (4 * q * H + n0) * 4;
#pragma unroll
    for (int g = 0; g < G; g += 2) {
        const f32x4 a0 = *reinterpret_cast<const f32x4 *>(xr + 16 * g);
        const f32x4 a1 = *reinterpret_cast<const f32x4 *>(xr + 16 * g + 16);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            // W[16 g + 4 q + j][n0]; the builtin returns the 32 bits as an integer
            const float b0 = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(wl, voff, (16 * g + j) * H * 4, 0));
            const float b1 = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(wl, voff, (16 * g + 16 + j) * H * 4, 0));
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[j], b0, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[j], b1, acc1, 0, 0, 0);
        }
    }
    f32x4 r;
#pragma unroll
    for (int reg = 0; reg < 4; reg++) r[reg] = acc0[reg] + acc1[reg];
    return r;
}

// Register reg of the two dW_1 accumulators (neuron n, inputs 16 kt + e) -> the partial set P, torch layout: input k < KIN
// is the weight w1 [H][KIN] at the set's start, k == kCgOnes the bias at P[b1 + n], the other columns are padding
template <int KIN>
__device__ __forceinline__ void cg_put_dw1(float *P, int b1, const f32x4 (&dw1)[2], int reg, int n, int e)
{
#pragma unroll
    for (int kt = 0; kt < 2; kt++) {
        const int k = 16 * kt + e;
        if (k < KIN) P[n * KIN + k] = dw1[kt][reg];
        else if (k == kCgOnes) P[b1 + n] = dw1[kt][reg];
    }
}

// s[k] = element i + k of the partial sets (set floats apart) summed in index order: partial[0] + partial[1] + ... + partial[nwg - 1];
// UNROLL4: the gradient path's #pragma unroll 4, the loss sums run without
template <int K, bool UNROLL4>
__device__ __forceinline__ void cg_sum_sets(const float *__restrict__ partial, int nwg, int set, int i, float (&s)[K])
{
#pragma unroll
    for (int k = 0; k < K; k++) s[k] = partial[i + k];
    if constexpr (UNROLL4) {
#pragma unroll 4
        for (int w = 1; w < nwg; w++)
#pragma unroll
            for (int k = 0; k < K; k++) s[k] = s[k] + partial[(size_t)w * set + i + k];
    } else {
        for (int w = 1; w < nwg; w++)
#pragma unroll
            for (int k = 0; k < K; k++) s[k] = s[k] + partial[(size_t)w * set + i + k];
    }
}

}  // namespace meshenv
