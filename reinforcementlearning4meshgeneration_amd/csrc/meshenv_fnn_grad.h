// meshenv_fnn_grad.h -- the loss of the supervised element-extraction network and its gradients (general/EBRD.py:272-320,
// train_ch3, one minibatch of B rows):
//
//   action, logits = model(x)                                                    # Policy, x [B][18]
//   loss = CrossEntropyLoss(reduction='sum')(logits, cls) + MSELoss(reduction='sum')(action, y[:, 1:])
//   loss.backward()
//
// with y [B][3] = (type, out0, out1) and cls = 2 type for type in {0, 0.5, 1} (map_type_to_tensors).  Two launches:
// k_fnn_grad, k_fnn_grad_reduce.  The network is that of meshenv_fnn.h: 18 -> 64 -> 128 -> 64 -> 32 -> 16 -> (2, 3), ReLU
// behind fc1 .. fc5.
//
// k_fnn_grad.  The idiom of k_ppo_grad for widths that differ from layer to layer: 16 rows per tile, v_mfma_f32_16x16x4_f32
// throughout, weights read from the LIVE [out][in] tensors (fg_first / fg_layer forward, buffer loads for da = dz W),
// EIGHT wavefronts per workgroup; blockIdx.x walks the tiles blockIdx.x, blockIdx.x + nwg, ... with its weight-gradient
// accumulators in registers.  All five activations of a tile stay in LDS (row strides K + 4: 36, 68, 132, 68, 36, 20 floats
// for x0, a1 .. a5) and become dz_l in place on the way back.  Per tile:
//
//   stage     x0 = the 16 rows (gathered through rows[] when given) padded to 32 columns, x0[21] = 1 (against which dW_1
//             yields db_1); the row's labels.  A row past B, a rows[] entry outside [0, N) or a type that is none of 0, 0.5,
//             1 is an INVALID row: its head gradient is exactly 0, so it adds nothing to any gradient or sum.
//   forward   a_l = relu(W_l a_{l-1} + b_l); layer l has N_l / 16 = 4, 8, 4, 2, 1 output tiles, wave w < N_l / 16 owns tile w
//   head      wave 0, one 16-wide tile: columns 0, 1 the action, 2..4 the logits.  log-softmax as torch computes it:
//             m = max, lse = logf((expf(l0 - m) + expf(l1 - m)) + expf(l2 - m)), logp_i = (l_i - m) - lse;
//             d_logit_i = expf(logp_i) - (i == cls), d_action_j = 2 (a_j - y_j); the row's terms ce = -logp_cls,
//             mse = d0 d0 + d1 d1, hit = argmax == cls (torch.argmax: fnn_argmax3)
//   backward  l = head, fc5, .., fc2: the layer's dW tiles (A = dz_l, B = a_{l-1}, K = the 16 rows) and db (B = 1) on the
//             waves listed at each step; da_{l-1} = dz_l W_l on one wave per 16 columns (fg_da); a barrier; a_{l-1} becomes
//             dz_{l-1} = (a_{l-1} > 0) da_{l-1} in place.  The head's da_5 is five fmaf per element on the vector unit.
//             Then dW_1 against x0.
//
// Accumulators of a wave: dW_2 4 + 1, dW_3 4 + 1, dW_4 1 + 1, dW_5 1 + 1, head 1 + 1, dW_1 1: 17 f32x4.
//
// Reduction order of a gradient element: one MFMA chain over the rows of the workgroup's tiles, then the partial sets in
// index order (k_fnn_grad_reduce).  The three row sums: one add chain over the rows of the workgroup's tiles, then the sets
// in index order.  No floating-point atomics: two calls on the same inputs give the same bits.
// The helpers of widths that differ between in and out (fg_*) are this header's own: none of meshenv_grad_tile.h's forward
// helpers is instantiated here, so the kernels that share those compile to what they were.
#pragma once

#include "meshenv_fnn.h"
#include "meshenv_grad_tile.h"

namespace meshenv {

constexpr int kFgWaves = 8;
constexpr int kFgThreads = 64 * kFgWaves;
constexpr int kFgLayers = 7;      // fc1 .. fc5, action_head, type_head: weight and bias each
constexpr int kFgSums = 3;        // row sums behind a partial set: cross entropy, squared error, rows whose argmax is cls
constexpr int kFgOut = 4;         // loss, classification loss, regression loss, hits

// The gradient set, torch layout, in MESHENV_FNN_TENSORS' order; padded to a multiple of 64 floats.  A partial set carries
// the three row sums after it.
struct FgLayout {
    static constexpr int w1 = 0, b1 = w1 + 64 * 18;
    static constexpr int w2 = b1 + 64, b2 = w2 + 128 * 64;
    static constexpr int w3 = b2 + 128, b3 = w3 + 64 * 128;
    static constexpr int w4 = b3 + 64, b4 = w4 + 32 * 64;
    static constexpr int w5 = b4 + 32, b5 = w5 + 16 * 32;
    static constexpr int wa = b5 + 16, ba = wa + kFnnAction * 16;
    static constexpr int wt = ba + kFnnAction, bt = wt + kFnnTypes * 16;
    static constexpr int params = bt + kFnnTypes;
    static constexpr int stride = (params + 63) & ~63;
    static constexpr int set = stride + 64;
};
static_assert(FgLayout::params == 20485 && FgLayout::stride == 20544, "the fourteen tensors of Policy");

struct FgArgs {
    int n, N, nwg;               // rows of the minibatch, rows of x / y, workgroups
    const float *x, *y;          // [N][18], [N][3]
    const int32_t *rows;         // [n] or nullptr: row i of the minibatch is x[rows[i]], y[rows[i]]
    const float *w[kFgLayers], *b[kFgLayers];
    float *partial;              // [nwg][FgLayout::set]
};

// relu(W_1 x0 + b_1) of the lane's neuron n0 for rows 4 q + reg: W_1 [64][18] read a float at a time (its rows are 72 bytes), of
// whose K = 32 the columns >= 18 (the padding and the column of ones) are read as 0; two accumulators over the two 16-groups
__device__ __forceinline__ f32x4 fg_first(const float *__restrict__ w1, const float *__restrict__ b1, const float *x0, int e, int q, int n0)
{
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    const unsigned o1 = (unsigned)(n0 * kCgObs + 4 * q);
    const float *xr = x0 + e * kCgInStride + 4 * q;
    const f32x4 a0 = *reinterpret_cast<const f32x4 *>(xr), a1 = *reinterpret_cast<const f32x4 *>(xr + 16);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const float w0 = w1[o1 + j];                                              // k = 4 q + j < 16
        const float w16 = 16 + 4 * q + j < kCgObs ? w1[o1 + 16 + j] : 0.0f;
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[j], w0, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[j], w16, acc1, 0, 0, 0);
    }
    const float b = b1[(unsigned)n0];
    f32x4 r;
#pragma unroll
    for (int reg = 0; reg < 4; reg++) r[reg] = fmaxf((acc0[reg] + acc1[reg]) + b, 0.0f);
    return r;
}

// relu(W x + b) of the lane's neuron n0 for rows 4 q + reg: x 16 rows of K activations in LDS (stride K + 4), W [N][K] for
// any N > n0, read 16 bytes at a time; accumulators alternate over the 16-groups of k, MFMA step (g, j) taking k = 16 g + 4 q + j
template <int K>
__device__ __forceinline__ f32x4 fg_layer(const float *__restrict__ w, const float *__restrict__ bias, const float *x, int e, int q, int n0)
{
    constexpr int G = K / 16, S = K + 4;
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    const float *xr = x + e * S + 4 * q;
    const unsigned off = (unsigned)(n0 * K + 4 * q);
#pragma unroll
    for (int g = 0; g < G; g++) {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(xr + 16 * g);
        const f32x4 b = *reinterpret_cast<const f32x4 *>((w + 16 * g) + off);
#pragma unroll
        for (int j = 0; j < 4; j++) acc[g & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], acc[g & 1], 0, 0, 0);
    }
    const float b = bias[(unsigned)n0];
    f32x4 r;
#pragma unroll
    for (int reg = 0; reg < 4; reg++) r[reg] = fmaxf((acc[0][reg] + acc[1][reg]) + b, 0.0f);
    return r;
}

// v[reg] -> buf[row = 4 q + reg][n0] (row stride s)
__device__ __forceinline__ void fg_store(float *buf, int s, const f32x4 &v, int q, int n0)
{
#pragma unroll
    for (int reg = 0; reg < 4; reg++) buf[(4 * q + reg) * s + n0] = v[reg];
}

// acc += dz[:, 16 nt + i]^T ap[:, 16 kt + j] over the tile's 16 rows: D[i = 4 q + reg][j = e] is dW[16 nt + 4 q + reg][16 kt + e]
__device__ __forceinline__ void fg_dw(f32x4 &acc, const float *dz, int sz, int nt, const float *ap, int sp, int kt, int q, int e)
{
#pragma unroll
    for (int s = 0; s < 4; s++) {
        const int row = 4 * q + s;   // A[i = e][k = q] = dz[row][16 nt + e], B[k = q][j = e] = ap[row][16 kt + e]
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(dz[row * sz + 16 * nt + e], ap[row * sp + 16 * kt + e], acc, 0, 0, 0);
    }
}

// acc += the column sums of dz[:, 16 nt + i]: D[i = 4 q + reg][any j] is db[16 nt + 4 q + reg]
__device__ __forceinline__ void fg_db(f32x4 &acc, const float *dz, int sz, int nt, int q, int e)
{
#pragma unroll
    for (int s = 0; s < 4; s++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(dz[(4 * q + s) * sz + 16 * nt + e], 1.0f, acc, 0, 0, 0);
}

// da[row = 4 q + reg][k0] = sum_n dz[row][n] W[n][k0] for a RECTANGULAR W [N][K] (cg_da is the square one): the lane's
// column k0 = 16 c + e, dz rows of stride N + 4; accumulators alternate over the 16-groups of n (N = 16: one group, the
// second stays 0).  W is read by columns through buffer loads: one descriptor of N K floats, one lane offset.
template <int N, int K>
__device__ __forceinline__ f32x4 fg_da(const float *w, const float *dz, int e, int q, int k0)
{
    constexpr int G = N / 16, S = N + 4;
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    const float *xr = dz + e * S + 4 * q;
    const __amdgpu_buffer_rsrc_t wl = __builtin_amdgcn_make_buffer_rsrc((void *)w, 0, N * K * 4, kCgBufferFlags);
    const int voff = (4 * q * K + k0) * 4;
#pragma unroll
    for (int g = 0; g < G; g++) {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(xr + 16 * g);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            // W[16 g + 4 q + j][k0]
            const float b = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(wl, voff, (16 * g + j) * K * 4, 0));
            acc[g & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b, acc[g & 1], 0, 0, 0);
        }
    }
    f32x4 r;
#pragma unroll
    for (int reg = 0; reg < 4; reg++) r[reg] = acc[0][reg] + acc[1][reg];
    return r;
}

// a[row = 4 q + reg][col] <- (a > 0) da[reg]: the kept ReLU activation becomes dz in place
__device__ __forceinline__ void fg_back(float *a, int s, const f32x4 &da, int q, int col)
{
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
        float *p = a + (4 * q + reg) * s + col;
        *p = *p > 0.0f ? da[reg] : 0.0f;
    }
}

// a dW tile -> the partial set, torch layout [N][K]
__device__ __forceinline__ void fg_put(float *W, int K, int nt, int kt, const f32x4 &acc, int q, int e)
{
#pragma unroll
    for (int reg = 0; reg < 4; reg++) W[(16 * nt + 4 * q + reg) * K + 16 * kt + e] = acc[reg];
}

__device__ __forceinline__ void fg_put_bias(float *B, int nt, const f32x4 &acc, int q, int e)
{
    if (e != 0) return;
#pragma unroll
    for (int reg = 0; reg < 4; reg++) B[16 * nt + 4 * q + reg] = acc[reg];
}

__global__ void __launch_bounds__(kFgThreads)
k_fnn_grad(FgArgs A)
{
    constexpr int S0 = kCgInStride, S1 = 64 + 4, S2 = 128 + 4, S3 = 64 + 4, S4 = 32 + 4, S5 = 16 + 4;
    using L = FgLayout;
    __shared__ __attribute__((aligned(16))) float x0[kCgRows * S0];
    __shared__ __attribute__((aligned(16))) float a1[kCgRows * S1];
    __shared__ __attribute__((aligned(16))) float a2[kCgRows * S2];
    __shared__ __attribute__((aligned(16))) float a3[kCgRows * S3];
    __shared__ __attribute__((aligned(16))) float a4[kCgRows * S4];
    __shared__ __attribute__((aligned(16))) float a5[kCgRows * S5];
    __shared__ __attribute__((aligned(16))) float dh[kCgRows * S5];   // the head gradient: columns 0, 1 action, 2..4 logits, 5..15 zero
    __shared__ float ys[kCgRows * 4];   // the row's labels: type, out0, out1, 1 where the row exists
    __shared__ float st[kCgRows * 4];   // the row's terms: cross entropy, squared error, hit
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int e = lane & 15, q = lane >> 4, n0 = 16 * wave + e;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 dw1 = zero, dw2[4] = {zero, zero, zero, zero}, db2 = zero, dw3[4] = {zero, zero, zero, zero}, db3 = zero;
    f32x4 dw4 = zero, db4 = zero, dw5 = zero, db5 = zero, dwh = zero, dbh = zero;
    float sacc = 0.0f;   // threads 64..66: the three row sums
    const int tiles = (A.n + kCgRows - 1) / kCgRows;
    if (t < kCgRows * S5) dh[t] = 0.0f;   // columns 5..15 stay zero; the first barrier of the tile loop publishes them

    for (int tile = blockIdx.x; tile < tiles; tile += A.nwg) {
        const int row0 = tile * kCgRows;
        {   // ---- stage: thread (r, k) one element of x0; the threads of columns 28..31 the row's labels
            const int r = t >> 5, k = t & 31, gr = row0 + r;
            int src = -1;
            if (gr < A.n) src = A.rows ? A.rows[gr] : gr;
            const bool have = (unsigned)src < (unsigned)A.N;
            float v = 0.0f;
            if (k == kCgOnes) v = 1.0f;
            else if (have && k < kCgObs) v = A.x[(size_t)src * kCgObs + k];
            x0[r * S0 + k] = v;
            if (k >= 28) {
                const int c = k - 28;
                ys[r * 4 + c] = c == 3 ? (have ? 1.0f : 0.0f) : (have ? A.y[(size_t)src * 3 + c] : 0.0f);
            }
        }
        __syncthreads();
        // ---- forward
        if (wave < 4) fg_store(a1, S1, fg_first(A.w[0], A.b[0], x0, e, q, n0), q, n0);
        __syncthreads();
        fg_store(a2, S2, fg_layer<64>(A.w[1], A.b[1], a1, e, q, n0), q, n0);
        __syncthreads();
        if (wave < 4) fg_store(a3, S3, fg_layer<128>(A.w[2], A.b[2], a2, e, q, n0), q, n0);
        __syncthreads();
        if (wave < 2) fg_store(a4, S4, fg_layer<64>(A.w[3], A.b[3], a3, e, q, n0), q, n0);
        __syncthreads();
        if (wave == 0) fg_store(a5, S5, fg_layer<32>(A.w[4], A.b[4], a4, e, q, n0), q, n0);
        __syncthreads();
        // ---- the head tile and its gradient (wave 0): column e < 2 a row of action_head, 2 <= e < 5 of type_head
        if (wave == 0) {
            const bool col = e < kFnnAction + kFnnTypes;
            const float *wr = e < kFnnAction ? A.w[5] + e * 16 : A.w[6] + (col ? e - kFnnAction : 0) * 16;
            const f32x4 bw = col ? *reinterpret_cast<const f32x4 *>(wr + 4 * q) : zero;
            const f32x4 ax = *reinterpret_cast<const f32x4 *>(a5 + e * S5 + 4 * q);
            f32x4 acc = zero;
#pragma unroll
            for (int j = 0; j < 4; j++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ax[j], bw[j], acc, 0, 0, 0);
            const float bh = e < kFnnAction ? A.b[5][e] : col ? A.b[6][e - kFnnAction] : 0.0f;
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int row = 4 * q + reg, first = lane & 48;
                const float v = acc[reg] + bh;   // head[row][e]; the row's five values sit in lanes first .. first + 4
                const float p0 = __shfl(v, first, 64), p1 = __shfl(v, first + 1, 64);
                const float l0 = __shfl(v, first + 2, 64), l1 = __shfl(v, first + 3, 64), l2 = __shfl(v, first + 4, 64);
                const float ty = ys[row * 4];
                const int cls = ty == 0.0f ? 0 : ty == 0.5f ? 1 : ty == 1.0f ? 2 : -1;
                const bool ok = ys[row * 4 + 3] != 0.0f && cls >= 0;
                const float m = fmaxf(fmaxf(l0, l1), l2);
                const float lse = logf((expf(l0 - m) + expf(l1 - m)) + expf(l2 - m));
                const float lp0 = (l0 - m) - lse, lp1 = (l1 - m) - lse, lp2 = (l2 - m) - lse;
                const float d0 = p0 - ys[row * 4 + 1], d1 = p1 - ys[row * 4 + 2];
                float d = 0.0f;
                if (ok) {
                    if (e == 0) d = 2.0f * d0;
                    else if (e == 1) d = 2.0f * d1;
                    else if (col) d = expf(e == 2 ? lp0 : e == 3 ? lp1 : lp2) - (e - kFnnAction == cls ? 1.0f : 0.0f);
                }
                if (col) dh[row * S5 + e] = d;
                else if (e == 5) {
                    st[row * 4] = ok ? -(cls == 0 ? lp0 : cls == 1 ? lp1 : lp2) : 0.0f;
                    st[row * 4 + 1] = ok ? d0 * d0 + d1 * d1 : 0.0f;
                    st[row * 4 + 2] = ok && fnn_argmax3(l0, l1, l2) == cls ? 1.0f : 0.0f;
                }
            }
        }
        __syncthreads();
        // ---- head: dW_h, db_h (wave 0), the row sums (wave 1), da_5 on the vector unit (waves 4..7, one element each)
        const int r5 = (t >> 4) & 15, k5 = t & 15;
        float v5 = 0.0f;
        if (wave == 0) {
            fg_dw(dwh, dh, S5, 0, a5, S5, 0, q, e);
            fg_db(dbh, dh, S5, 0, q, e);
        } else if (wave == 1) {
            if (lane < kFgSums)
#pragma unroll
                for (int row = 0; row < kCgRows; row++) sacc = sacc + st[row * 4 + lane];
        } else if (wave >= 4) {
            v5 = dh[r5 * S5] * A.w[5][k5];
            v5 = fmaf(dh[r5 * S5 + 1], A.w[5][16 + k5], v5);
#pragma unroll
            for (int c = 0; c < kFnnTypes; c++) v5 = fmaf(dh[r5 * S5 + kFnnAction + c], A.w[6][16 * c + k5], v5);
        }
        __syncthreads();   // dW_h has read a_5
        if (wave >= 4) {
            float *p = a5 + r5 * S5 + k5;
            *p = *p > 0.0f ? v5 : 0.0f;
        }
        __syncthreads();
        // ---- fc5 [16][32]: dW_5 on waves 0, 1 (one input tile each), db_5 on wave 2, da_4 on waves 4, 5
        {
            f32x4 da = zero;
            if (wave < 2) fg_dw(dw5, a5, S5, 0, a4, S4, wave, q, e);
            else if (wave == 2) fg_db(db5, a5, S5, 0, q, e);
            else if (wave == 4 || wave == 5) da = fg_da<16, 32>(A.w[4], a5, e, q, 16 * (wave - 4) + e);
            __syncthreads();
            if (wave == 4 || wave == 5) fg_back(a4, S4, da, q, 16 * (wave - 4) + e);
        }
        __syncthreads();
        // ---- fc4 [32][64]: dW_4 tile (wave & 1, wave >> 1), db_4 on waves 0, 1, da_3 on waves 4..7
        {
            f32x4 da = zero;
            fg_dw(dw4, a4, S4, wave & 1, a3, S3, wave >> 1, q, e);
            if (wave < 2) fg_db(db4, a4, S4, wave, q, e);
            else if (wave >= 4) da = fg_da<32, 64>(A.w[3], a4, e, q, 16 * (wave - 4) + e);
            __syncthreads();
            if (wave >= 4) fg_back(a3, S3, da, q, 16 * (wave - 4) + e);
        }
        __syncthreads();
        // ---- fc3 [64][128]: dW_3 tiles (wave & 3, 4 (wave >> 2) + i), db_3 on waves 0..3, da_2 on every wave
        {
#pragma unroll
            for (int i = 0; i < 4; i++) fg_dw(dw3[i], a3, S3, wave & 3, a2, S2, 4 * (wave >> 2) + i, q, e);
            if (wave < 4) fg_db(db3, a3, S3, wave, q, e);
            const f32x4 da = fg_da<64, 128>(A.w[2], a3, e, q, n0);
            __syncthreads();
            fg_back(a2, S2, da, q, n0);
        }
        __syncthreads();
        // ---- fc2 [128][64]: dW_2 tiles (wave, i), db_2, da_1 on waves 0..3
        {
            f32x4 da = zero;
#pragma unroll
            for (int i = 0; i < 4; i++) fg_dw(dw2[i], a2, S2, wave, a1, S1, i, q, e);
            fg_db(db2, a2, S2, wave, q, e);
            if (wave < 4) da = fg_da<128, 64>(A.w[1], a2, e, q, n0);
            __syncthreads();
            if (wave < 4) fg_back(a1, S1, da, q, n0);
        }
        __syncthreads();
        // ---- fc1 [64][18]: dW_1 tile (wave & 3, wave >> 2) and, against the column of ones, db_1
        fg_dw(dw1, a1, S1, wave & 3, x0, S0, wave >> 2, q, e);
        __syncthreads();   // every buffer is free for the next tile
    }

    // ---- the workgroup's partial set, torch layout
    float *P = A.partial + (size_t)blockIdx.x * L::set;
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {   // fc1: inputs k < 18 the weight, k == kCgOnes the bias, the rest padding
        const int n = 16 * (wave & 3) + 4 * q + reg, k = 16 * (wave >> 2) + e;
        if (k < kCgObs) P[L::w1 + n * kCgObs + k] = dw1[reg];
        else if (k == kCgOnes) P[L::b1 + n] = dw1[reg];
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        fg_put(P + L::w2, 64, wave, i, dw2[i], q, e);
        fg_put(P + L::w3, 128, wave & 3, 4 * (wave >> 2) + i, dw3[i], q, e);
    }
    fg_put_bias(P + L::b2, wave, db2, q, e);
    if (wave < 4) fg_put_bias(P + L::b3, wave, db3, q, e);
    fg_put(P + L::w4, 64, wave & 1, wave >> 1, dw4, q, e);
    if (wave < 2) {
        fg_put_bias(P + L::b4, wave, db4, q, e);
        fg_put(P + L::w5, 32, 0, wave, dw5, q, e);
    } else if (wave == 2) {
        fg_put_bias(P + L::b5, 0, db5, q, e);
    }
    if (wave == 0) {   // the head tile: neurons 0, 1 action_head, 2..4 type_head
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int n = 4 * q + reg;
            if (n < kFnnAction) {
                P[L::wa + n * 16 + e] = dwh[reg];
                if (e == 0) P[L::ba + n] = dbh[reg];
            } else if (n < kFnnAction + kFnnTypes) {
                P[L::wt + (n - kFnnAction) * 16 + e] = dwh[reg];
                if (e == 0) P[L::bt + (n - kFnnAction)] = dbh[reg];
            }
        }
    } else if (wave == 1 && lane < kFgSums) {
        P[L::stride + lane] = sacc;
    }
}

// grad[i] = partial[0][i] + partial[1][i] + ... in index order; the three row sums the same way, then out[0..3] = loss =
// ce + mse, ce, mse, hits, and accum[k] = accum[k] + out[k] (nullable; this thread is its one writer)
__global__ void __launch_bounds__(256)
k_fnn_grad_reduce(const float *__restrict__ partial, int nwg, float *__restrict__ grad, float *__restrict__ out, float *__restrict__ accum)
{
    using L = FgLayout;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < L::params) {
        float s[1];
        cg_sum_sets<1, true>(partial, nwg, L::set, i, s);
        grad[i] = s[0];
    }
    if (i == 0) {
        float s[kFgSums];
        cg_sum_sets<kFgSums, false>(partial, nwg, L::set, L::stride, s);
        const float o[kFgOut] = {s[0] + s[1], s[0], s[1], s[2]};
#pragma unroll
        for (int k = 0; k < kFgOut; k++) {
            out[k] = o[k];
            if (accum) accum[k] = accum[k] + o[k];
        }
    }
}

}  // namespace meshenv
