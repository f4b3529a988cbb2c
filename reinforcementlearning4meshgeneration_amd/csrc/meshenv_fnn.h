// meshenv_fnn.h -- forward of the supervised element-extraction network (the reference's "FNN mesher", general/EBRD.py:85-91,
// 120-126: Policy) and the bookkeeping of the closed meshing loop around k_move (EBRD.py:525-548).
//
//   x1 = relu(fc1 x)  18 -> 64      x2 = relu(fc2 x1)  64 -> 128     x3 = relu(fc3 x2)  128 -> 64
//   x4 = relu(fc4 x3) 64 -> 32      x5 = relu(fc5 x4)  32 -> 16      action = action_head x5 (2), type_values = type_head x5 (3)
//
// k_fnn_forward gives, per environment, what EBRD.get_action (:174-177) hands to env.move:
//   points[e] = (double)action[e][0..1]       the widening tolist() performs; nothing is computed in float64
//   types[e]  = argmax(type_values[e]) / 2.0  in {0.0, 0.5, 1.0}: round(., 2) of the caller (:544) is the identity on these
// argmax is torch's: the LOWEST index among equal maxima; a NaN logit counts as the maximum and the FIRST NaN wins.
//
// Layout.  The MFMA tiling of meshenv_actor.h / meshenv_policy.h (v_mfma_f32_16x16x4_f32: exact f32, 16 environments = MFMA M
// per workgroup; LayerRegs / load_layer / policy_layer and the k-permuted LDS rows of stride K + 4 are theirs).  Every width is
// a multiple of 16: the layers have 4, 8, 4, 2, 1 output tiles and the two heads share one (columns 0-1 the action, 2-4 the
// type logits).  What the non-uniform widths add is the tile-to-wave table below and the K = 16 product of the head tile,
// whose single k-group gives policy_layer's two-accumulator split nothing to split (fnn_head_tile).
//
// Waves.  FOUR wavefronts per workgroup, one per SIMD.  Wave w owns tile w of fc1, tiles w and w + 4 of fc2, tile w of fc3,
// tile w of fc4 (w < 2), and wave 0 owns fc5 and the head tile.  Registers: a tile of a K-input layer is K / 4 floats per
// lane, so wave 0 holds 8 + 2 * 16 + 32 + 16 + 8 + 4 = 100 floats of weights (waves 2, 3: 72) -- ALL of them requested before
// the observations are read, so the kernel pays one memory latency, not one per layer.  The compiler's figures: 116 VGPRs + 16
// AGPRs, no scratch, i.e. 136 allocated registers and three waves per SIMD -- three workgroups per CU, more than the 16.5 KB
// of LDS each or a batch of 4096 envs (one workgroup per CU, a wave has its SIMD to itself) ever asks for.  Eight waves would
// halve fc2's two tiles per wave (32 of ~100 MFMAs on the longest wave) and double the waves that only wait at the five
// barriers; the layers behind fc3 have fewer tiles than even four waves.
// LDS: two activation buffers of 16 rows x 132 floats (the widest row, K = 128, plus 4), 16.5 KB; a layer reads one and
// writes the other, each in the stride K + 4 of the layer that reads it (36, 68, 132, 68, 36, 20 floats: 16 rows x 16 B on
// distinct banks for every one of them).
//
// finished (nullable): where finished[e] != 0 every requested output of env e is still written, as ZEROS -- the rows of a
// finished environment in the histories of meshenv_move_fnn_multi; the network's value on a frozen observation is of no use
// to anyone, and the buffers stay defined.
#pragma once

#include "meshenv_kernels.h"
#include "meshenv_policy.h"

namespace meshenv {

constexpr int kFnnEnvs = 16;      // environments per workgroup = MFMA M
constexpr int kFnnWaves = 4;
constexpr int kFnnLayers = 6;     // fc1 .. fc5 and the shared head tile
constexpr int kFnnAction = 2, kFnnTypes = 3;
constexpr int kFnnRow = 132;      // floats per LDS row of an activation buffer

// inputs (K, padded to a multiple of 16), outputs and 16-wide output tiles of the six layers
__host__ __device__ constexpr int fnn_k(int l) { return l == 0 ? 32 : l == 1 ? 64 : l == 2 ? 128 : l == 3 ? 64 : l == 4 ? 32 : 16; }
__host__ __device__ constexpr int fnn_in(int l) { return l == 0 ? 18 : fnn_k(l); }
__host__ __device__ constexpr int fnn_out(int l) { return l == 0 ? 64 : l == 1 ? 128 : l == 2 ? 64 : l == 3 ? 32 : l == 4 ? 16 : 5; }
__host__ __device__ constexpr int fnn_tiles(int l) { return (fnn_out(l) + 15) / 16; }
// floats of layer l in the packed buffer: the weight in the B-operand order [tile][K / 16][lane 64][4], then the bias [16 tiles]
__host__ __device__ constexpr int fnn_w_floats(int l) { return fnn_tiles(l) * fnn_k(l) * 16; }
__host__ __device__ constexpr int fnn_w_offset(int l)
{
    int at = 0;
    for (int i = 0; i < l; i++) at += fnn_w_floats(i) + 16 * fnn_tiles(i);
    return at;
}
__host__ __device__ constexpr int fnn_b_offset(int l) { return fnn_w_offset(l) + fnn_w_floats(l); }
constexpr int kFnnPackedFloats = fnn_b_offset(kFnnLayers - 1) + 16;
// the same as compile-time constants (device code: no address arithmetic left to run)
template <int L>
struct FnnAt {
    static constexpr int w = fnn_w_offset(L), b = fnn_b_offset(L);
};
static_assert(kFnnPackedFloats == 21568, "include/meshenv_fnn.h: MESHENV_FNN_PACKED_FLOATS");

struct FnnArgs {
    const float *packed;        // [kFnnPackedFloats]
    int n;
    const float *obs;           // [n][18]
    const uint8_t *finished;    // [n] or nullptr
    double *points;             // [n][2]   every output nullable
    double *types;              // [n]
    float *actions;             // [n][2]
    float *logits;              // [n][3]
    float *obs_copy;            // [n][18]: the observation the forward read (zeros where finished)
};

// torch.argmax over the three type logits
__device__ __forceinline__ int fnn_argmax3(float l0, float l1, float l2)
{
    int best = 0;
    float top = l0;
    if (!(top != top) && (l1 > top || l1 != l1)) { best = 1; top = l1; }
    if (!(top != top) && (l2 > top || l2 != l2)) best = 2;
    return best;
}

// the head tile: a K = 16 product is ONE k-group of four MFMA steps on one accumulator
__device__ __forceinline__ f32x4 fnn_head_tile(const LayerRegs<1> &r, const float *x, int lane)
{
    const int e = lane & 15, q = lane >> 4;
    const f32x4 a = *reinterpret_cast<const f32x4 *>(x + e * (16 + 4) + q * 4);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; j++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], r.w[0][j], acc, 0, 0, 0);
    return acc;
}

__global__ void __launch_bounds__(64 * kFnnWaves)
k_fnn_forward(FnnArgs A)
{
    __shared__ __attribute__((aligned(16))) float bufA[kFnnEnvs * kFnnRow];
    __shared__ __attribute__((aligned(16))) float bufB[kFnnEnvs * kFnnRow];
    const int t = threadIdx.x, env0 = blockIdx.x * kFnnEnvs;
    const int lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const float *__restrict__ P = A.packed;
    // every tile this wave owns, requested before anything else
    LayerRegs<2> r1;
    LayerRegs<4> r2a, r2b;
    LayerRegs<8> r3;
    LayerRegs<4> r4;
    LayerRegs<2> r5;
    LayerRegs<1> rh;
    load_layer<2>(r1, P + FnnAt<0>::w, wave, lane);
    load_layer<4>(r2a, P + FnnAt<1>::w, wave, lane);
    load_layer<4>(r2b, P + FnnAt<1>::w, wave + 4, lane);
    load_layer<8>(r3, P + FnnAt<2>::w, wave, lane);
    if (wave < 2) load_layer<4>(r4, P + FnnAt<3>::w, wave, lane);
    if (wave == 0) {
        load_layer<2>(r5, P + FnnAt<4>::w, 0, lane);
        load_layer<1>(rh, P + FnnAt<5>::w, 0, lane);
    }
    // observations -> bufA in the K = 32 layout (zero for k >= 18 and for envs past n)
    for (int i = t; i < kFnnEnvs * kPolInPad; i += 64 * kFnnWaves) {
        const int e = i >> 5, k = i & 31, env = env0 + e;
        float v = 0.0f;
        if (k < 18 && env < A.n) {
            v = A.obs[(size_t)env * 18 + k];
            if (A.obs_copy) A.obs_copy[(size_t)env * 18 + k] = (A.finished && A.finished[env]) ? 0.0f : v;
        }
        bufA[e * kPolInStride + (k & 3) * (kPolInPad / 4) + (k >> 2)] = v;
    }
    __syncthreads();
    policy_layer<2, 64, kPolicyReLU>(r1, P + FnnAt<0>::b, bufA, kPolInStride, bufB, wave, lane);
    __syncthreads();
    policy_layer<4, 128, kPolicyReLU>(r2a, P + FnnAt<1>::b, bufB, 64 + 4, bufA, wave, lane);
    policy_layer<4, 128, kPolicyReLU>(r2b, P + FnnAt<1>::b, bufB, 64 + 4, bufA, wave + 4, lane);
    __syncthreads();
    policy_layer<8, 64, kPolicyReLU>(r3, P + FnnAt<2>::b, bufA, 128 + 4, bufB, wave, lane);
    __syncthreads();
    if (wave < 2) policy_layer<4, 32, kPolicyReLU>(r4, P + FnnAt<3>::b, bufB, 64 + 4, bufA, wave, lane);
    __syncthreads();
    if (wave != 0) return;
    // fc5 and the heads on wave 0 alone: what is left is one tile wide (the wave's own LDS traffic is in program order)
    policy_layer<2, 16, kPolicyReLU>(r5, P + FnnAt<4>::b, bufA, 32 + 4, bufB, 0, lane);
    wave_sync();   // the rows written above, before other lanes of the wave read them
    const f32x4 acc = fnn_head_tile(rh, bufB, lane);
    const int e = lane & 15, q = lane >> 4;
    const float bh = P[FnnAt<5>::b + e];
    // lane (col e, rows 4 q + reg): cols 0, 1 the action, cols 2, 3, 4 the type logits; the lane of col 0 writes the row
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
        const float v = acc[reg] + bh;
        const float a1 = __shfl(v, lane + 1, 64), l0 = __shfl(v, lane + 2, 64), l1 = __shfl(v, lane + 3, 64),
                    l2 = __shfl(v, lane + 4, 64);
        const int env = env0 + 4 * q + reg;
        if (e != 0 || env >= A.n) continue;
        const bool live = !(A.finished && A.finished[env]);
        const float a0 = v;
        if (A.points) {
            A.points[2 * (size_t)env] = live ? (double)a0 : 0.0;
            A.points[2 * (size_t)env + 1] = live ? (double)a1 : 0.0;
        }
        if (A.types) A.types[env] = live ? (double)fnn_argmax3(l0, l1, l2) / 2.0 : 0.0;
        if (A.actions) {
            A.actions[2 * (size_t)env] = live ? a0 : 0.0f;
            A.actions[2 * (size_t)env + 1] = live ? a1 : 0.0f;
        }
        if (A.logits) {
            A.logits[3 * (size_t)env] = live ? l0 : 0.0f;
            A.logits[3 * (size_t)env + 1] = live ? l1 : 0.0f;
            A.logits[3 * (size_t)env + 2] = live ? l2 : 0.0f;
        }
    }
}

// ------------------------------------------------------------------------------------------ the closed loop around k_move
//
// EBRD.py:541-548 breaks out of its loop at `done`; in a batch a finished environment must stay exactly as that step left it.
// finished[e] is set once done[e] != 0 or code[e] >= kMoveRaises (the reference would have raised or ended there); k_move_skip
// and, through the mask k_move_mask derives from the codes, the smoothing launches leave such an env alone.  This kernel runs
// after the move of step t is complete (k_move_finish included): it is the only writer of finished and steps.
__global__ void k_fnn_advance(DevState S, uint8_t *__restrict__ finished, int32_t *__restrict__ steps,
                              const uint8_t *__restrict__ step_done, const uint8_t *__restrict__ step_complete,
                              const uint8_t *__restrict__ step_code, uint8_t *__restrict__ done, uint8_t *__restrict__ complete,
                              uint8_t *__restrict__ code, int32_t *__restrict__ n_elements)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= S.n_envs || finished[e]) return;   // (the rows of a finished env were written by k_move_skip: 255, 0, 0)
    const uint8_t d = step_done[e], c = step_code[e];
    steps[e] += 1;
    done[e] = d;
    complete[e] = step_complete[e];
    code[e] = c;
    if (n_elements) n_elements[e] = S.scal[e].n_elem;
    if (d || c >= (uint8_t)kMoveRaises) finished[e] = 1;
}

}  // namespace meshenv
