// k_optim_step: the Adam steps of SAC / TD3 / PPO, A2C's RMSprop step and SB3's polyak_update over any mix of tensors in one launch
// (include/meshenv_optim.h).
//
// A launch is driven by two tables in device memory, written by meshenv_optim_bind: the SEGMENTS, one per tensor (its
// pointers, its length, what to do with it and which block of per-optimiser scalars it reads), and the JOBS, one per
// workgroup: (segment, first element).  A workgroup of 256 threads owns kOptChunk = 1024 consecutive elements of one segment;
// thread t owns elements [4 t, 4 t + 4) of the chunk and every element is read and written by exactly one thread, so there
// is nothing to reduce: no LDS, no atomics, no scratch, and repeated launches from the same state give the same bits.
//
// Alignment is a property of the segment (OptSeg::vec, decided from the pointers at bind time): the chunk starts at a multiple
// of 1024 floats, so a thread's four floats are 16-byte aligned in every tensor exactly when all the segment's base
// pointers are.  The gradient views of FusedActorGrad are not (log_std.weight.grad follows the 3 floats of mu.bias.grad):
// such a segment takes the scalar path, where thread t owns elements t, t + 256, t + 512, t + 768 and a wave's accesses
// stay contiguous.  The last, partial group of four of an aligned segment is done element by element as well.
//
// The arithmetic is torch.optim.adam._single_tensor_adam's (non-capturable) and SB3's polyak_update, in float32 in their
// order of operations; the translation unit is compiled with -ffp-contract=off and correctly rounded sqrt and division, so
// every line below is the stated sequence of IEEE operations:
//     m  = m + (g - m) * (1 - beta1)                       exp_avg.lerp_(grad, 1 - beta1), weight < 0.5
//     v  = v * beta2 + ((1 - beta2) * g) * g               exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
//     d  = sqrtf(v) / bias_correction2_sqrt + eps          (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
//     p  = p + (-step_size) * (m / d)                      param.addcdiv_(exp_avg, denom, value=-step_size)
//     t  = t * (1 - tau) + tau * p                         target.mul_(1 - tau); target.add_(param, alpha=tau)
// and, for the on-policy recipes (A2C's default optimiser), torch.optim.rmsprop._single_tensor_rmsprop
// with momentum = 0 and centered = False: kOptRmsprop, whose block of scalars carries alpha in beta2, 1 - alpha in w2 and lr
// in step_size, and whose v is square_avg (no first moment: m is NULL):
//     v  = v * alpha + ((1 - alpha) * g) * g               square_avg.mul_(alpha).addcmul_(grad, grad, value=1 - alpha)
//     d  = sqrtf(v) + eps                                  square_avg.sqrt().add_(eps)
//     p  = p + (-lr) * (g / d)                             param.addcdiv_(grad, avg, value=-lr)
// Non-finite gradients go through the same operations and propagate as they do there.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace meshenv {

constexpr int kOptChunk = 1024;     // elements per workgroup: 256 threads x 4
constexpr int kOptThreads = 256;
constexpr int kOptBlocks = 4;       // blocks of per-optimiser scalars a launch can carry

enum { kOptAdam = 1, kOptPolyak = 2, kOptAdamPolyak = 3, kOptRmsprop = 4 };

struct OptSeg {
    float *p;           // the parameter: written by Adam, read by Polyak
    const float *g;     // its gradient (Adam)
    float *m, *v;       // exp_avg, exp_avg_sq (Adam); RMSprop: NULL, square_avg
    float *t;           // the target parameter (Polyak)
    int32_t n;          // elements
    int32_t op;         // kOptAdam, kOptPolyak, kOptAdamPolyak, kOptRmsprop
    int32_t block;      // which OptScalars block (Adam)
    int32_t vec;        // 1: all of this segment's pointers are 16-byte aligned
};

struct OptJob {
    int32_t seg;        // index into the segment table
    int32_t first;      // first element of the chunk, a multiple of kOptChunk
};

// Host-computed, passed by value: nothing is read back and nothing is uploaded per step.
struct OptScalars {
    float step_size[kOptBlocks];       // lr / (1 - beta1^step)
    float bc2_sqrt[kOptBlocks];        // sqrt(1 - beta2^step)
    float w1[kOptBlocks];              // 1 - beta1
    float beta2[kOptBlocks];
    float w2[kOptBlocks];              // 1 - beta2
    float eps[kOptBlocks];
    float tau, one_minus_tau;
};

struct OptCoef {
    float neg_step, bc2_sqrt, w1, beta2, w2, eps, tau, omt;
};

template <int OP>
__device__ __forceinline__ void opt_element(const OptCoef &c, float &p, float g, float &m, float &v, float &t)
{
    if (OP & kOptAdam) {
        m = m + (g - m) * c.w1;
        v = v * c.beta2 + (c.w2 * g) * g;
        const float d = sqrtf(v) / c.bc2_sqrt + c.eps;
        p = p + c.neg_step * (m / d);
    }
    if (OP & kOptPolyak) t = t * c.omt + c.tau * p;
    if (OP == kOptRmsprop) {
        v = v * c.beta2 + (c.w2 * g) * g;
        const float d = sqrtf(v) + c.eps;
        p = p + c.neg_step * (g / d);
    }
}

template <int OP>
__device__ __forceinline__ void opt_one(const OptSeg &s, const OptCoef &c, int i)
{
    float p = s.p[i], g = 0.0f, m = 0.0f, v = 0.0f, t = 0.0f;
    if (OP & kOptAdam) { g = s.g[i]; m = s.m[i]; v = s.v[i]; }
    if (OP & kOptPolyak) t = s.t[i];
    if (OP == kOptRmsprop) { g = s.g[i]; v = s.v[i]; }
    opt_element<OP>(c, p, g, m, v, t);
    if (OP & kOptAdam) { s.p[i] = p; s.m[i] = m; s.v[i] = v; }
    if (OP == kOptRmsprop) { s.p[i] = p; s.v[i] = v; }
    if (OP & kOptPolyak) s.t[i] = t;
}

template <int OP>
__device__ __forceinline__ void opt_chunk(const OptSeg &s, const OptCoef &c, int first)
{
    const int tid = (int)threadIdx.x;
    const int i4 = first + 4 * tid;
    if (s.vec && i4 + 4 <= s.n) {
        float4 p = *reinterpret_cast<const float4 *>(s.p + i4), g{}, m{}, v{}, t{};
        if (OP & kOptAdam) {
            g = *reinterpret_cast<const float4 *>(s.g + i4);
            m = *reinterpret_cast<const float4 *>(s.m + i4);
            v = *reinterpret_cast<const float4 *>(s.v + i4);
        }
        if (OP & kOptPolyak) t = *reinterpret_cast<const float4 *>(s.t + i4);
        if (OP == kOptRmsprop) {
            g = *reinterpret_cast<const float4 *>(s.g + i4);
            v = *reinterpret_cast<const float4 *>(s.v + i4);
        }
        opt_element<OP>(c, p.x, g.x, m.x, v.x, t.x);
        opt_element<OP>(c, p.y, g.y, m.y, v.y, t.y);
        opt_element<OP>(c, p.z, g.z, m.z, v.z, t.z);
        opt_element<OP>(c, p.w, g.w, m.w, v.w, t.w);
        if (OP & kOptAdam) {
            *reinterpret_cast<float4 *>(s.p + i4) = p;
            *reinterpret_cast<float4 *>(s.m + i4) = m;
            *reinterpret_cast<float4 *>(s.v + i4) = v;
        }
        if (OP & kOptPolyak) *reinterpret_cast<float4 *>(s.t + i4) = t;
        if (OP == kOptRmsprop) {
            *reinterpret_cast<float4 *>(s.p + i4) = p;
            *reinterpret_cast<float4 *>(s.v + i4) = v;
        }
    } else if (s.vec) {                         // the segment's last, partial group of four
        for (int i = i4; i < s.n; i++) opt_one<OP>(s, c, i);
    } else {
        const int end = first + kOptChunk < s.n ? first + kOptChunk : s.n;
        for (int i = first + tid; i < end; i += kOptThreads) opt_one<OP>(s, c, i);
    }
}

__global__ __launch_bounds__(kOptThreads) void k_optim_step(const OptSeg *__restrict__ segs, const OptJob *__restrict__ jobs,
                                                             OptScalars S)
{
    const OptJob job = jobs[blockIdx.x];
    const OptSeg s = segs[job.seg];
    const int b = s.block;
    OptCoef c;
    c.neg_step = -S.step_size[b]; c.bc2_sqrt = S.bc2_sqrt[b]; c.w1 = S.w1[b]; c.beta2 = S.beta2[b]; c.w2 = S.w2[b];
    c.eps = S.eps[b]; c.tau = S.tau; c.omt = S.one_minus_tau;
    if (s.op == kOptAdam) opt_chunk<kOptAdam>(s, c, job.first);
    else if (s.op == kOptPolyak) opt_chunk<kOptPolyak>(s, c, job.first);
    else if (s.op == kOptRmsprop) opt_chunk<kOptRmsprop>(s, c, job.first);
    else opt_chunk<kOptAdamPolyak>(s, c, job.first);
}

}  // namespace meshenv
