// The kernels that let SB3's SAC.train / TD3.train run as ONE queue of launches with no host in between
// (include/meshenv_offpolicy_train.h).  Unlike the on-policy call there is no early stop: which steps
// update the actor and the targets is known on the host before anything is enqueued, so nothing here gates a step.
//
// slots[K_max][kOffSlot] floats, owned by the train handle: per gradient step k
//     [0] critic_loss      written by step k's k_critic_grad_reduce
//     [1] actor_loss       written by step k's k_actor_grad_reduce / k_td3_actor_grad_reduce, on actor steps only
//     [2] ent_coef_loss    written by k_actor_grad_reduce with a learned coefficient
//     [3] ent_coef         written by step k's k_optim_step_noted (SAC with a learned coefficient)
// Nothing is zeroed between calls: k_offpolicy_finish reads only the slots this train() wrote.
//
// k_optim_step_noted is k_optim_step (same tables, same opt_chunk<OP>, hence the same bits) whose thread 0 of workgroup 0 also
// writes note[0] = expf(log_ent_coef[0]): SB3 logs ent_coef as it is BEFORE the step's entropy-coefficient update, and the
// expression is k_actor_grad's own for alpha, so the logged value is the coefficient the step's actor loss applies.  It runs
// the CRITIC program, which writes neither log_ent_coef (the host refuses such a program) nor the slot, after the previous
// step's actor / ent-coef launch and before this one's: no workgroup reads a word another workgroup of the same launch
// writes.  No atomics, no spinning.  k_optim_step and k_optim_step_gated are not changed.
//
// k_offpolicy_finish, one workgroup of kTrFinishThreads once per train(): the float64 sum of each column over the steps that
// wrote it, each thread over its steps t, t + 1024, ... in order and then train_block_sum's binary tree (meshenv_onpolicy_train.h),
// divided by the count.  The actor steps are k = phase, phase + period, ... < K (SAC: every step; TD3: every policy_delay-th).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "meshenv_onpolicy_train.h"
#include "meshenv_optim.h"

namespace meshenv {

constexpr int kOffOut = 8;            // critic_loss actor_loss ent_coef_loss ent_coef gradient_steps actor_steps polyak_updates last_critic_loss
constexpr int kOffSlot = 4;
enum { kOffSacLearned = 0, kOffSacFixed = 1, kOffTd3 = 2 };

struct OptNote {
    const float *log_ent_coef;   // the live [1] tensor
    float *note;                 // &slots[k][3]
};

__global__ __launch_bounds__(kOptThreads) void k_optim_step_noted(const OptSeg *__restrict__ segs, const OptJob *__restrict__ jobs,
                                                                   OptScalars S, OptNote N)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) N.note[0] = expf(N.log_ent_coef[0]);
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

struct OffFinishArgs {
    const float *slots;      // [K][kOffSlot]
    double *out;             // kOffOut doubles
    int32_t K;               // gradient steps of this train()
    int32_t phase, period;   // the actor steps: k = phase, phase + period, ... < K (phase >= K: none)
    int32_t actor_steps, polyak_updates;
    int32_t mode;            // kOffSacLearned, kOffSacFixed, kOffTd3
    float ent_coef;          // kOffSacFixed: the fixed coefficient
};

__global__ void __launch_bounds__(kTrFinishThreads) k_offpolicy_finish(OffFinishArgs A)
{
    __shared__ double sums[kTrFinishThreads];
    const int t = threadIdx.x;
    const bool learned = A.mode == kOffSacLearned;
    double critic = 0.0, actor = 0.0, ent_loss = 0.0, ent = 0.0;
    for (int k = t; k < A.K; k += kTrFinishThreads) {
        const float *s = A.slots + (size_t)k * kOffSlot;
        critic = critic + (double)s[0];
        if (learned) ent = ent + (double)s[3];
        if (k >= A.phase && (k - A.phase) % A.period == 0) {
            actor = actor + (double)s[1];
            if (learned) ent_loss = ent_loss + (double)s[2];
        }
    }
    critic = train_block_sum(critic, sums, t);
    actor = train_block_sum(actor, sums, t);
    ent_loss = train_block_sum(ent_loss, sums, t);
    ent = train_block_sum(ent, sums, t);
    if (t != 0) return;
    const double nan = __builtin_nan("");
    A.out[0] = critic / (double)A.K;
    A.out[1] = A.actor_steps > 0 ? actor / (double)A.actor_steps : nan;
    A.out[2] = learned && A.actor_steps > 0 ? ent_loss / (double)A.actor_steps : nan;
    A.out[3] = learned ? ent / (double)A.K : A.mode == kOffSacFixed ? (double)A.ent_coef : nan;
    A.out[4] = (double)A.K;
    A.out[5] = (double)A.actor_steps;
    A.out[6] = (double)A.polyak_updates;
    A.out[7] = (double)A.slots[(size_t)(A.K - 1) * kOffSlot];
}

}  // namespace meshenv
