// The kernels that let SB3's PPO.train / A2C.train run as ONE queue of launches with no host in between
// (include/meshenv_onpolicy_train.h): the early stop on target_kl lives on the device.
//
// stop[K + 1] (int32, K = epochs x minibatches per epoch) is a chain of flags, one per minibatch.  stop[0] is zero for ever
// (no kernel writes it).  The step of minibatch m reads stop[m] and slot 4 (approx_kl) of the minibatch's k_ppo_grad_reduce
// outputs and forms
//     stopped = stop[m] != 0 || (double)approx_kl > kl_limit          kl_limit = 1.5 * target_kl in doubles; +inf: never
// which is what SB3 tests BEFORE zero_grad / backward / clip / step.  Thread 0 of workgroup 0 writes stop[m + 1] = stopped.  No
// workgroup reads a word that another workgroup of the same launch writes: stop[m] and the outputs were written by earlier
// launches of the stream, stop[m + 1] and the tally are read by later ones.  No atomics, no cooperative launch, no spinning.
//
// k_optim_step_gated is k_optim_step (same tables, same opt_chunk<OP>, hence the same bits) behind that predicate: both words
// come from uniform addresses, so the branch is uniform over the wave, and a stopped workgroup returns without touching the
// parameters or the optimiser's state.  k_optim_step itself is not changed.
//
// The tally (thread 0 of workgroup 0 of the same launch) runs while stop[m] == 0, so also for the minibatch that stops: SB3
// appends to its lists before it tests.  It adds policy_loss, value_loss, entropy_loss, clip_fraction and approx_kl to float64
// sums, one minibatch after another in queue order (a sequential sum: the bound the tests hold it to), restarts the approx_kl
// sum at the first minibatch of an epoch, keeps the last loss and grad_norm, and counts the minibatches evaluated, the steps
// applied and the epochs entered.  The first minibatch of a train() (never stopped) starts every word afresh, so nothing is
// zeroed between calls.
//
// k_train_finish, one workgroup once per train(): explained_variance of the rollout's values against its returns as numpy
// states it, 1 - var(returns - values) / var(returns) (NaN when var(returns) == 0), with d = returns - values formed in float32
// and the two means and the two sums of centred squares in float64, two passes, each thread over its rows t, t + 1024, ... in
// order and then a binary tree over the 1024 partial sums (pg_block_sum's shape, over doubles); std = the float32 mean of the
// three exp(log_std_i), each the float64 exp rounded to float32; and the tally's sums as means.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "meshenv_optim.h"

namespace meshenv {

constexpr int kTrOut = 12;            // loss policy_gradient_loss value_loss entropy_loss approx_kl clip_fraction explained_variance std
                                      // steps_applied epochs_run minibatches_evaluated grad_norm
constexpr int kTrFinishThreads = 1024;

// the tally: doubles
enum { kTlPolicy = 0, kTlValue, kTlEntropy, kTlClip, kTlKl, kTlKlCount, kTlLoss, kTlNorm, kTlEvaluated, kTlSteps, kTlEpochs, kTlWords };

struct TrainGate {
    int32_t *stop;          // &stop[m]: [0] is read, [1] is written
    const float *pg_out;    // the kPgOut outputs of minibatch m's meshenv_ppo_grad_backward
    double *tally;          // kTlWords doubles
    double kl_limit;        // 1.5 * target_kl; +inf without a target_kl
    int32_t first_of_epoch; // 1: minibatch m opens an epoch
    int32_t first_of_train; // 1: m == 0
};

__device__ __forceinline__ void train_tally(const TrainGate &G, bool was_stopped, bool stopped)
{
    G.stop[1] = stopped ? 1 : 0;
    if (was_stopped) return;
    double w[kTlWords];
    for (int i = 0; i < kTlWords; i++) w[i] = G.first_of_train ? 0.0 : G.tally[i];
    if (G.first_of_epoch) {
        w[kTlKl] = 0.0;
        w[kTlKlCount] = 0.0;
        w[kTlEpochs] = w[kTlEpochs] + 1.0;
    }
    const float *o = G.pg_out;
    w[kTlPolicy] = w[kTlPolicy] + (double)o[1];
    w[kTlValue] = w[kTlValue] + (double)o[2];
    w[kTlEntropy] = w[kTlEntropy] + (double)o[3];
    w[kTlClip] = w[kTlClip] + (double)o[5];
    w[kTlKl] = w[kTlKl] + (double)o[4];
    w[kTlKlCount] = w[kTlKlCount] + 1.0;
    w[kTlLoss] = (double)o[0];
    w[kTlNorm] = (double)o[6];
    w[kTlEvaluated] = w[kTlEvaluated] + 1.0;
    if (!stopped) w[kTlSteps] = w[kTlSteps] + 1.0;
    for (int i = 0; i < kTlWords; i++) G.tally[i] = w[i];
}

__global__ __launch_bounds__(kOptThreads) void k_optim_step_gated(const OptSeg *__restrict__ segs, const OptJob *__restrict__ jobs,
                                                                   OptScalars S, TrainGate G)
{
    const bool was_stopped = G.stop[0] != 0;
    const bool stopped = was_stopped || (double)G.pg_out[4] > G.kl_limit;
    if (blockIdx.x == 0 && threadIdx.x == 0) train_tally(G, was_stopped, stopped);
    if (stopped) return;
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

// k_optim_step_counted (include/meshenv_onpolicy_learn.h) is k_optim_step_gated without the host-computed
// OptScalars: how many steps the device has applied is a word on the device, so the Adam bias corrections of a step are looked
// up by it.  count[K + 1] (int32) is a chain like stop[]: count[m] is the number of steps applied since the table's origin before
// minibatch m, read by every workgroup; thread 0 of workgroup 0 writes count[m + 1] = count[m] + (stopped ? 0 : 1), which only
// later launches read.  table[entries][blocks][2] (doubles) holds bias_correction1 and bias_correction2_sqrt of the
// (j + 1)-th step after the origin, formed by the host as adam_scalars forms them; lr arrives as a double and
//     step_size = (float)(lr / bias_correction1)           bc2_sqrt = (float)bias_correction2_sqrt
// are the IEEE division and the round-to-nearest conversions that the host's lr / bc1 stored into a float are, so an applied
// step has k_optim_step_gated's bits.  A count outside [0, entries) never indexes the table: the launch behaves as stopped and
// thread 0 of workgroup 0 sets *error, which the host reads with the count.
struct OptCounted {
    int32_t *count;         // &count[m]: [0] is read, [1] is written
    const double *table;    // [entries][blocks][2]
    int32_t *error;         // set to 1 by a launch whose count is outside the table
    int32_t entries, blocks;
    double lr[kOptBlocks];
    float w1[kOptBlocks], beta2[kOptBlocks], w2[kOptBlocks], eps[kOptBlocks];
    float tau, one_minus_tau;
};

__global__ __launch_bounds__(kOptThreads) void k_optim_step_counted(const OptSeg *__restrict__ segs, const OptJob *__restrict__ jobs,
                                                                     OptCounted C, TrainGate G)
{
    const bool was_stopped = G.stop[0] != 0;
    const int32_t n = C.count[0];
    const bool outside = n < 0 || n >= C.entries;
    const bool stopped = was_stopped || outside || (double)G.pg_out[4] > G.kl_limit;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        train_tally(G, was_stopped, stopped);
        C.count[1] = n + (stopped ? 0 : 1);
        if (outside) *C.error = 1;
    }
    if (stopped) return;
    const OptJob job = jobs[blockIdx.x];
    const OptSeg s = segs[job.seg];
    const int b = s.block;
    const double *e = C.table + ((size_t)n * C.blocks + b) * 2;
    OptCoef c;
    c.neg_step = -(float)(C.lr[b] / e[0]); c.bc2_sqrt = (float)e[1]; c.w1 = C.w1[b]; c.beta2 = C.beta2[b]; c.w2 = C.w2[b];
    c.eps = C.eps[b]; c.tau = C.tau; c.omt = C.one_minus_tau;
    if (s.op == kOptAdam) opt_chunk<kOptAdam>(s, c, job.first);
    else if (s.op == kOptPolyak) opt_chunk<kOptPolyak>(s, c, job.first);
    else if (s.op == kOptRmsprop) opt_chunk<kOptRmsprop>(s, c, job.first);
    else opt_chunk<kOptAdamPolyak>(s, c, job.first);
}

// pg_block_sum over doubles: the sum to every thread, in a fixed order
__device__ __forceinline__ double train_block_sum(double s, double *red, int t)
{
    red[t] = s;
    __syncthreads();
    for (int w = kTrFinishThreads / 2; w > 0; w >>= 1) {
        if (t < w) red[t] = red[t] + red[t + w];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// The whole of k_train_finish by its one workgroup; true for the thread that wrote the outputs
__device__ __forceinline__ bool train_finish(const float *__restrict__ values, const float *__restrict__ returns, int rows,
                                             const float *__restrict__ log_std, const double *__restrict__ tally, double *__restrict__ out)
{
    __shared__ double red[kTrFinishThreads];
    const int t = threadIdx.x;
    double sr = 0.0, sd = 0.0;
    for (int i = t; i < rows; i += kTrFinishThreads) {
        const float r = returns[i], d = r - values[i];
        sr = sr + (double)r;
        sd = sd + (double)d;
    }
    const double mean_r = train_block_sum(sr, red, t) / (double)rows;
    const double mean_d = train_block_sum(sd, red, t) / (double)rows;
    sr = 0.0;
    sd = 0.0;
    for (int i = t; i < rows; i += kTrFinishThreads) {
        const float r = returns[i], d = r - values[i];
        const double cr = (double)r - mean_r, cd = (double)d - mean_d;
        sr = sr + cr * cr;
        sd = sd + cd * cd;
    }
    const double var_r = train_block_sum(sr, red, t) / (double)rows;
    const double var_d = train_block_sum(sd, red, t) / (double)rows;
    if (t != 0) return false;
    const float e0 = (float)exp((double)log_std[0]), e1 = (float)exp((double)log_std[1]), e2 = (float)exp((double)log_std[2]);
    const float std_mean = ((e0 + e1) + e2) / 3.0f;
    const double n = tally[kTlEvaluated];
    out[0] = tally[kTlLoss];
    out[1] = tally[kTlPolicy] / n;
    out[2] = tally[kTlValue] / n;
    out[3] = tally[kTlEntropy] / n;
    out[4] = tally[kTlKl] / tally[kTlKlCount];
    out[5] = tally[kTlClip] / n;
    out[6] = var_r == 0.0 ? __builtin_nan("") : 1.0 - var_d / var_r;
    out[7] = (double)std_mean;
    out[8] = tally[kTlSteps];
    out[9] = tally[kTlEpochs];
    out[10] = n;
    out[11] = tally[kTlNorm];
    return true;
}

__global__ void __launch_bounds__(kTrFinishThreads)
k_train_finish(const float *__restrict__ values, const float *__restrict__ returns, int rows, const float *__restrict__ log_std,
               const double *__restrict__ tally, double *__restrict__ out)
{
    train_finish(values, returns, rows, log_std, tally, out);
}

// k_train_finish for a counted train() (k_optim_step_counted): the same outputs into a row of the learn()'s history, and the
// hand-over to the next train() of the queue: count[K] into count[0], epochs_run added to the running _n_updates word.  One
// workgroup; the words are read and written by thread 0 alone, after every step launch of this train() and before any of the next.
__global__ void __launch_bounds__(kTrFinishThreads)
k_learn_finish(const float *__restrict__ values, const float *__restrict__ returns, int rows, const float *__restrict__ log_std,
               const double *__restrict__ tally, double *__restrict__ out, int32_t *count, int K, int32_t *n_updates)
{
    if (!train_finish(values, returns, rows, log_std, tally, out)) return;
    count[0] = count[K];
    *n_updates = *n_updates + (int32_t)tally[kTlEpochs];
}

}  // namespace meshenv
