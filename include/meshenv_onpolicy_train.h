/*
 * meshenv_onpolicy_train.h -- C-ABI of the on-policy training call of libmeshenv_hip.so: the body of SB3 2.x's PPO.train /
 * A2C.train (stable_baselines3/ppo/ppo.py, a2c/a2c.py),
 *     for epoch in range(n_epochs):
 *         for rollout_data in rollout_buffer.get(batch_size):
 *             ... evaluate_actions, the losses ...
 *             if target_kl is not None and approx_kl > 1.5 * target_kl: continue_training = False; break
 *             zero_grad; backward; clip_grad_norm_; optimizer.step()
 *         _n_updates += 1
 *         if not continue_training: break
 *     explained_variance(values, returns); the logged means
 * as ONE call that enqueues every launch of every epoch (csrc/meshenv_onpolicy_train.h): no host work
 * in between, no synchronisation, no device-to-host copy and no per-step host-to-device copy.  The early stop is a flag on the
 * device: after it, the remaining gradient launches of the queue still run on unchanged parameters and are ignored, and no
 * further step is applied.  The conventions are those of meshenv.h (return codes MESHENV_E_*, *_dev device pointers owned by
 * the caller, one GPU and one stream per handle, no CPU fallback).
 *
 * The call drives handles the caller owns, through the launch code of their own entry points: a MeshPpoGrad
 * (meshenv_ppo_grad.h), a MeshOptim with a bound program (meshenv_optim.h), a MeshRolloutBuffer (meshenv_rollout.h) and,
 * optionally, a MeshPolicy with live tensors bound (meshenv_policy_bind) that is refreshed at the end.
 */
#ifndef MESHENV_ONPOLICY_TRAIN_H
#define MESHENV_ONPOLICY_TRAIN_H

#include <stdint.h>

#include "meshenv.h"
#include "meshenv_optim.h"
#include "meshenv_ppo_grad.h"
#include "meshenv_rollout.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MESHENV_TRAIN_OUTPUTS 12            /* doubles in out_dev, in the order of the enum below */
#define MESHENV_TRAIN_MAX_MINIBATCHES 65536 /* the cap on K = n_epochs x minibatches per epoch */

enum {
    MESHENV_TRAIN_LOSS = 0,                 /* the last loss evaluated */
    MESHENV_TRAIN_POLICY_GRADIENT_LOSS = 1, /* the means over the minibatches evaluated, float64 sums in queue order */
    MESHENV_TRAIN_VALUE_LOSS = 2,
    MESHENV_TRAIN_ENTROPY_LOSS = 3,
    MESHENV_TRAIN_APPROX_KL = 4,            /* the mean over the minibatches evaluated in the LAST epoch entered */
    MESHENV_TRAIN_CLIP_FRACTION = 5,
    MESHENV_TRAIN_EXPLAINED_VARIANCE = 6,   /* 1 - var(returns - values) / var(returns); NaN when var(returns) == 0 */
    MESHENV_TRAIN_STD = 7,                  /* the float32 mean of exp(log_std), after the last step */
    MESHENV_TRAIN_STEPS_APPLIED = 8,        /* optimiser steps applied: K without a stop */
    MESHENV_TRAIN_EPOCHS_RUN = 9,           /* epochs entered, the one that stopped included: SB3's _n_updates increment */
    MESHENV_TRAIN_MINIBATCHES_EVALUATED = 10,
    MESHENV_TRAIN_GRAD_NORM = 11            /* the last evaluated minibatch's total norm before clipping (NaN without clipping) */
};

typedef struct MeshOnPolicyTrain MeshOnPolicyTrain;

/* A handle on `device` whose launches go to `stream` (a hipStream_t; NULL: the default stream); it owns the stop flags, the
 * per-minibatch loss outputs and the tally.  MESHENV_E_ARG: out is NULL; MESHENV_E_HIP: no such device, allocation failed. */
int meshenv_onpolicy_train_create(int device, void *stream, MeshOnPolicyTrain **out);
/* Waits for the handle's stream.  NULL is allowed. */
void meshenv_onpolicy_train_destroy(MeshOnPolicyTrain *t);
/* Later launches go to `stream`.  MESHENV_E_ARG: t is NULL. */
int meshenv_onpolicy_train_set_stream(MeshOnPolicyTrain *t, void *stream);
/* The last failure on the handle (of meshenv_onpolicy_train_create when t is NULL). */
const char *meshenv_onpolicy_train_last_error(const MeshOnPolicyTrain *t);

/* One train(): with rows = T * n_envs, M = ceil(rows / batch_size) and K = n_epochs * M, per epoch e one meshenv_rollout_gather
 * with the e-th permutation, then per minibatch the launches of meshenv_ppo_grad_backward on the slice [k batch_size,
 * min((k + 1) batch_size, rows)) of the gather outputs (a last, shorter minibatch is kept, down to one row) and one
 * k_optim_step_gated launch of `program` with scalars[e * M + k]; then k_train_finish and, with a policy, meshenv_policy_refresh.
 *   g, o, r        bound handles on the device and the stream of t; `program` of o is bound (meshenv_optim_bind) to the
 *                  parameters and the gradient buffer of g
 *   policy         a MeshPolicy with meshenv_policy_bind done, or NULL
 *   in_dev         the six [T][n_envs] histories of meshenv_rollout_gather; value (in_dev[2]) and returns (in_dev[5]) are also
 *                  what explained_variance is taken over
 *   gather_dev     the six gather outputs, [rows][18], [rows][3], [rows] x 4
 *   perm_dev       [n_epochs][rows] indices of perm_bytes = 4 or 8 bytes each
 *   a2c .. max_grad_norm   as meshenv_ppo_grad_backward takes them
 *   target_kl      SB3's target_kl as a double; +inf: none (A2C; PPO with target_kl None)
 *   scalars        K MeshOptimScalars in host memory, read before the call returns: those of the 1st .. K-th step from now
 *   out_dev        MESHENV_TRAIN_OUTPUTS doubles, 8-byte aligned, written by the last launch but the refresh
 * After a stop p.grad holds the stopping minibatch's (clipped) gradients, where SB3 would still hold the previous one's.
 * MESHENV_E_ARG: a NULL handle or pointer, n_epochs < 1, batch_size < 1, a negative or NaN target_kl, rows >
 * MESHENV_ROLLOUT_MAX_ROWS, K > MESHENV_TRAIN_MAX_MINIBATCHES, n_scalars != K, handles on different devices, whatever the driven
 * entry points refuse; MESHENV_E_STATE: an unbound handle or program, handles on different streams; MESHENV_E_HIP: a launch
 * failed. */
int meshenv_onpolicy_train_run(MeshOnPolicyTrain *t, MeshPpoGrad *g, MeshOptim *o, int program, MeshRolloutBuffer *r,
                               MeshPolicy *policy, int T, int n_envs, const float *const *in_dev, float *const *gather_dev,
                               const void *perm_dev, int perm_bytes, int n_epochs, int batch_size, int a2c, double clip_range,
                               float ent_coef, float vf_coef, int normalize_advantage, int clip_grad, float max_grad_norm,
                               double target_kl, const MeshOptimScalars *scalars, int n_scalars, double *out_dev);

#ifdef __cplusplus
}
#endif
#endif /* MESHENV_ONPOLICY_TRAIN_H */
