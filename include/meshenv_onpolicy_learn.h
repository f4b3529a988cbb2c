/*
 * meshenv_onpolicy_learn.h -- C-ABI of what SB3 2.x's OnPolicyAlgorithm.learn (stable_baselines3/common/on_policy_algorithm.py)
 *     while num_timesteps < total_timesteps:
 *         collect_rollouts(env, callback, rollout_buffer, n_steps)
 *         train()
 * needs beyond meshenv_onpolicy_train.h so that a PPO with a target_kl never drains the queue between two train() calls
 * (csrc/meshenv_onpolicy_train.h: k_optim_step_counted, k_learn_finish).  meshenv_onpolicy_train_run
 * takes the Adam scalars of its K steps as host-computed kernel arguments, so the host has to know how many steps the last
 * train() applied before it can enqueue the next one.  Here that count stays on the device: the step of minibatch m looks its
 * bias corrections up in a table in device memory by count[m], and the finish kernel hands count[K] to the next train().  The
 * conventions are those of meshenv.h (return codes MESHENV_E_*, *_dev device pointers owned by the caller, one GPU and one
 * stream per handle, no CPU fallback).
 *
 * The caller owns the WORDS: int32 words_dev[MESHENV_LEARN_WORDS + K], in order the running _n_updates word (epochs entered),
 * the error word (non-zero: a launch found its count outside the table and behaved as stopped), the step count (steps applied
 * since the table's origin: count[0] of the next train()), then count[1 .. K] of the train() in flight.  One copy of the first
 * MESHENV_LEARN_WORDS words after the last train() is all the host reads.
 */
#ifndef MESHENV_ONPOLICY_LEARN_H
#define MESHENV_ONPOLICY_LEARN_H

#include <stdint.h>

#include "meshenv.h"
#include "meshenv_onpolicy_train.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MESHENV_LEARN_WORDS 3                  /* _n_updates, error, step count: what the host reads back */
#define MESHENV_LEARN_MAX_ENTRIES 1048576      /* the cap on a table's entries (2^20) */

enum { MESHENV_LEARN_WORD_N_UPDATES = 0, MESHENV_LEARN_WORD_ERROR = 1, MESHENV_LEARN_WORD_STEPS = 2 };

/* What a counted step takes instead of MeshOptimScalars' step_size and bc2_sqrt: the learning rate of this train() per block
 * as a double (SB3's lr_schedule changes it per iteration); the kernel forms step_size = (float)(lr / bias_correction1) and
 * bc2_sqrt = (float)bias_correction2_sqrt from the table.  The other fields are MeshOptimScalars' own. */
typedef struct MeshOptimCounted {
    double lr[MESHENV_OPTIM_BLOCKS];
    float w1[MESHENV_OPTIM_BLOCKS];
    float beta2[MESHENV_OPTIM_BLOCKS];
    float w2[MESHENV_OPTIM_BLOCKS];
    float eps[MESHENV_OPTIM_BLOCKS];
    float tau, one_minus_tau;
} MeshOptimCounted;

typedef struct MeshOnPolicyLearn MeshOnPolicyLearn;

/* A handle on `device` whose launches go to `stream` (a hipStream_t; NULL: the default stream); it owns the table and its
 * pinned staging block.  MESHENV_E_ARG: out is NULL; MESHENV_E_HIP: no such device. */
int meshenv_onpolicy_learn_create(int device, void *stream, MeshOnPolicyLearn **out);
/* Waits for the handle's stream.  NULL is allowed. */
void meshenv_onpolicy_learn_destroy(MeshOnPolicyLearn *l);
/* Later launches go to `stream`.  MESHENV_E_ARG: l is NULL. */
int meshenv_onpolicy_learn_set_stream(MeshOnPolicyLearn *l, void *stream);
/* The last failure on the handle (of meshenv_onpolicy_learn_create when l is NULL). */
const char *meshenv_onpolicy_learn_last_error(const MeshOnPolicyLearn *l);

/* Binds a table and the words, stream-ordered: table_host ([entries][blocks][2] doubles: bias_correction1 and
 * bias_correction2_sqrt of the (j + 1)-th step after the origin, per block of optimiser scalars; read before the call returns)
 * goes through the pinned block to the device, and the first MESHENV_LEARN_WORDS words of words_dev are zeroed, both on the
 * handle's stream.  Nothing synchronises unless the table has to grow (launches in flight may read the old one) or the last
 * upload from the pinned block has not finished.  A bind starts a new origin: the entries that meshenv_onpolicy_learn_run calls
 * have claimed are forgotten.
 * MESHENV_E_ARG: l, table_host or words_dev is NULL, entries < 1 or > MESHENV_LEARN_MAX_ENTRIES, blocks < 1 or >
 * MESHENV_OPTIM_BLOCKS, n_words < MESHENV_LEARN_WORDS + 1, words_dev off 4-byte alignment, an entry that is not finite or
 * whose bias_correction1 is zero; MESHENV_E_HIP: allocation, upload or memset failed. */
int meshenv_onpolicy_learn_bind(MeshOnPolicyLearn *l, const double *table_host, int entries, int blocks, int32_t *words_dev,
                                int64_t n_words);

/* One counted train(): meshenv_onpolicy_train_run with k_optim_step_counted for k_optim_step_gated and k_learn_finish for
 * k_train_finish.  Every argument up to target_kl is meshenv_onpolicy_train_run's; then
 *   counted        the scalars of every step of this train(), host memory, read before the call returns
 *   history_dev    [iterations][MESHENV_TRAIN_OUTPUTS] doubles, 8-byte aligned; row `iteration` is written
 * The call claims K = n_epochs * ceil(T * n_envs / batch_size) entries of the bound table: whatever the device decides, a
 * train() applies at most K steps, so the sum of the claims bounds every count that a launch can read.
 * MESHENV_E_ARG: what meshenv_onpolicy_train_run refuses; l, counted or history_dev NULL; iteration outside [0, iterations);
 * the claims since the bind plus K exceed the table's entries (no launch may index past a table: nothing is enqueued); the
 * bound words are fewer than MESHENV_LEARN_WORDS + K; a non-finite lr; the program has a block outside the table's.
 * MESHENV_E_STATE: nothing bound; what meshenv_onpolicy_train_run answers so.  MESHENV_E_HIP: a launch failed. */
int meshenv_onpolicy_learn_run(MeshOnPolicyLearn *l, MeshOnPolicyTrain *t, MeshPpoGrad *g, MeshOptim *o, int program,
                               MeshRolloutBuffer *r, MeshPolicy *policy, int T, int n_envs, const float *const *in_dev,
                               float *const *gather_dev, const void *perm_dev, int perm_bytes, int n_epochs, int batch_size, int a2c,
                               double clip_range, float ent_coef, float vf_coef, int normalize_advantage, int clip_grad,
                               float max_grad_norm, double target_kl, const MeshOptimCounted *counted, double *history_dev,
                               int iteration, int iterations);

#ifdef __cplusplus
}
#endif
#endif /* MESHENV_ONPOLICY_LEARN_H */
