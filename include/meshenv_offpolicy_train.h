/*
 * meshenv_offpolicy_train.h -- C-ABI of the off-policy training call of libmeshenv_hip.so: the body of SB3 2.x's SAC.train /
 * TD3.train (stable_baselines3/sac/sac.py, td3/td3.py),
 *     SAC:  for gradient_step in range(gradient_steps):
 *               replay_data = self.replay_buffer.sample(batch_size)
 *               ent_coef = th.exp(self.log_ent_coef.detach());  the entropy-coefficient step
 *               with th.no_grad(): ... target_q_values
 *               critic_loss; self.critic.optimizer.step()
 *               actor_loss;  self.actor.optimizer.step()
 *               if gradient_step % self.target_update_interval == 0: polyak_update(critic, critic_target, tau)
 *           self._n_updates += gradient_steps
 *     TD3:  for _ in range(gradient_steps):
 *               self._n_updates += 1
 *               replay_data = self.replay_buffer.sample(batch_size)
 *               with th.no_grad(): ... clipped noise ... target_q_values
 *               critic_loss; self.critic.optimizer.step()
 *               if self._n_updates % self.policy_delay == 0:
 *                   actor_loss; self.actor.optimizer.step(); polyak_update of the critic and of the actor
 *     the logged means
 * as ONE call that enqueues every launch of every gradient step (csrc/meshenv_offpolicy_train.h): no
 * host work in between, no synchronisation, no device-to-host copy and no per-step host-to-device copy.  Which steps update
 * the actor and the targets is decided by the caller before the call (actor_program).  The conventions are those of meshenv.h
 * (return codes MESHENV_E_*, *_dev device pointers owned by the caller, one GPU and one stream per handle, no CPU fallback).
 *
 * The call drives handles the caller owns, through their own entry points: the MeshEnv whose replay store is sampled, a
 * MeshTarget, a MeshCriticGrad, a MeshActorGrad (SAC) or a MeshTd3ActorGrad (TD3; meshenv_td3_actor_grad.h) and a MeshOptim
 * with the critic and the actor program(s) bound (meshenv_optim.h).  The order inside a step is the one the library's
 * examples compose: draw, target (from the snapshot of the last refresh), critic gradients, critic step, actor gradients (which
 * read the unstepped log_ent_coef), the actor program (actor, entropy coefficient and Polyak in one launch), refresh.
 */
#ifndef MESHENV_OFFPOLICY_TRAIN_H
#define MESHENV_OFFPOLICY_TRAIN_H

#include <stdint.h>

#include "meshenv.h"
#include "meshenv_optim.h"
#include "meshenv_td3_actor_grad.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MESHENV_OFFTRAIN_OUTPUTS 8             /* doubles in out_dev, in the order of the enum below */
#define MESHENV_OFFTRAIN_MAX_STEPS 65536       /* the cap on gradient_steps of one call: 1 MiB of loss slots */
#define MESHENV_REPLAY_BATCHES_MAX_SAMPLES 16777216   /* the cap on n_batches * batch of meshenv_replay_sample_batches: 2^24 */
#define MESHENV_OFFTRAIN_SAMPLE_FLOATS 41      /* floats of the sample workspace per sample: 18 + 3 + 18 + 1 + 1 */

enum {
    MESHENV_OFFTRAIN_CRITIC_LOSS = 0,      /* the means are float64 sums over the steps that wrote the value, divided by their count */
    MESHENV_OFFTRAIN_ACTOR_LOSS = 1,       /* NaN when no actor step ran */
    MESHENV_OFFTRAIN_ENT_COEF_LOSS = 2,    /* NaN with a fixed coefficient and for TD3 */
    MESHENV_OFFTRAIN_ENT_COEF = 3,         /* learned: the mean of expf(log_ent_coef) before each step; fixed: the value; TD3: NaN */
    MESHENV_OFFTRAIN_GRADIENT_STEPS = 4,
    MESHENV_OFFTRAIN_ACTOR_STEPS = 5,
    MESHENV_OFFTRAIN_POLYAK_UPDATES = 6,
    MESHENV_OFFTRAIN_LAST_CRITIC_LOSS = 7
};

typedef struct MeshOffPolicyTrain MeshOffPolicyTrain;

/* A handle on `device` whose launches go to `stream` (a hipStream_t; NULL: the default stream); it owns the per-step loss
 * slots.  MESHENV_E_ARG: out is NULL; MESHENV_E_HIP: no such device, allocation failed. */
int meshenv_offpolicy_train_create(int device, void *stream, MeshOffPolicyTrain **out);
/* Waits for the handle's stream.  NULL is allowed. */
void meshenv_offpolicy_train_destroy(MeshOffPolicyTrain *t);
/* Later launches go to `stream`.  MESHENV_E_ARG: t is NULL. */
int meshenv_offpolicy_train_set_stream(MeshOffPolicyTrain *t, void *stream);
/* The last failure on the handle (of meshenv_offpolicy_train_create when t is NULL). */
const char *meshenv_offpolicy_train_last_error(const MeshOffPolicyTrain *t);

/* n_batches x replay_buffer.sample(batch) in one launch: batch g of the outputs ([n_batches][batch][18], [..][3], [..][18],
 * [..][1], [..][1], and optionally the drawn rows / envs as [n_batches][batch] int32) has exactly the bits of
 * meshenv_replay_sample(h, store_dev, rows, size, batch, seed, counter + g, NULL, NULL, ...); counter + g wraps modulo 2^64.
 * MESHENV_E_ARG: what meshenv_replay_sample refuses (batch < 1, rows < 1, size outside [1, rows], a NULL or overlapping
 * pointer, a store off 16-byte alignment), n_batches < 1, n_batches * batch > MESHENV_REPLAY_BATCHES_MAX_SAMPLES. */
int meshenv_replay_sample_batches(MeshEnv *h, const float *store_dev, int rows, int size, int batch, int n_batches, uint64_t seed,
                                  uint64_t counter, float *obs_out_dev, float *actions_out_dev, float *next_obs_out_dev,
                                  float *dones_out_dev, float *rewards_out_dev, int32_t *rows_out_dev, int32_t *envs_out_dev);

/* One train() of K gradient steps.  Per chunk of `chunk` steps one meshenv_replay_sample_batches at counter0 + (first step of
 * the chunk) into sample_dev; per step k the launches of meshenv_target_forward (sampled noise at (seed, counter0 + k)),
 * meshenv_critic_grad_backward, the critic program with critic_scalars[k] (k_optim_step_noted when sac_ag has a learned
 * log_ent_coef bound), and where actor_program[k] >= 0 the actor backward (SAC: sampled noise at (seed, counter0 + k)) and
 * that program with the next of actor_scalars; meshenv_target_refresh after every step of SAC and after the actor steps of
 * TD3; then k_offpolicy_finish.
 *   env            the MeshEnv the replay store belongs to (its n_envs); store_dev, rows, size as meshenv_replay_sample takes them
 *   target, cg     bound handles (meshenv_target_bind + meshenv_target_refresh, meshenv_critic_grad_bind)
 *   sac_ag, td3_ag exactly one of the two, bound
 *   o              the MeshOptim; critic_program and every program named in actor_program are bound (meshenv_optim_bind)
 *   sample_dev     five buffers for `chunk` batches: [chunk][batch][18], [..][3], [..][18], [..][1], [..][1] floats
 *                  (MESHENV_OFFTRAIN_SAMPLE_FLOATS per sample in all); a later chunk's draw is enqueued after the earlier
 *                  chunk's steps, so stream order makes the reuse safe
 *   target_dev     [batch] floats: target_q_values of the step in flight; it overlaps no sample buffer
 *   actor_program  K ints in host memory: the program index of step k's actor step, or -1 for none.  The steps >= 0 must be
 *                  k = first, first + period, ... for one period (SB3's two schedules are); all of them, or none
 *   critic_scalars K MeshOptimScalars; actor_scalars: one per step with actor_program[k] >= 0, in order.  Host memory, read
 *                  before the call returns
 *   out_dev        MESHENV_OFFTRAIN_OUTPUTS doubles, 8-byte aligned, written by the last launch
 * All handles are on the device and the stream of t.
 * MESHENV_E_ARG: a NULL handle or pointer, both or neither actor-gradient handle, K < 1, K > MESHENV_OFFTRAIN_MAX_STEPS,
 * batch < 1, chunk < 1, chunk * batch > MESHENV_REPLAY_BATCHES_MAX_SAMPLES, n_actor_scalars that does not match actor_program,
 * actor steps that do not recur with one period, a misaligned out_dev, a critic program with a segment on log_ent_coef, handles
 * on different devices, whatever the driven entry points refuse; MESHENV_E_STATE: an unbound handle or program, a target never
 * refreshed, handles on different streams; MESHENV_E_HIP: a launch failed. */
int meshenv_offpolicy_train_run(MeshOffPolicyTrain *t, MeshEnv *env, MeshTarget *target, MeshCriticGrad *cg, MeshActorGrad *sac_ag,
                                MeshTd3ActorGrad *td3_ag, MeshOptim *o, int critic_program, const float *store_dev, int rows, int size,
                                int batch, int K, uint64_t seed, uint64_t counter0, float *const *sample_dev, int chunk,
                                float *target_dev, const int32_t *actor_program, const MeshOptimScalars *critic_scalars,
                                const MeshOptimScalars *actor_scalars, int n_actor_scalars, double *out_dev);

#ifdef __cplusplus
}
#endif
#endif /* MESHENV_OFFPOLICY_TRAIN_H */
