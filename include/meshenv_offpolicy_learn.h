/*
 * meshenv_offpolicy_learn.h -- C-ABI of what SB3 2.x's OffPolicyAlgorithm.learn needs around SAC.train / TD3.train
 * (stable_baselines3/common/off_policy_algorithm.py) so that its loop
 *     while num_timesteps < total_timesteps:
 *         rollout = collect_rollouts(env, train_freq, action_noise, learning_starts, replay_buffer)
 *         if num_timesteps > learning_starts: train(gradient_steps, batch_size)
 * stays on the device (csrc/meshenv_learn.h):
 *   - the behaviour actor of SAC follows the trained parameters without a host rebuild (meshenv_actor_bind / _refresh; the
 *     TD3 behaviour policy has meshenv_policy_bind / _refresh of meshenv_ppo_grad.h);
 *   - _sample_action before learning_starts (meshenv_uniform_actions) and the env steps that take its actions
 *     (meshenv_step_actions_multi);
 *   - the Monitor's episode returns and lengths (meshenv_episode_stats_*).
 * Every call enqueues on the handle's stream and returns: no host copy, no synchronisation.  The conventions are those of
 * meshenv.h (return codes MESHENV_E_*, *_dev device pointers owned by the caller, no CPU fallback).
 */
#ifndef MESHENV_OFFPOLICY_LEARN_H
#define MESHENV_OFFPOLICY_LEARN_H

#include <stdint.h>

#include "meshenv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MESHENV_UNIFORM_PHILOX_TAG 4           /* the fourth Philox counter word of meshenv_uniform_actions */
#define MESHENV_EPISODE_RING_DOUBLES 3         /* doubles per ring entry: return, length, complete */

/* ---- the live SAC behaviour actor ---- */

/* The ten LIVE device tensors of the SAC actor, torch.nn.Linear layout, float32 contiguous, in the order
 * w1 b1 w2 b2 w3 b3 mu_w mu_b log_std_w log_std_b ([128][18], [128], [128][128], [128], [128][128], [128], [3][128], [3],
 * [3][128], [3]): recorded, not read.  meshenv_actor_load must have laid the packed buffer out first (the padding it zeroed
 * is never rewritten; low / high stay as loaded).
 * MESHENV_E_ARG: a is NULL, n != 10, a NULL entry; MESHENV_E_STATE: no weights loaded. */
int meshenv_actor_bind(MeshActor *a, const float *const *tensors_dev, int n);
/* The bound tensors, as they are now, into the packed weights: ONE launch on the handle's stream.  Launches that follow on
 * that stream (meshenv_actor_forward / _sample, meshenv_step_actor*) see the new weights.
 * MESHENV_E_STATE: nothing bound; MESHENV_E_HIP: the launch failed. */
int meshenv_actor_refresh(MeshActor *a);
/* The last failure of the two calls above on the handle. */
const char *meshenv_actor_last_error(const MeshActor *a);

/* ---- warm-up actions ---- */

/* actions_dev [T][n][3] (the Box low_high_host[0..2] .. [3..5]) and buffer_actions_dev [T][n][3] (in [-1, 1)) of T vector
 * steps of h's n envs, one launch: element (t, env, c) from Philox4x32-10 keyed by seed at counter words
 * (env, lo(counter + t), hi(counter + t), MESHENV_UNIFORM_PHILOX_TAG), output word c:
 *     u = (float)(word >> 8) * 2^-24;  buffer = 2 u - 1;  action = low + 0.5 * (buffer + 1) * (high - low)   (float32).
 * MESHENV_E_ARG: h NULL, T < 1, a NULL pointer, non-finite bounds or high <= low. */
int meshenv_uniform_actions(MeshEnv *h, int T, uint64_t seed, uint64_t counter, const float *low_high_host, float *actions_dev,
                            float *buffer_actions_dev);

/* T x meshenv_step on slices of caller-owned histories: step t takes actions_dev[t] ([T][n][3]) and writes obs_dev[t + 1]
 * (obs_dev is [T + 1][n][18]; slice 0, what the first action was chosen on, is the caller's and is not read), reward_dev[t]
 * ([T][n] doubles), done_dev[t], complete_dev[t] ([T][n] bytes) and terminal_obs_dev[t] ([T][n][18] or NULL).  What
 * meshenv_step_actor_multi is, without the actor.
 * MESHENV_E_ARG: h NULL, T < 1, a NULL required pointer. */
int meshenv_step_actions_multi(MeshEnv *h, int T, const float *actions_dev, float *obs_dev, double *reward_dev, uint8_t *done_dev,
                               uint8_t *complete_dev, float *terminal_obs_dev, int auto_reset);

/* ---- episode statistics ---- */

typedef struct MeshEpisodeStats MeshEpisodeStats;

/* A handle on `device` whose launches go to `stream`; the state it updates is the caller's.
 * MESHENV_E_ARG: out is NULL; MESHENV_E_HIP: no such device. */
int meshenv_episode_stats_create(int device, void *stream, MeshEpisodeStats **out);
/* Waits for the handle's stream.  NULL is allowed. */
void meshenv_episode_stats_destroy(MeshEpisodeStats *s);
int meshenv_episode_stats_set_stream(MeshEpisodeStats *s, void *stream);
const char *meshenv_episode_stats_last_error(const MeshEpisodeStats *s);

/* The Monitor over T vector steps of n envs, one launch of one workgroup.  reward_dev [T][n] doubles, done_dev and
 * complete_dev [T][n] bytes.  Persistent state, zeroed by the caller before the first call: carry_return_dev [n] doubles,
 * carry_len_dev [n] int32, ring_dev [window][3] doubles (return, length, complete), count_dev one uint64 (8-byte aligned).
 * An env's return is the sequential double sum of its rewards in step order since its last done; finished episodes enter the
 * ring in the order of t * n + env at slots (count + rank) % window; when more than `window` finish in one call only the last
 * `window` are written, and count advances by all of them.  work_return_dev [T * n] doubles and work_len_dev [T * n] int32
 * are scratch.  No rounding is applied (the Monitor's round(r, 6) is the reader's).
 * MESHENV_E_ARG: s NULL, T < 1, n < 1, window < 1, T * n >= 2^31, a NULL pointer, a misaligned count_dev. */
int meshenv_episode_stats_update(MeshEpisodeStats *s, int T, int n, int window, const double *reward_dev, const uint8_t *done_dev,
                                 const uint8_t *complete_dev, double *carry_return_dev, int32_t *carry_len_dev, double *ring_dev,
                                 uint64_t *count_dev, double *work_return_dev, int32_t *work_len_dev);

#ifdef __cplusplus
}
#endif
#endif /* MESHENV_OFFPOLICY_LEARN_H */
