/*
 * meshenv_ppo_grad.h -- C-ABI of the PPO / A2C loss gradient of libmeshenv_hip.so, and of the refresh of a loaded policy from
 * its live tensors.  meshenv_ppo_grad_backward is the statement of SB3 2.x's PPO.train (A2C.train with a2c != 0) for one
 * minibatch of n rows,
 *     values, log_prob, entropy = self.policy.evaluate_actions(rollout_data.observations, actions)
 *     advantages = (advantages - advantages.mean()) / (advantages.std() + 1e-8)          # normalize_advantage and n > 1
 *     ratio = th.exp(log_prob - rollout_data.old_log_prob)
 *     policy_loss = -th.min(advantages * ratio, advantages * th.clamp(ratio, 1 - clip_range, 1 + clip_range)).mean()
 *     value_loss = F.mse_loss(rollout_data.returns, values);  entropy_loss = -th.mean(entropy)
 *     loss = policy_loss + self.ent_coef * entropy_loss + self.vf_coef * value_loss
 *     self.policy.optimizer.zero_grad(); loss.backward()
 *     th.nn.utils.clip_grad_norm_(self.policy.parameters(), self.max_grad_norm)
 * (A2C: policy_loss = -(advantages * log_prob).mean(), no ratio; clip_range_vf is None in both) as at most four launches
 * (csrc/meshenv_ppo_grad.h: k_ppo_adv_stats, k_ppo_grad, k_ppo_grad_reduce, k_ppo_grad_clip), for the
 * recipes of rl/baselines/RL_Mesh.py:113-177.  The conventions are those of meshenv.h (return codes MESHENV_E_*, *_dev device
 * pointers owned by the caller, one GPU and one stream per handle, no CPU fallback); the entry points live in a header of
 * their own, as those of meshenv_optim.h and meshenv_td3_actor_grad.h do.
 *
 * The policy (float32, torch.nn.Linear layout: weight [out][in] row-major, bias [out]): an SB3 ActorCriticPolicy with a pi
 * and a vf tower of two hidden layers of the same width 64 or 128, ReLU or Tanh, on 18 observations; action_net
 * Linear(H, 3), value_net Linear(H, 1), a state-independent log_std [3] (DiagGaussianDistribution).  Every tensor is read
 * LIVE at each call through the pointer recorded by the bind: optimisers that write in place need no new bind.
 */
#ifndef MESHENV_PPO_GRAD_H
#define MESHENV_PPO_GRAD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MESHENV_PPO_GRAD_FLOATS_64 11072   /* the gradient buffer at width 64: 11 015 gradients padded to a multiple of 64 */
#define MESHENV_PPO_GRAD_FLOATS_128 38464  /* at width 128: 38 407 gradients */
#define MESHENV_PPO_GRAD_OUTPUTS 8         /* floats of out_dev */
#define MESHENV_PPO_GRAD_PARTS 5           /* pointers of parts_dev */

typedef struct MeshPpoGrad MeshPpoGrad;
typedef struct MeshPolicy MeshPolicy;      /* meshenv.h: meshenv_policy_create */

/* A handle on `device` whose launches go to `stream` (a hipStream_t; NULL: the default stream).  MESHENV_E_ARG: out is
 * NULL; MESHENV_E_HIP: no such device. */
int meshenv_ppo_grad_create(int device, void *stream, MeshPpoGrad **out);
/* Waits for the handle's stream, frees the workspace.  NULL is allowed. */
void meshenv_ppo_grad_destroy(MeshPpoGrad *g);
/* Later launches go to `stream`.  MESHENV_E_ARG: g is NULL. */
int meshenv_ppo_grad_set_stream(MeshPpoGrad *g, void *stream);
/* The last failure on the handle (of meshenv_ppo_grad_create when g is NULL). */
const char *meshenv_ppo_grad_last_error(const MeshPpoGrad *g);

/* Binds the live tensors of policy.parameters() that the statement differentiates, and the gradient buffer.
 *   hidden, activation  64 or 128; 0 (ReLU) or 1 (Tanh).  256 is refused: its dW_2 needs a column split that is not built.
 *   tensors_dev  n_tensors = 13 pointers: pi w1 [H][18], b1 [H], w2 [H][H], b2 [H], wh [3][H] (action_net), bh [3]; vf w1, b1,
 *                w2, b2, wh [1][H] (value_net), bh [1]; log_std [3]
 *   grad_dev     n_grad = MESHENV_PPO_GRAD_FLOATS_<hidden> floats, which every meshenv_ppo_grad_backward OVERWRITES with the
 *                (clipped) gradients in tensors_dev's order and torch's layout, one tensor behind the other from float 0; the
 *                padding is not written
 * The first bind allocates the workspace: 128 partial gradient sets of the wider layout and the advantage statistics.
 * MESHENV_E_ARG: g is NULL, a NULL pointer, another width / activation / n_tensors / n_grad, or a w2 / wh off 16-byte
 * alignment (they are read 16 bytes at a time); MESHENV_E_HIP: the allocation failed. */
int meshenv_ppo_grad_bind(MeshPpoGrad *g, int hidden, int activation, const float *const *tensors_dev, int n_tensors,
                          float *grad_dev, int64_t n_grad);

/* The loss of the n rows and its gradients into the bound buffer.  Launches on the handle's stream, no synchronisation, no
 * device-to-host copy, no floating-point atomics (repeated calls give the same bits): the advantage statistics (when
 * normalize_advantage and n > 1), the gradient kernel, the ordered reduction, and with clip_grad the clip.
 *   obs_dev [n][18], actions_dev [n][3] (the unclipped Gaussian samples RolloutBuffer stores), old_log_prob_dev [n] (NULL
 *   allowed with a2c), advantages_dev [n], returns_dev [n]; none of them is written
 *   a2c          0: PPO's clipped surrogate with clip_range > 0; otherwise A2C's loss (clip_range is not read)
 *   clip_range   a double, as SB3 holds it: the clamp's limits are float32(1 - clip_range) and float32(1 + clip_range), formed in
 *                double as torch forms them, and clip_fraction compares with float32(clip_range)
 *   ent_coef, vf_coef, normalize_advantage   the statement's
 *   clip_grad, max_grad_norm   clip_grad != 0: clip_grad_norm_(max_grad_norm > 0) on the 13 gradients
 *   out_dev      MESHENV_PPO_GRAD_OUTPUTS floats: loss, policy_loss, value_loss, entropy_loss, approx_kl = mean((ratio - 1) -
 *                log_ratio), clip_fraction = mean(|ratio - 1| > clip_range) (both 0 with a2c), grad_norm = the total norm before
 *                clipping (NaN without clip_grad), one spare
 *   parts_dev    NULL, or MESHENV_PPO_GRAD_PARTS pointers to [n] floats: log_prob, ratio (1 with a2c), values, the advantages
 *                as used (normalised), pass (1 where the row's surrogate passes its gradient to ratio, else 0)
 *   acts_dev     NULL, or 4 pointers to [n][hidden] kept activations: pi layer 1, pi layer 2, vf layer 1, vf layer 2
 * MESHENV_E_STATE: nothing bound; MESHENV_E_ARG: g is NULL, n < 1 or n > 2^24 - 16, a required pointer NULL, a non-finite
 * coefficient, clip_range <= 0 without a2c, max_grad_norm <= 0 with clip_grad, a NULL entry of parts_dev / acts_dev;
 * MESHENV_E_HIP: a launch failed. */
int meshenv_ppo_grad_backward(MeshPpoGrad *g, int n, const float *obs_dev, const float *actions_dev, const float *old_log_prob_dev,
                              const float *advantages_dev, const float *returns_dev, int a2c, double clip_range, float ent_coef,
                              float vf_coef, int normalize_advantage, int clip_grad, float max_grad_norm, float *out_dev,
                              float *const *parts_dev, float *const *acts_dev);

/* Records the device pointers of the live tensors of a LOADED policy (meshenv_policy_load laid its packed buffer out): 13 for
 * the actor-critic kind, in meshenv_ppo_grad_bind's order, 6 (w1 b1 w2 b2 mu_w mu_b) for the deterministic kind.  What
 * SB3 does implicitly: collect_rollouts reads the parameters policy.optimizer.step() has just written.  A later
 * meshenv_policy_load drops the binding.  MESHENV_E_STATE: nothing loaded; MESHENV_E_ARG: p or a pointer NULL, another
 * n_tensors. */
int meshenv_policy_bind(MeshPolicy *p, const float *const *tensors_dev, int n_tensors);
/* One launch on the policy's stream: the bound tensors into the packed buffer, in exactly the layout meshenv_policy_load
 * builds on the host (same padding, same zeroes; low / high and the deterministic kind's sigma stay as loaded).  No host
 * copy, no synchronisation.  MESHENV_E_STATE: nothing bound; MESHENV_E_HIP: the launch failed. */
int meshenv_policy_refresh(MeshPolicy *p);

#ifdef __cplusplus
}
#endif
#endif /* MESHENV_PPO_GRAD_H */
