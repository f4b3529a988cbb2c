/*
 * meshenv_td3_actor_grad.h -- C-ABI of the TD3 / DDPG actor loss gradient of libmeshenv_hip.so: the statements of SB3 2.x's
 * TD3.train that run every policy_delay steps,
 *     actor_loss = -self.critic.q1_forward(replay_data.observations, self.actor(replay_data.observations)).mean()
 *     self.actor.optimizer.zero_grad(); actor_loss.backward()
 * as two launches per call (csrc/meshenv_td3_actor_grad.h: k_td3_actor_grad, k_td3_actor_grad_reduce; DESIGN.md section
 * 18).  The conventions are those of meshenv.h (return codes MESHENV_E_*, *_dev device pointers owned by the caller, one GPU
 * and one stream per handle, no CPU fallback); the entry points live in a header of their own, as those of meshenv_optim.h
 * do, because meshenv_actor_grad_* of meshenv.h is the SAC statement and stays as it is.
 *
 * The networks (float32, torch.nn.Linear layout: weight [out][in] row-major, bias [out]):
 *     actor   ReLU [256, 256] on 18 observations, then Linear(256, 3) + Tanh
 *     critic  q_networks[0]: ReLU [256, 256] on cat(obs, action) = 21, then Linear(256, 1).  Only this critic is read: a
 *             second critic (TD3) or none (DDPG) makes no difference to the statement.
 * Every tensor is read LIVE at each call through the pointer recorded by meshenv_td3_actor_grad_bind: optimisers that
 * write in place need no new bind.  The critic's parameters receive no gradient.
 */
#ifndef MESHENV_TD3_ACTOR_GRAD_H
#define MESHENV_TD3_ACTOR_GRAD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MESHENV_TD3_ACTOR_GRAD_FLOATS 71488 /* the gradient buffer: 71 427 gradients padded to a multiple of 64 */

typedef struct MeshTd3ActorGrad MeshTd3ActorGrad;

/* A handle on `device` whose launches go to `stream` (a hipStream_t; NULL: the default stream).  MESHENV_E_ARG: out is
 * NULL; MESHENV_E_HIP: no such device. */
int meshenv_td3_actor_grad_create(int device, void *stream, MeshTd3ActorGrad **out);
/* Waits for the handle's stream, frees the workspace.  NULL is allowed. */
void meshenv_td3_actor_grad_destroy(MeshTd3ActorGrad *g);
/* Later launches go to `stream`.  MESHENV_E_ARG: g is NULL. */
int meshenv_td3_actor_grad_set_stream(MeshTd3ActorGrad *g, void *stream);
/* The last failure on the handle (of meshenv_td3_actor_grad_create when g is NULL). */
const char *meshenv_td3_actor_grad_last_error(const MeshTd3ActorGrad *g);

/* Binds the live tensors and the gradient buffer.
 *   actor_dev  n_actor = 6 pointers: w1 [256][18], b1 [256], w2 [256][256], b2 [256], w3 [3][256], b3 [3]
 *   q1_dev     n_critic = 6 pointers: w1 [256][21], b1 [256], w2 [256][256], b2 [256], out_w [1][256], out_b [1]
 *   grad_dev   n_grad = MESHENV_TD3_ACTOR_GRAD_FLOATS floats, which every meshenv_td3_actor_grad_backward OVERWRITES with
 *              the actor's gradients in actor_dev's order and torch's layout: w1 at float 0, b1 at 4608, w2 at 4864, b2 at
 *              70400, w3 at 70656, b3 at 71424; the 61 floats of padding are not written
 * The first bind allocates the workspace: 128 partial gradient sets of n_grad + 64 floats.
 * MESHENV_E_ARG: g is NULL, a NULL pointer, another n_actor / n_critic / n_grad, or w2 / w3 / out_w off 16-byte alignment
 * (they are read 16 bytes at a time); MESHENV_E_HIP: the allocation failed. */
int meshenv_td3_actor_grad_bind(MeshTd3ActorGrad *g, const float *const *actor_dev, int n_actor, const float *const *q1_dev,
                                int n_critic, float *grad_dev, int64_t n_grad);

/* actor_loss of the n rows of obs_dev [n][18] into loss_dev [1] and its gradients into the bound buffer: two launches on the
 * handle's stream, no synchronisation, no floating-point atomics (repeated calls give the same bits).
 *   parts_dev  NULL, or 4 pointers: actions [n][3] = actor(obs), q1 [n], dq_da [n][3] (dQ1/daction), d_pre [n][3] (the
 *              gradient of the loss at the head's pre-activation: (-(dq_da / n)) * (1 - actions^2))
 *   acts_dev   NULL, or 4 pointers to [n][256] post-ReLU activations: actor layer 1, actor layer 2, critic layer 1, critic
 *              layer 2 (`> 0` is the mask the backward pass used)
 * MESHENV_E_STATE: nothing bound; MESHENV_E_ARG: g is NULL, n < 1 or n > 2^24 - 16, obs_dev or loss_dev NULL, a NULL entry
 * of parts_dev / acts_dev; MESHENV_E_HIP: a launch failed. */
int meshenv_td3_actor_grad_backward(MeshTd3ActorGrad *g, int n, const float *obs_dev, float *loss_dev, float *const *parts_dev,
                                    float *const *acts_dev);

#ifdef __cplusplus
}
#endif
#endif /* MESHENV_TD3_ACTOR_GRAD_H */
