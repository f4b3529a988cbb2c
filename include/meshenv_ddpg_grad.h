/*
 * meshenv_ddpg_grad.h -- C-ABI of DDPG's two gradient statements at SB3's default widths [400, 300] (SB3 2.x's TD3.train,
 * which DDPG inherits, with n_critics = 1):
 *     critic_loss = loss_scale * 2 * mean(0.5 (Q1(cat(obs, actions)) - y)^2);  critic.optimizer.zero_grad(); critic_loss.backward()
 *     actor_loss  = -Q1(cat(obs, tanh(mu(obs)))).mean();                       actor.optimizer.zero_grad(); actor_loss.backward()
 * as three launches per call (csrc/meshenv_wide_grad.h: k_wgrad_critic_rows / k_wgrad_actor_rows, k_wgrad_weights,
 * k_wgrad_reduce).  The conventions are those of meshenv.h (return codes MESHENV_E_*, *_dev device
 * pointers owned by the caller, one GPU and one stream per handle, no CPU fallback).  meshenv_ddpg.h holds the forward half
 * (the load of the [400, 300] actor into a MeshPolicy) and stays as it is.
 *
 * The networks (float32, torch.nn.Linear layout: weight [out][in] row-major, bias [out]):
 *     actor   ReLU [400, 300] on 18 observations, then Linear(300, 3) + Tanh
 *     critic  q_networks[0]: ReLU [400, 300] on cat(obs, action) = 21, then Linear(300, 1)
 * Every tensor is read LIVE at each call through the pointer recorded by meshenv_ddpg_grad_bind: optimisers that write in
 * place need no new bind, and there is no refresh.
 */
#ifndef MESHENV_DDPG_GRAD_H
#define MESHENV_DDPG_GRAD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MESHENV_DDPG_GRAD_ACTOR_FLOATS 128832  /* 128 803 actor gradients padded to a multiple of 64 */
#define MESHENV_DDPG_GRAD_CRITIC_FLOATS 129408 /* 129 401 critic gradients padded to a multiple of 64 */
#define MESHENV_DDPG_GRAD_FLOATS (MESHENV_DDPG_GRAD_ACTOR_FLOATS + MESHENV_DDPG_GRAD_CRITIC_FLOATS)
#define MESHENV_DDPG_GRAD_MAX_ROWS 65536       /* the largest batch of one call */

typedef struct MeshDdpgGrad MeshDdpgGrad;

/* A handle on `device` whose launches go to `stream` (a hipStream_t; NULL: the default stream).  loss_scale: 1.0 (SB3's
 * TD3.train: F.mse_loss summed over the critics, no factor) or 0.5 (the convention of meshenv_critic_grad's td3 kind); it
 * scales critic_loss and the critic's gradients and nothing else.  MESHENV_E_ARG: out is NULL, or another loss_scale;
 * MESHENV_E_HIP: no such device. */
int meshenv_ddpg_grad_create(int device, void *stream, float loss_scale, MeshDdpgGrad **out);
/* Waits for the handle's stream, frees the workspace.  NULL is allowed. */
void meshenv_ddpg_grad_destroy(MeshDdpgGrad *g);
/* Later launches go to `stream`.  MESHENV_E_ARG: g is NULL. */
int meshenv_ddpg_grad_set_stream(MeshDdpgGrad *g, void *stream);
/* The last failure on the handle (of meshenv_ddpg_grad_create when g is NULL). */
const char *meshenv_ddpg_grad_last_error(const MeshDdpgGrad *g);

/* Binds the live tensors and the gradient buffer.
 *   actor_dev  n_actor = 6 pointers: w1 [400][18], b1 [400], w2 [300][400], b2 [300], w3 [3][300], b3 [3]
 *   q1_dev     n_critic = 6 pointers: w1 [400][21], b1 [400], w2 [300][400], b2 [300], out_w [1][300], out_b [1]
 *   grad_dev   n_grad = MESHENV_DDPG_GRAD_FLOATS floats: the actor's gradient set at float 0 (w1 at 0, b1 at 7200, w2 at 7600,
 *              b2 at 127600, w3 at 127900, b3 at 128800), the critic's at MESHENV_DDPG_GRAD_ACTOR_FLOATS (w1 at +0, b1 at
 *              +8400, w2 at +8800, b2 at +128800, out_w at +129100, out_b at +129400), torch's layout.  A backward call
 *              OVERWRITES its own set and leaves the other and the padding alone.
 * Allocates nothing: the workspace is sized by the calls.
 * MESHENV_E_ARG: g is NULL, a NULL pointer, another n_actor / n_critic / n_grad, or w2 / w3 / out_w off 16-byte alignment
 * (they are read 16 bytes at a time). */
int meshenv_ddpg_grad_bind(MeshDdpgGrad *g, const float *const *actor_dev, int n_actor, const float *const *q1_dev, int n_critic,
                           float *grad_dev, int64_t n_grad);

/* critic_loss of the n rows obs_dev [n][18], actions_dev [n][3], y_dev [n] into loss_dev [1] and the critic's gradients into
 * its set of the bound buffer: three launches on the handle's stream, no floating-point atomics (repeated calls give the same
 * bits).  The workspace holds 1476 floats per row of the largest n seen (rounded up to 16) and up to 64 partial gradient
 * sets; it only grows, and growing it waits for the handle's stream first: a call at an n not above the largest seen
 * allocates nothing and does not synchronise.
 *   parts_dev  NULL, or 3 pointers: q [n], and the post-ReLU activations [n][400], [n][300] (`> 0` is the mask the backward
 *              pass used)
 * MESHENV_E_STATE: nothing bound; MESHENV_E_ARG: g is NULL, n < 1 or n > MESHENV_DDPG_GRAD_MAX_ROWS, a NULL input, a NULL
 * entry of parts_dev; MESHENV_E_HIP: an allocation or a launch failed. */
int meshenv_ddpg_grad_critic_backward(MeshDdpgGrad *g, int n, const float *obs_dev, const float *actions_dev, const float *y_dev,
                                      float *loss_dev, float *const *parts_dev);

/* actor_loss of the n rows of obs_dev [n][18] into loss_dev [1] and the actor's gradients into its set of the bound buffer;
 * the critic is differentiated with respect to the action only and its gradient set is not touched.  Launches, workspace and
 * return codes as above.
 *   parts_dev  NULL, or 4 pointers: actions [n][3] = actor(obs), q1 [n], dq_da [n][3] (dQ1/daction), d_pre [n][3] (the
 *              gradient of the loss at the head's pre-activation: (-(dq_da / n)) * (1 - actions^2))
 *   acts_dev   NULL, or 4 pointers to post-ReLU activations: actor [n][400], [n][300], critic [n][400], [n][300] */
int meshenv_ddpg_grad_actor_backward(MeshDdpgGrad *g, int n, const float *obs_dev, float *loss_dev, float *const *parts_dev,
                                     float *const *acts_dev);

#ifdef __cplusplus
}
#endif
#endif /* MESHENV_DDPG_GRAD_H */
