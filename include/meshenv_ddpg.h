/*
 * meshenv_ddpg.h -- C-ABI of what DDPG adds to libmeshenv_hip.so: its [400, 300] actor as a MeshPolicy (csrc/meshenv_wide.h,
 * DESIGN.md section 31).  The conventions are those of meshenv.h (return codes MESHENV_E_*, host weight pointers in
 * torch.nn.Linear layout, one GPU and one stream per handle, no CPU fallback); the entry point lives in a header of its own so
 * that meshenv.h and its exports stay as they are.  DDPG's TD target is kind 2 of meshenv_target_create (meshenv.h).
 */
#ifndef MESHENV_DDPG_H
#define MESHENV_DDPG_H

#include "meshenv.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The deterministic kind with two hidden widths (csrc/meshenv_wide.h): DDPG's actor as the reference builds it,
 * DDPG('MlpPolicy', env) (rl/baselines/RL_Mesh.py:113-228, v2/src/mesh_rl/algorithms/sb3_algos.py:31-43), i.e. SB3's
 * TD3Policy default net_arch [400, 300] with ReLU: mu = Linear(18, 400), ReLU, Linear(400, 300), ReLU, Linear(300, 3), Tanh.
 * Accepts kind 1, activation 0 (ReLU), (hidden1, hidden2) = (400, 300); anything else fails with MESHENV_E_ARG and a message
 * naming what is supported.  Weights as meshenv_policy_load takes them (host pointers, [out][in] row-major): w1 [400][18],
 * b1 [400], w2 [300][400], b2 [300], head_w [3][300], head_b [3], sigma [3] (nullable: no action noise), low, high [3].
 * The handle then serves meshenv_policy_forward, meshenv_step_policy_multi, meshenv_evaluate, meshenv_evaluate_queued and
 * meshenv_policy_bind / meshenv_policy_refresh (six live tensors) exactly as a kind-1 policy of meshenv_policy_load does.
 */
int meshenv_policy_load_widths(MeshPolicy *p, int kind, int hidden1, int hidden2, int activation, const float *w1, const float *b1,
                               const float *w2, const float *b2, const float *head_w, const float *head_b, const float *sigma,
                               const float *low, const float *high);

#ifdef __cplusplus
}
#endif

#endif /* MESHENV_DDPG_H */
