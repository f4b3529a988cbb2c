/*
 * meshenv_optim.h -- C-ABI of the optimiser step of libmeshenv_hip.so: the Adam steps of SB3's SAC.train / TD3.train and
 * its polyak_update, applied in place to the caller's tensors by one launch of k_optim_step per call
 * (csrc/meshenv_optim.h).  The conventions are those of meshenv.h (return codes MESHENV_E_*, *_dev
 * device pointers owned by the caller, one GPU and one stream per handle, no CPU fallback); the entry points live in a
 * header of their own because they bind to torch.optim.Adam's state rather than to an environment.
 *
 * What they replace, per gradient step of stable_baselines3/sac/sac.py (td3/td3.py likewise):
 *     self.critic.optimizer.step()
 *     self.actor.optimizer.step();  self.ent_coef_optimizer.step()
 *     polyak_update(self.critic.parameters(), self.critic_target.parameters(), self.tau)
 *
 * A handle holds up to MESHENV_OPTIM_PROGRAMS programs.  A program is a list of SEGMENTS, one per tensor:
 *     op     MESHENV_OPTIM_ADAM         param, grad, exp_avg, exp_avg_sq       (target NULL)
 *            MESHENV_OPTIM_POLYAK       param (read), target                   (grad, exp_avg, exp_avg_sq NULL)
 *            MESHENV_OPTIM_ADAM_POLYAK  all five: the target sees the stepped parameter (TD3's actor -> actor_target)
 *            MESHENV_OPTIM_RMSPROP      param, grad, exp_avg_sq = square_avg   (exp_avg, target NULL): torch.optim.RMSprop with
 *                                       momentum = 0 and centered = False, A2C's default optimiser.  There is no RMSprop +
 *                                       Polyak op: nothing on-policy has a target network
 *     n      elements, float32, contiguous
 *     block  which block of per-optimiser scalars the Adam update reads (0 .. MESHENV_OPTIM_BLOCKS - 1)
 *     vec    1 when every pointer of the segment is 16-byte aligned (128-bit loads and stores), 0 for the scalar path;
 *            MESHENV_E_ARG when 1 is passed for a segment that is not
 * meshenv_optim_bind writes a program's tables to device memory (stream-ordered, from pinned memory); it is called again
 * only when a pointer has changed.  meshenv_optim_step launches a program with the scalars of that step as kernel
 * arguments: no synchronisation, no device-to-host read and no host-to-device copy.
 */
#ifndef MESHENV_OPTIM_H
#define MESHENV_OPTIM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MESHENV_OPTIM_PROGRAMS 8
#define MESHENV_OPTIM_BLOCKS 4
#define MESHENV_OPTIM_CHUNK 1024 /* elements per workgroup */

enum { MESHENV_OPTIM_ADAM = 1, MESHENV_OPTIM_POLYAK = 2, MESHENV_OPTIM_ADAM_POLYAK = 3, MESHENV_OPTIM_RMSPROP = 4 };

/* The scalars of one step, computed on the host in doubles exactly as torch.optim.adam._single_tensor_adam does from the
 * incremented step, then rounded to float: step_size = lr / (1 - beta1^step), bc2_sqrt = (1 - beta2^step)^0.5,
 * w1 = 1 - beta1, w2 = 1 - beta2.  A block read by MESHENV_OPTIM_RMSPROP segments holds alpha in beta2, 1 - alpha in w2, lr in
 * step_size, and eps; its w1 and bc2_sqrt are not read. */
typedef struct MeshOptimScalars {
    float step_size[MESHENV_OPTIM_BLOCKS];
    float bc2_sqrt[MESHENV_OPTIM_BLOCKS];
    float w1[MESHENV_OPTIM_BLOCKS];
    float beta2[MESHENV_OPTIM_BLOCKS];
    float w2[MESHENV_OPTIM_BLOCKS];
    float eps[MESHENV_OPTIM_BLOCKS];
    float tau, one_minus_tau;
} MeshOptimScalars;

typedef struct MeshOptim MeshOptim;

int meshenv_optim_create(int device, void *stream, MeshOptim **out);
void meshenv_optim_destroy(MeshOptim *o);
int meshenv_optim_set_stream(MeshOptim *o, void *stream);
/* The last failure on the handle (of meshenv_optim_create when o is NULL). */
const char *meshenv_optim_last_error(const MeshOptim *o);

/* Program `program` := n_seg segments; the arrays have n_seg entries each (host memory, read before the call returns).
 * MESHENV_E_ARG: a NULL or missing pointer for the op, a pointer an op does not take, n < 1, a pointer off 4-byte
 * alignment, vec = 1 on a segment with a pointer off 16-byte alignment, block out of range, more than 2^31 - 1 jobs. */
int meshenv_optim_bind(MeshOptim *o, int program, int n_seg, float *const *param_dev, const float *const *grad_dev,
                       float *const *exp_avg_dev, float *const *exp_avg_sq_dev, float *const *target_dev, const int64_t *n,
                       const int32_t *op, const int32_t *block, const int32_t *vec);

/* One launch of k_optim_step over every segment of the program.  MESHENV_E_STATE when the program is not bound. */
int meshenv_optim_step(MeshOptim *o, int program, const MeshOptimScalars *scalars);

#ifdef __cplusplus
}
#endif
#endif /* MESHENV_OPTIM_H */
