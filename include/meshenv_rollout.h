/*
 * meshenv_rollout.h -- C-ABI of the on-policy rollout buffer of libmeshenv_hip.so: the minibatches of one epoch of SB3 2.x's
 * RolloutBuffer.get,
 *     indices = np.random.permutation(self.buffer_size * self.n_envs)
 *     ... swap_and_flatten of every field ...
 *     yield self._get_samples(indices[start_idx : start_idx + batch_size])
 * as ONE launch per epoch (csrc/meshenv_rollout.h: k_rollout_gather): every row of the six fields is
 * written in permuted order into six field-major outputs, and minibatch k is the slice [k B, (k + 1) B) of each of them.  The
 * conventions are those of meshenv.h (return codes MESHENV_E_*, *_dev device pointers owned by the caller, one GPU and one
 * stream per handle, no CPU fallback); the entry points live in a header of their own, as those of meshenv_optim.h and
 * meshenv_ppo_grad.h do.  (meshenv_rollout and meshenv_rollout_kernel of meshenv.h are the random-action rollout of an
 * environment handle and have nothing to do with this one.)
 */
#ifndef MESHENV_ROLLOUT_H
#define MESHENV_ROLLOUT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MESHENV_ROLLOUT_FIELDS 6          /* observations, actions, old_values, old_log_prob, advantages, returns */
#define MESHENV_ROLLOUT_CHUNK 1024        /* output floats per workgroup */
#define MESHENV_ROLLOUT_MAX_ROWS 16777200 /* 2^24 - 16: the limit of meshenv_ppo_grad_backward */

typedef struct MeshRolloutBuffer MeshRolloutBuffer;

/* A handle on `device` whose launches go to `stream` (a hipStream_t; NULL: the default stream).  MESHENV_E_ARG: out is
 * NULL; MESHENV_E_HIP: no such device. */
int meshenv_rollout_create(int device, void *stream, MeshRolloutBuffer **out);
/* Waits for the handle's stream.  NULL is allowed. */
void meshenv_rollout_destroy(MeshRolloutBuffer *r);
/* Later launches go to `stream`.  MESHENV_E_ARG: r is NULL. */
int meshenv_rollout_set_stream(MeshRolloutBuffer *r, void *stream);
/* The last failure on the handle (of meshenv_rollout_create when r is NULL). */
const char *meshenv_rollout_last_error(const MeshRolloutBuffer *r);

/* One launch on the handle's stream, no synchronisation: with rows = T * n_envs and SB3's flat row index i = env * T + t,
 *     out_dev[f][j] = in_dev[f][t][env]        for i = perm_dev[j], j = 0 .. rows - 1, and each of the six fields f
 *   in_dev    MESHENV_ROLLOUT_FIELDS pointers, [T][n_envs] histories as collect_rollout leaves them: obs [T][n_envs][18],
 *             buffer_actions [T][n_envs][3], value, log_prob, advantages, returns [T][n_envs]; none of them is written
 *   out_dev   MESHENV_ROLLOUT_FIELDS pointers: [rows][18], [rows][3], [rows] x 4; no output may overlap an input
 *   perm_dev  rows indices of perm_bytes = 4 (int32) or 8 (int64) bytes each.  An index outside [0, rows) is never
 *             dereferenced: row j of every output is NaN
 *   variant   0: every field in 4-byte pieces; 1: the observations in 8-byte pieces (both observation pointers 8-byte aligned)
 * MESHENV_E_ARG: r is NULL, T < 1, n_envs < 1, rows > MESHENV_ROLLOUT_MAX_ROWS, a NULL pointer, a pointer off 4-byte
 * alignment (perm_dev: off perm_bytes), another perm_bytes or variant, variant 1 on an observation pointer off 8-byte
 * alignment; MESHENV_E_HIP: the launch failed. */
int meshenv_rollout_gather(MeshRolloutBuffer *r, int T, int n_envs, const void *perm_dev, int perm_bytes,
                           const float *const *in_dev, float *const *out_dev, int variant);

#ifdef __cplusplus
}
#endif
#endif /* MESHENV_ROLLOUT_H */
