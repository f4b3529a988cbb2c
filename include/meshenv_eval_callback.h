/*
 * meshenv_eval_callback.h -- C-ABI of SB3 2.x's EvalCallback (stable_baselines3/common/callbacks.py; the reference's
 * CustomCallback, rl/baselines/CustomizeCallback.py:241-310) decided on the device (csrc/meshenv_eval_callback.h, DESIGN.md
 * section 25):
 *   - an evaluation that is only queued: meshenv_evaluate's loop for a fixed number of vector steps, no host read
 *     (meshenv_evaluate_queued);
 *   - the reduction of its records to one history row, the comparison with the best mean so far and the `improved` word
 *     (meshenv_eval_reduce);
 *   - a copy of the live parameter tensors into one flat buffer, gated by that word (meshenv_keep_best).
 * Every call enqueues on the handle's stream and returns: no host copy, no synchronisation.  The conventions are those of
 * meshenv.h (return codes MESHENV_E_*, *_dev device pointers owned by the caller, no CPU fallback).
 */
#ifndef MESHENV_EVAL_CALLBACK_H
#define MESHENV_EVAL_CALLBACK_H

#include <stdint.h>

#include "meshenv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MESHENV_EVAL_ROW_DOUBLES 9             /* doubles per history row, see meshenv_eval_reduce */
#define MESHENV_EVAL_STATE_DOUBLES 4           /* best_mean, best_eval, last_mean, evaluations */
#define MESHENV_KEEP_BEST_MAX_ENTRIES 64       /* tensors per meshenv_keep_best call */

/* ---- the queued evaluation ---- */

/* meshenv_evaluate with the host reads removed: meshenv_reset, the start of the tally, then exactly `steps` times the policy
 * (or the actor), one step with auto-reset and one tally launch.  `sample`, `seed` and `counter` are meshenv_evaluate's: the
 * actions of vector step t use noise counter counter + t.  Envs that reach their target keep stepping unrecorded; an episode
 * that does not end within `steps` is not recorded and its env stays in bufs->short_dev[0].  Nothing is returned through host
 * pointers and nothing waits for the stream: the records stay in bufs until the caller reads or reduces them.  The step
 * buffers are allocated before the first launch (by the first call; none with bufs->obs_dev set).
 * MESHENV_E_ARG: h NULL, both or neither of policy and actor, steps < 1, a bad bufs; MESHENV_E_STATE: no weights loaded,
 * another device or stream, ep_quality_dev without an element log. */
int meshenv_evaluate_queued(MeshEnv *h, MeshPolicy *policy, MeshActor *actor, int sample, uint64_t seed, uint64_t counter, int steps,
                            const MeshEvalBuffers *bufs);

/* ---- the reduction and the gated copy ---- */

typedef struct MeshEvalCallback MeshEvalCallback;

/* A handle on `device` whose launches go to `stream`; every buffer it touches is the caller's.
 * MESHENV_E_ARG: out is NULL; MESHENV_E_HIP: no such device. */
int meshenv_eval_callback_create(int device, void *stream, MeshEvalCallback **out);
/* Waits for the handle's stream.  NULL is allowed. */
void meshenv_eval_callback_destroy(MeshEvalCallback *c);
int meshenv_eval_callback_set_stream(MeshEvalCallback *c, void *stream);
const char *meshenv_eval_callback_last_error(const MeshEvalCallback *c);

/* One launch of one 64-lane workgroup over the tally's buffers of n_envs envs and `total` episode slots (bufs: target_dev,
 * offset_dev, count_dev, ep_return_dev, ep_length_dev, ep_flags_dev, ep_n_elements_dev, short_dev are read).  Slot s of env e
 * is recorded iff s - offset[e] < min(count[e], target[e]); every other slot is a hole and is not read.
 *   Order of every float64 sum: lane l adds, from 0.0, the recorded slots of envs l, l + 64, l + 128, ... (envs ascending, an
 *   env's slots ascending); the 64 partial sums are then combined by an xor butterfly, p[l] += p[l ^ d] for d = 32, 16, 8, 4,
 *   2, 1.  mean_reward = sum(return) / recorded; std_reward = sqrt(sum((return - mean_reward)^2) / recorded) in the same
 *   order (the population value, numpy's std); the lengths, complete flags and element counts are summed as integers.
 * Row `row` of history_dev [capacity][9] receives
 *     num_timesteps, mean_reward, std_reward, mean_ep_length, recorded, short, complete_rate, mean_n_elements, improved
 * where mean_n_elements is over the recorded episodes with n_elements >= 0, and every mean over nothing is the quiet NaN
 * 0x7FF8000000000000.  improved = recorded > 0 and mean_reward > state_dev[0], strictly: a tie and a NaN do not improve.
 * state_dev [4] = best_mean (the caller starts it at -inf), best_eval (the row of the best evaluation; -1), last_mean, evaluations
 * (row + 1); best_mean and best_eval change only when improved.  improved_dev [1] receives 0 or 1.
 * MESHENV_E_ARG: c NULL, n_envs < 1, total < 0, row outside [0, capacity), a bad bufs, a NULL or misaligned pointer. */
int meshenv_eval_reduce(MeshEvalCallback *c, int n_envs, int total, const MeshEvalBuffers *bufs, int row, int capacity,
                        double num_timesteps, double *history_dev, double *state_dev, int32_t *improved_dev);

/* One float32 tensor of a meshenv_keep_best call: numel floats at src_dev go to best_dev + dst_offset (in floats). */
typedef struct MeshKeepEntry {
    const float *src_dev;
    int64_t dst_offset;
    int64_t numel;
} MeshKeepEntry;

/* One launch that copies the n_entries tensors of entries_host (a host array, read before returning) into best_dev
 * [best_floats] when improved_dev[0] != 0 and writes nothing when it is 0; every workgroup reads the word once.  Per tensor:
 * scalar copies up to the first 16-byte boundary of the destination, 16-byte copies from there when the source is 16-byte
 * aligned at that element (scalar copies otherwise), scalar copies for the tail.  The ranges must not overlap each other or
 * a source.
 * MESHENV_E_ARG: c NULL, n_entries outside 1 .. MESHENV_KEEP_BEST_MAX_ENTRIES, a NULL or misaligned pointer, numel < 1, a
 * range outside [0, best_floats). */
int meshenv_keep_best(MeshEvalCallback *c, const MeshKeepEntry *entries_host, int n_entries, float *best_dev, int64_t best_floats,
                      const int32_t *improved_dev);

#ifdef __cplusplus
}
#endif
#endif /* MESHENV_EVAL_CALLBACK_H */
