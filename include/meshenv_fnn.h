/*
 * meshenv_fnn.h -- C-ABI of the supervised element-extraction network ("FNN mesher") of libmeshenv_hip.so: the forward of
 * general/EBRD.py's Policy (:85-91, 120-126) as one launch, and the meshing loop of EBRD.py:525-548,
 *     state = env.reset(static=True)
 *     while True:
 *         action, type = get_action(state, model)                      # :174-177
 *         state, _, done, info = env.move(action, round(type, 2))
 *         if done: break
 * for every environment of a handle as ONE call that enqueues T forwards and T moves with no host work and no synchronisation
 * in between (csrc/meshenv_fnn.h: k_fnn_forward, k_fnn_advance; csrc/meshenv_kernels.h: k_move_skip).
 * The inference half: the training of the network (EBRD.py train_ch3) is meshenv_fnn_train.h's.  The conventions are those of meshenv.h (return
 * codes MESHENV_E_*, *_dev device pointers owned by the caller, one GPU and one stream per handle, no CPU fallback); the entry
 * points live in a header of their own, as those of meshenv_ppo_grad.h and meshenv_topology.h do: meshenv.h and
 * MESHENV_ABI_VERSION are unchanged.
 *
 * The network (float32, torch.nn.Linear layout: weight [out][in] row-major, bias [out]), in the order of MESHENV_FNN_TENSORS:
 *     fc1 [64][18], [64]    fc2 [128][64], [128]   fc3 [64][128], [64]   fc4 [32][64], [32]   fc5 [16][32], [16]
 *     action_head [2][16], [2]    type_head [3][16], [3]
 * every hidden layer followed by ReLU.  No other architecture is supported (original_ann.py's 6 -> 500 -> 500 -> 3 and the
 * commented-out variants of EBRD.py are refused by shape).
 */
#ifndef MESHENV_FNN_H
#define MESHENV_FNN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MESHENV_FNN_TENSORS 14            /* seven weights and seven biases */
#define MESHENV_FNN_PACKED_FLOATS 21568   /* the packed buffer: per layer the weight tiles in MFMA B-operand order, then the bias */
#define MESHENV_MOVE_SKIPPED 255          /* code of a finished environment's rows in the histories of meshenv_move_fnn_multi */

typedef struct MeshFnn MeshFnn;
typedef struct MeshEnv MeshEnv;           /* meshenv.h: meshenv_create */

/* A handle on `device` whose launches go to `stream` (a hipStream_t; NULL: the default stream).  MESHENV_E_ARG: out is NULL;
 * MESHENV_E_HIP: no such device. */
int meshenv_fnn_create(int device, void *stream, MeshFnn **out);
/* Waits for the handle's stream, frees the weights and the loop's scratch.  NULL is allowed. */
void meshenv_fnn_destroy(MeshFnn *f);
/* Later launches go to `stream`.  MESHENV_E_ARG: f is NULL. */
int meshenv_fnn_set_stream(MeshFnn *f, void *stream);
/* The last failure on the handle (of meshenv_fnn_create or meshenv_fnn_pack when f is NULL). */
const char *meshenv_fnn_last_error(const MeshFnn *f);

/* The host half of meshenv_fnn_load; needs no GPU.  Packs the fourteen HOST tensors (torch.save(model.state_dict()) of
 * EBRD.py:320 holds exactly these) into out_host[MESHENV_FNN_PACKED_FLOATS]: for layer l = fc1, fc2, fc3, fc4, fc5, heads, one
 * behind the other, the weight as [tile][K / 16][lane 64][4] with element j of lane l in group g =
 * W[n = 16 tile + (l & 15)][k = 4 (4 g + j) + (l >> 4)] (K = 32, 64, 128, 64, 32, 16: fc1's 18 inputs zero-padded), then the
 * bias [16 tiles].  The two heads share one tile: n = 0, 1 the action_head's rows, n = 2, 3, 4 the type_head's; n >= 5 zero.
 *   tensors   MESHENV_FNN_TENSORS pointers: fc1.weight, fc1.bias, ..., fc5.bias, action_head.weight, action_head.bias,
 *             type_head.weight, type_head.bias
 *   shapes    [MESHENV_FNN_TENSORS][2] (rows, columns; a bias is (n, 1))
 * MESHENV_E_ARG: a NULL pointer, or a shape other than the list above (the message names the expected shapes). */
int meshenv_fnn_pack(const float *const *tensors, const int32_t *shapes, float *out_host);

/* Replaces Policy(...).load_state_dict(...) + .to(device) (EBRD.py:517-519): packs the host tensors (meshenv_fnn_pack) and
 * uploads them.  Synchronises the handle's stream first (the previous weights may be in use).  MESHENV_E_ARG as
 * meshenv_fnn_pack; MESHENV_E_HIP: the upload failed. */
int meshenv_fnn_load(MeshFnn *f, const float *const *tensors, const int32_t *shapes);

/* Replaces get_action (EBRD.py:174-177) for n observations: one launch on the handle's stream, no synchronisation.
 *   obs_dev       [n][18] float32: the static observation meshenv_reset_static / meshenv_move return (zeros = None)
 *   finished_dev  NULL, or [n] uint8: where nonzero the env's outputs are written as zeros
 *   points_dev    [n][2] float64 = (double)action, the exact widening tolist() performs
 *   types_dev     [n] float64 = argmax(type logits) / 2 in {0, 0.5, 1}; the lowest index among equal maxima, a NaN logit counts
 *                 as the maximum and the first NaN wins (torch.argmax)
 *   actions_dev   [n][2] float32, logits_dev [n][3] float32: the heads' raw outputs
 * Every output is nullable, one at least is required.  MESHENV_E_STATE: nothing loaded; MESHENV_E_ARG: f is NULL, n < 1,
 * obs_dev NULL or no output; MESHENV_E_HIP: the launch failed. */
int meshenv_fnn_forward(MeshFnn *f, int n, const float *obs_dev, const uint8_t *finished_dev, double *points_dev,
                        double *types_dev, float *actions_dev, float *logits_dev);

/* Replaces T iterations of the loop of EBRD.py:541-548 for every env of h: for t = 0 .. T - 1 a forward on obs_dev and the
 * launches of meshenv_move with its outputs, enqueued on the stream the two handles share.  An env FINISHES at the move
 * that returns done != 0 or code >= MESHENV_MOVE_RAISES (where the reference leaves its loop or raises); from then on it is
 * skipped by every launch of this and of later calls: ring, element log, not_valid_points, last_not_valid_points, cached
 * observation and its row of obs_dev stay exactly as that move left them.  No auto-reset.
 *   obs_dev        [n][18] in / out: the observation of every env (meshenv_reset_static's, or the last call's); each move
 *                  overwrites the rows of the envs it ran
 *   finished_dev   [n] uint8 in / out, steps_dev [n] int32 in / out (moves made, the finishing one included): zero them after
 *                  a reset, pass them back unchanged to continue
 *   done_dev, complete_dev, code_dev   [n] uint8 out: those of each env's LAST move (not written for an env that was finished
 *                  on entry)
 *   n_elements_dev NULL, or [n] int32 out: elements of the env's running episode after its last move (as the three above)
 *   hist_*         NULL, or the per-step histories: points [T][n][2] and types [T][n] float64 as fed to the move, obs [T][n][18]
 *                  the observation the forward read, code / done / complete [T][n] uint8 as the move returned them.  The rows of
 *                  an env behind its last move hold code = MESHENV_MOVE_SKIPPED and zeros.
 * With meshenv_set_timing(h, 1) armed every forward launch is bracketed by one event pair of the handle's pool
 * (meshenv_kernel_times then returns the forwards' own times; the moves are not bracketed).
 * MESHENV_E_STATE: no weights loaded, or the two handles on different devices or streams; MESHENV_E_ARG: a NULL handle or
 * required pointer, T < 1, and what meshenv_move refuses; MESHENV_E_HIP: an allocation or a launch failed. */
int meshenv_move_fnn_multi(MeshEnv *h, MeshFnn *f, int T, float *obs_dev, uint8_t *finished_dev, int32_t *steps_dev,
                           uint8_t *done_dev, uint8_t *complete_dev, uint8_t *code_dev, int32_t *n_elements_dev,
                           double *hist_points_dev, double *hist_types_dev, float *hist_obs_dev, uint8_t *hist_code_dev,
                           uint8_t *hist_done_dev, uint8_t *hist_complete_dev);

#ifdef __cplusplus
}
#endif
#endif /* MESHENV_FNN_H */
