/*
 * meshenv_fnn_train.h -- C-ABI of the training half of the supervised element-extraction network ("FNN mesher") of
 * libmeshenv_hip.so: the loss of general/EBRD.py's train_ch3 (:272-320) for one minibatch of n rows,
 *     action, logits = model(x)                                                    # Policy, meshenv_fnn.h
 *     loss = CrossEntropyLoss(reduction='sum')(logits, cls) + MSELoss(reduction='sum')(action, y[:, 1:])
 *     loss.backward()
 * with y [.][3] = (type, out0, out1) and cls = 2 type for type in {0, 0.5, 1} (map_type_to_tensors), as two launches
 * (csrc/meshenv_fnn_grad.h: k_fnn_grad, k_fnn_grad_reduce), and the refresh of a loaded MeshFnn from
 * the live tensors an optimiser steps.  The optimiser step itself is meshenv_optim.h's.  The conventions are those of
 * meshenv.h (return codes MESHENV_E_*, *_dev device pointers owned by the caller, one GPU and one stream per handle, no
 * CPU fallback); the entry points live in a header of their own: meshenv.h, meshenv_fnn.h and MESHENV_ABI_VERSION are
 * unchanged.
 *
 * The network is meshenv_fnn.h's (float32, torch.nn.Linear layout), its fourteen tensors in the order of
 * MESHENV_FNN_TENSORS.  Every tensor is read LIVE at each call through the pointer recorded by the bind: optimisers that
 * write in place need no new bind.
 */
#ifndef MESHENV_FNN_TRAIN_H
#define MESHENV_FNN_TRAIN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MESHENV_FNN_GRAD_FLOATS 20544    /* the gradient buffer: 20 485 gradients padded to a multiple of 64 */
#define MESHENV_FNN_GRAD_OUTPUTS 4       /* floats of out_dev and of accum_dev */
#define MESHENV_FNN_GRAD_MAX_GROUPS 128  /* workgroups of k_fnn_grad: min(ceil(n / 16), 128) */

typedef struct MeshFnnGrad MeshFnnGrad;
typedef struct MeshFnn MeshFnn;          /* meshenv_fnn.h: meshenv_fnn_create */

/* A handle on `device` whose launches go to `stream` (a hipStream_t; NULL: the default stream).  MESHENV_E_ARG: out is
 * NULL; MESHENV_E_HIP: no such device. */
int meshenv_fnn_grad_create(int device, void *stream, MeshFnnGrad **out);
/* Waits for the handle's stream, frees the workspace.  NULL is allowed. */
void meshenv_fnn_grad_destroy(MeshFnnGrad *g);
/* Later launches go to `stream`.  MESHENV_E_ARG: g is NULL. */
int meshenv_fnn_grad_set_stream(MeshFnnGrad *g, void *stream);
/* The last failure on the handle (of meshenv_fnn_grad_create when g is NULL). */
const char *meshenv_fnn_grad_last_error(const MeshFnnGrad *g);

/* Binds the live tensors of model.parameters() and the gradient buffer.
 *   tensors_dev  MESHENV_FNN_TENSORS pointers: fc1.weight [64][18], fc1.bias [64], ..., fc5.bias, action_head.weight [2][16],
 *                action_head.bias [2], type_head.weight [3][16], type_head.bias [3]
 *   grad_dev     n_grad = MESHENV_FNN_GRAD_FLOATS floats, which every meshenv_fnn_grad_backward OVERWRITES with the
 *                gradients in tensors_dev's order and torch's layout, one tensor behind the other from float 0; the padding
 *                is not written
 * The first bind allocates the workspace: MESHENV_FNN_GRAD_MAX_GROUPS partial gradient sets.
 * MESHENV_E_ARG: g is NULL, a NULL pointer, another n_grad, or a weight behind fc1's off 16-byte alignment (they are read 16
 * bytes at a time); MESHENV_E_HIP: the allocation failed. */
int meshenv_fnn_grad_bind(MeshFnnGrad *g, const float *const *tensors_dev, float *grad_dev, int64_t n_grad);

/* The loss of n rows and its gradients: two launches on the handle's stream, no synchronisation, no argument written but
 * out_dev, accum_dev and the bound gradient buffer.
 *   x_dev, y_dev  [N][18], [N][3] float32: the samples (meshenv_extract_samples with n_neighbor = n_radius = 3 gives these
 *                 21 columns)
 *   rows_dev      NULL: the minibatch is rows 0 .. n - 1; or [n] int32: row i of the minibatch is x[rows[i]], y[rows[i]]
 *   out_dev       [4] float32: loss, classification loss, regression loss (sums over the rows, as reduction='sum' gives
 *                 them), and the rows whose argmax(logits) equals cls
 *   accum_dev     NULL, or [4] float32 to which out is ADDED by the one thread that writes out (an epoch's sums)
 * A row whose type is none of 0, 0.5, 1, or whose rows entry lies outside [0, N), adds nothing to any gradient or sum; the
 * caller is expected to have refused such data.  No floating-point atomics: the same inputs give the same bits.
 * MESHENV_E_STATE: nothing bound; MESHENV_E_ARG: g is NULL, a NULL required pointer, n < 1, n > N with rows_dev NULL, or N
 * beyond 2^24; MESHENV_E_HIP: a launch failed. */
int meshenv_fnn_grad_backward(MeshFnnGrad *g, int n, int N, const float *x_dev, const float *y_dev, const int32_t *rows_dev,
                              float *out_dev, float *accum_dev);

/* Records the live tensors (tensors_dev as meshenv_fnn_grad_bind takes them) a LOADED MeshFnn refreshes its packed buffer
 * from.  MESHENV_E_STATE: nothing loaded (meshenv_fnn_load lays the buffer out and zeroes its padding); MESHENV_E_ARG: f is
 * NULL or a NULL pointer. */
int meshenv_fnn_bind(MeshFnn *f, const float *const *tensors_dev);
/* One launch on the handle's stream: packs the bound tensors, as they are when the launch runs, into the packed buffer in
 * exactly the layout meshenv_fnn_pack builds on the host.  No host copy, no synchronisation.  MESHENV_E_STATE: nothing
 * bound; MESHENV_E_HIP: the launch failed. */
int meshenv_fnn_refresh(MeshFnn *f);

#ifdef __cplusplus
}
#endif
#endif /* MESHENV_FNN_TRAIN_H */
