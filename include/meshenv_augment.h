/*
 * meshenv_augment.h -- C-ABI of the synthetic-sample generator of libmeshenv_hip.so: the training set of the supervised mesher,
 * MeshAugmentation.sampling / sampling_main of the reference's general/data_augmentation.py, drawn, scored and selected on
 * the device (csrc/meshenv_augment.h).  The conventions are those of meshenv.h (return codes
 * MESHENV_E_*, *_dev device pointers owned by the caller, one GPU and one stream per handle, no CPU fallback); the entry
 * points live in a header of their own because they bind to no environment.
 *
 * Types are indexed t = 0, 1, 2 for the reference's type labels 0.5, 0, 1 (the order sampling() concatenates them in), angle
 * bins b = 0 .. 10 for the keys 0.4, 0.6, .., 2.4, workers w = 0 .. pool - 1.  Bin g = (w * 3 + t) * 11 + b.
 */
#ifndef MESHENV_AUGMENT_H
#define MESHENV_AUGMENT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MESHENV_AUGMENT_PHILOX_TAG 5   /* fourth Philox counter word of every draw: a stream of its own */
#define MESHENV_AUGMENT_BINS 11
#define MESHENV_AUGMENT_TYPES 3
#define MESHENV_AUGMENT_MAX_ACTIONS 20 /* candidates of a type-0.5 proposal; 1 for types 0 and 1 */
#define MESHENV_AUGMENT_UNIFORMS 57    /* uniforms of a type-0.5 proposal; 17 for types 0 and 1 */
#define MESHENV_AUGMENT_MAX_POOL 1024
#define MESHENV_AUGMENT_MAX_ROUND 1048576 /* proposals of one bin in one round */
#define MESHENV_AUGMENT_MAX_ROUNDS 4095   /* so that a bin's proposal index stays below 2^32 */
#define MESHENV_AUGMENT_STATS 4        /* proposals drawn, candidates scored, rows written, rounds taken */

typedef struct MeshAugment MeshAugment;

int meshenv_augment_create(int device, void *stream, MeshAugment **out);
void meshenv_augment_destroy(MeshAugment *a);
int meshenv_augment_set_stream(MeshAugment *a, void *stream);
/* The last failure on the handle (of meshenv_augment_create when a is NULL). */
const char *meshenv_augment_last_error(const MeshAugment *a);

/* compute_quality and estimate_max_quality(method=3) of n caller-given candidates (data_augmentation.py:447-513 with
 * sample_2_vertices :356-383, check_intersection :521-537, check_internal_element :539-552, compute_boundary_quality
 * :554-642), and check_obs_quality (:291-315) of their observations.  obs_dev [n][18], act_dev [n][3] float64.
 * rejected_dev, valid_dev [n] uint8; q_dev [n][4] float64 = ele, boundary, max_ele, max_boundary (ele = boundary = 0 for an
 * invalid element, as the reference returns); accept_dev [n] uint8 or NULL: the test of :255 at `threshold`.  Where the
 * reference raises (a reflex corner at the origin) the maxima are NaN and accept is 0.  One launch, no synchronisation. */
int meshenv_augment_score(MeshAugment *a, int n, const double *obs_dev, const double *act_dev, double threshold,
                          uint8_t *rejected_dev, uint8_t *valid_dev, double *q_dev, uint8_t *accept_dev);

/* The proposal maps on recorded uniforms (for tests): random (:317-318), the bin angle (:235), sample_state (:29-63),
 * sample_action (:65-77), check_obs_quality.  uniforms_dev [n][57] float64 in draw order (types 0 and 1 read 17), t_dev,
 * b_dev [n] int32 -> angle_dev [n], obs_dev [n][18], act_dev [n][20][3] (rows past the type's count are zero) float64,
 * rejected_dev [n] uint8.  MESHENV_E_ARG for an index out of range (t_host / b_host: the same indices in host memory, checked
 * before the launch). */
int meshenv_augment_propose(MeshAugment *a, int n, const double *uniforms_dev, const int32_t *t_dev, const int32_t *b_dev,
                            const int32_t *t_host, const int32_t *b_host, double *angle_dev, double *obs_dev, double *act_dev,
                            uint8_t *rejected_dev);

/* sampling_main(pool, n, threshold) (:956-986; pool = 1: sampling(n, threshold), :131-176, over sampling_4_type, :223-289).
 * Every bin owes Q - 1 rows, Q = ceil(frac_t * (n / pool) / 11) with frac = 0.5, 0.25, 0.25: the reference counts an accepted
 * candidate before it appends it and leaves at the quota.  The rows of bin g are the first Q - 1 accepted candidates in
 * (proposal, action) order of the Philox stream (seed, w, t, b), whatever round_size is; they are written at their final
 * offsets, ordered worker, type 0.5 / 0 / 1, bin, acceptance: x [R][18] = the observation, y [R][3] = (type, out0, out1), as
 * float64 (x64_dev, y64_dev) and / or float32 (x32_dev, y32_dev); at least one pair is required.  `rows` must be the R the
 * formula gives.  A round draws 33 * pool * round_size proposals, shared equally among the unfinished bins (round_size each in
 * the first round, more as bins finish, at most 2^20 each); after each round the 33 * pool counts are read back (the one
 * synchronisation per round), and after max_rounds rounds with a bin still short the call returns MESHENV_E_RANGE -- the
 * reference would spin forever -- with the rows found so far in place; the handle stays usable.
 * counts_host [33 * pool] (may be NULL): rows written per bin.  stats_host [4] (may be NULL): MESHENV_AUGMENT_STATS, counted
 * on the device.  MESHENV_E_ARG: n < 0, pool outside 1 .. 1024, threshold outside (0, 1], round_size outside 64 .. 2^20 or no
 * multiple of 64, max_rounds outside 1 .. 4095, a wrong `rows`. */
int meshenv_augment_sample(MeshAugment *a, int64_t n, double threshold, uint64_t seed, int pool, int round_size, int max_rounds,
                           int64_t rows, double *x64_dev, double *y64_dev, float *x32_dev, float *y32_dev, int32_t *counts_host,
                           uint64_t *stats_host);

#ifdef __cplusplus
}
#endif
#endif /* MESHENV_AUGMENT_H */
