/*
 * oracle/meshenv_ref.h -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Scalar CPU restatement (plain C, host libm) of the reference's
 * element-extraction step()/reset() hot path (rl/boundary_env.py + general/mesh.py +
 * general/components.py + general/data.py; line cites are in meshenv_ref.c and
 * refer to the frozen, logic-identical snapshot v2/src/mesh_rl/legacy/).
 *
 * Parity status: PINNED.  tests/test_oracle_golden.py checks this file
 * bit-for-bit (obs, reward, topology, candidate list) against traces recorded
 * from the reference itself (oracle/gen_golden.py -> tests/golden/ npz files).
 *
 * oracle/meshenv_cpu_shim.c exports the step()/reset()/move() entry points of include/meshenv.h
 * under the same names over this restatement (libmeshenv_cpu.so, host pointers).
 *
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may
 * load this library.  The product library (libmeshenv_hip.so) never links,
 * loads or calls anything declared here.
 */
#ifndef MESHENV_REF_H
#define MESHENV_REF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct RefEnv RefEnv;

/* One environment over one domain polygon (clockwise ring, n0 vertices, xy = [x0,y0,x1,y1,...]).
 * original_area / est_min_l / est_crit_l are the domain constants the reference computes in
 * __init__/reset (Boundary2D.poly_area, MeshGeneration.estimate_area_range); the host computes
 * them (reinforcementlearning4meshgeneration_amd/domains.py) and passes them in.
 * cap_new = capacity of the new-vertex / element logs. */
RefEnv *meshenv_ref_create(int n0, const double *xy, double original_area, double est_min_l,
                           double est_crit_l, int cap_new);
void meshenv_ref_destroy(RefEnv *e);

/* The seven geometry constants of MeshEnvParams (include/meshenv.h), in its order: radius, max_ref_angle, key_lambda,
 * min_degree, max_degree, same_point_eps, ray_length.  meshenv_ref_create sets the reference's literals
 * (4, 0.972*pi, 0.618, 0.01*pi, 0.99*pi, 0.001, 10000); this replaces them and resets the env. */
void meshenv_ref_set_params(RefEnv *e, const double *p /*[7]*/);

/* reset(): rl/boundary_env.py:67-84.  Writes obs[18]; returns 1 if the reference would return None. */
int meshenv_ref_reset(RefEnv *e, float *obs);

/* step(action[3]): rl/boundary_env.py:113-263.  Returns 1 if obs is None in the reference. */
int meshenv_ref_step(RefEnv *e, const float *action, float *obs, double *reward, uint8_t *done,
                     uint8_t *is_complete);

/* reset(static=True), rl/boundary_env.py:67-84 with PointEnvironment(static=True): row 0 of the observation carries 0
 * instead of the area ratio (general/components.py:1213-1218) */
int meshenv_ref_reset_static(RefEnv *e, float *obs, int is_static);

/* move(new_point, type), rl/boundary_env.py:265-432 (the deterministic API the ANN / testbed scripts drive), for
 * Python-float arguments.  point[2] = (radius fraction, angle); see meshenv_ref.c for the return codes. */
enum {
    MESHENV_REF_MOVE_OK = 0, MESHENV_REF_MOVE_NONE = 1, MESHENV_REF_MOVE_RAISES = 2,
    MESHENV_REF_MOVE_NEEDS_SMOOTHING = 3, /* only when the element log overflowed: smooth_pave cannot be run (episode ends) */
    MESHENV_REF_MOVE_SMOOTH_RAISES = 4    /* the reference raises inside smooth_pave (math domain error / division by zero) */
};
int meshenv_ref_move(RefEnv *e, const double *point, double type, float *obs, uint8_t *done, uint8_t *is_complete);
int meshenv_ref_not_valid_count(const RefEnv *e);

/* state readout for parity tests */
int meshenv_ref_ring_len(const RefEnv *e);
void meshenv_ref_get_ring(const RefEnv *e, int32_t *ids, double *xy);
/* smooth_pave(boundary.vertices, updated_boundary.vertices, iteration=..., interior=True), general/mesh.py:790-795:
 * Gauss-Seidel relaxation of the generated vertices off the front + candidate list rebuilt; -1 = log overflow */
int meshenv_ref_smooth_interior(RefEnv *e, int iteration, int32_t *sweeps_out, double *diff_out);
/* MeshGeneration.smooth(boundary.vertices, iteration=...), general/mesh.py:1290-1392 (finished meshes, general/EBRD.py:391);
 * branch_out[3]: vertex visits with 1 / 2 / other numbers of related elements; -2 = the reference raises IndexError */
int meshenv_ref_smooth_final(RefEnv *e, int iteration, double lr_1, double lr_2, int32_t *sweeps_out, double *diff_out,
                             int64_t *branch_out);
/* middle_vertex / side_vertex / indention_vertex (general/mesh.py:805-909) as plain functions, for unit tests */
int meshenv_ref_front_construction(int which, const double *in /*[8]*/, double *out_xy /*[2]*/);
/* smooth_current_boundary_3 (general/mesh.py:939-1028) alone; -3 = the reference raises (ValueError / ZeroDivisionError) */
int meshenv_ref_smooth_front(RefEnv *e);
/* smooth_pave(..., interior=False) + the find_next_state that follows it in move() (rl/boundary_env.py:405-420) */
int meshenv_ref_smooth_pave_full(RefEnv *e, int iteration, int is_static, float *obs, int32_t *sweeps_out);
/* candidate list in the reference's list order: (key asc, insertion desc) */
int meshenv_ref_get_candidates(const RefEnv *e, int32_t *ids, double *keys);
int meshenv_ref_ref_id(const RefEnv *e);
void meshenv_ref_get_scalars(const RefEnv *e, int32_t *n_elem, int32_t *failed_num, int32_t *n_vert,
                             double *current_area);
/* vertex_xy[n_vert*2] (initial ring first, then new vertices), quads[n_elem*4] global ids */
void meshenv_ref_get_elements(const RefEnv *e, int32_t *quads, double *vertex_xy, int32_t *n_elem,
                              int32_t *n_vert);

/* batch driver used by tests and by bench.py's cpu_baseline leg: steps n envs once each,
 * auto-resetting finished ones when auto_reset != 0 (obs then holds the reset obs and
 * terminal_obs, if non-NULL, the last obs).  threads > 1 uses OpenMP when compiled with it. */
/* element quality report (general/components.py:863-933; Measurement/quality_verdict.py:77-90) */
void meshenv_ref_element_quality(const double *xy /*[4][2]*/, double *out /*[8]*/);
double meshenv_ref_quad_quality(const double *xy /*[4][2]*/, int index /* 0, 1, 3, 4, 5 */);
void meshenv_ref_quality_stats(const double *vals /*[n][8]*/, int n, double *stats /*[8][4]*/);

void meshenv_ref_step_batch(RefEnv **envs, int n, const float *actions, float *obs, double *reward,
                            uint8_t *done, uint8_t *is_complete, float *terminal_obs, int auto_reset,
                            int threads);
/* T vector steps in one OpenMP parallel region (cpu_baseline leg of bench.py); outputs of the last step */
void meshenv_ref_rollout_batch(RefEnv **envs, int n, int T, const float *actions /*[T][n][3]*/, float *obs, double *reward,
                               uint8_t *done, uint8_t *is_complete, int auto_reset, int threads);

/* libm calls made by the CALLING thread since the last reset: out[3] = atan2, sin, cos (bench.py reports the
 * reference algorithm's fp64 transcendental count per env-step; meaningful for threads == 1 runs) */
void meshenv_ref_math_calls(uint64_t *out, int reset);

/* primitives exported for unit tests */
double meshenv_ref_round4_py(double x);
double meshenv_ref_round4_np(double x);
float meshenv_ref_round4_npf(float x);
double meshenv_ref_cw(double sx, double sy, double ax, double ay, double bx, double by);
int meshenv_ref_is_cross(const double *a1, const double *a2, const double *b1, const double *b2);

#ifdef __cplusplus
}
#endif
#endif
