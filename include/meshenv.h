/*
 * meshenv.h -- C-ABI of libmeshenv_hip.so: the MI355X-native, vectorised replacement for the
 * reference's BoudaryEnv step()/reset() hot path.
 *
 * The reference (ZhuoQiuMcgill/ReinforcementLearning4MeshGeneration) is pure Python and has no
 * FFI layer; the boundary it exposes for this path is the Gym class surface
 *   rl/boundary_env.py:18     class BoudaryEnv(MeshGeneration, gym.Env)
 *   rl/boundary_env.py:67-84  reset()            -> meshenv_reset
 *   rl/boundary_env.py:113-263 step(action)      -> meshenv_step
 *   rl/baselines/dummy_vec_env.py:41-51 step_wait (the vectorised caller)  -> one meshenv_step per call
 * so every entry point below cites the Python method it replaces.  INTEGRATION.md shows the
 * ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns 0 on success, a negative MESHENV_E_* code on failure;
 *     meshenv_last_error() returns a human-readable message for the last failure on that handle
 *     (or for a failed meshenv_create when passed NULL);
 *   - pointers named *_dev are DEVICE pointers (e.g. torch.Tensor.data_ptr() of a tensor on the
 *     handle's GPU), owned by the caller, and must stay valid until the stream work that uses
 *     them has completed; pointers named *_host are host pointers;
 *   - a handle is bound to one GPU and one HIP stream; all work is stream-ordered on that stream;
 *     handles are not thread-safe;
 *   - there is no CPU fallback: every call fails with MESHENV_E_HIP if the GPU is unavailable.
 */
#ifndef MESHENV_H
#define MESHENV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MESHENV_ABI_VERSION 1

#define MESHENV_OBS_DIM 18 /* observation_space shape, rl/boundary_env.py:38-39 */
#define MESHENV_ACT_DIM 3  /* action_space shape, rl/boundary_env.py:27 */

enum {
    MESHENV_OK = 0,
    MESHENV_E_ARG = -1,    /* bad argument (null pointer, size out of range, unsupported parameter) */
    MESHENV_E_HIP = -2,    /* a HIP runtime call failed / no usable GPU */
    MESHENV_E_RANGE = -3,  /* env / domain index out of range */
    MESHENV_E_STATE = -4   /* call not valid in the handle's current state */
};

/* per-env status bits returned by meshenv_get_status() */
enum {
    MESHENV_ST_NO_REFERENCE = 1, /* candidate list empty: the reference's find_next_state() returned None
                                    (rl/boundary_env.py:569-571); obs is all zeros */
    MESHENV_ST_LOG_OVERFLOW = 2  /* more elements / new vertices than log_capacity; counts stay exact,
                                    the log holds the first log_capacity entries */
};

/* Constants of rl/boundary_env.py:26-56, general/mesh.py:26-28 and general/components.py:721-722.
 * meshenv_default_params() fills the reference's values.  neighbor_num and radius_num fix the
 * observation layout and must stay 6 and 3. */
typedef struct MeshEnvParams {
    int32_t struct_size;        /* sizeof(MeshEnvParams), for ABI checking */
    int32_t neighbor_num;       /* 6    rl/boundary_env.py:32 */
    int32_t radius_num;         /* 3    rl/boundary_env.py:33 */
    int32_t fail_limit;         /* 100  rl/boundary_env.py:260 */
    int32_t log_capacity;       /* elements (and new vertices) logged per env per episode; 0 = no log */
    int32_t reserved;
    double radius;              /* 4      rl/boundary_env.py:35 */
    double max_ref_angle;       /* 0.972*pi  general/mesh.py:26 */
    double key_lambda;          /* 0.618  general/mesh.py:213 */
    double min_degree;          /* 0.01*pi general/components.py:722 */
    double max_degree;          /* 0.99*pi general/components.py:721 */
    double same_point_eps;      /* 0.001  rl/boundary_env.py:601 */
    double ray_length;          /* 10000  general/mesh.py:540 */
} MeshEnvParams;

typedef struct MeshEnv MeshEnv; /* opaque */

void meshenv_default_params(MeshEnvParams *p);

int meshenv_abi_version(void);

/* Number of HIP devices visible (0 if none / runtime unusable). */
int meshenv_device_count(void);

/*
 * Construct n_envs environments over n_domains polygons.
 * Replaces BoudaryEnv.__init__ (rl/boundary_env.py:21-65) + MeshGeneration.__init__
 * (general/mesh.py:17-30) for a whole batch.
 *
 *   dom_offsets_host[n_domains+1]  vertex offsets of each domain ring in dom_xy_host
 *   dom_xy_host[2*total]           clockwise rings, (x, y) interleaved, float64
 *   dom_consts_host[3*n_domains]   per domain: original_area, est_min_l, est_crit_l
 *                                  (Boundary2D.poly_area, general/components.py:477-479;
 *                                   MeshGeneration.estimate_area_range, general/mesh.py:679-692)
 *   env_domain_host[n_envs]        domain index of every environment
 *   stream                         hipStream_t to bind (NULL = the device's default stream)
 *
 * The environments come up already reset (their first observation is available through
 * meshenv_reset with a NULL mask).
 */
int meshenv_create(int device, int n_domains, const int32_t *dom_offsets_host, const double *dom_xy_host,
                   const double *dom_consts_host, int n_envs, const int32_t *env_domain_host,
                   const MeshEnvParams *params, void *stream, MeshEnv **out);

/*
 * The same with one GENERATED domain per environment (BASELINE.json configs[4]: ui/GenerateRandomPolygon.py envs with
 * variable vertex count): env k runs on the polygon of Python's random.Random(seed0 + k) --
 *   generatePolygon(250, 250, 100, 0.55, 0.7, numVerts)   ui/GenerateRandomPolygon.py:5-49, 63 (numVerts = num_verts, or
 *                                                         randint(8, 64) from the same stream when num_verts == 0)
 *   consecutive duplicate pixels dropped, coordinates / 100 (general/polygon.py:110-117), made clockwise by the
 *   drawing UI's rule (ui/tk-ui.py:84-101, 169-176), every edge split into ceil(length / edge) equal pieces with an even
 *   vertex total, coordinates rounded to 4 places --
 * generated, and its constants (poly_area, estimate_area_range) computed, on the device (csrc/meshenv_domgen.h); the host
 * side is only a prefix sum over the ring lengths.  reinforcementlearning4meshgeneration_amd.domains.random_domain(seed)
 * is the host restatement of the same ring (bit-identical; tests/test_gpu_domgen.py).  Fails with MESHENV_E_STATE if a
 * polygon keeps fewer than 5 distinct pixels (the host function would draw another one from the stream).
 */
int meshenv_create_random(int device, int n_envs, uint64_t seed0, int num_verts, double edge, const MeshEnvParams *params,
                          void *stream, MeshEnv **out);

/*
 * The same generator followed by the REFERENCE's densification instead of the uniform split: Density.calculate_density
 * (ui/tk-ui.py:252-276; arithmetic-progression spacing from density(prev) * base_length to density(k) * base_length on
 * every edge, Python round half-to-even, one middle point dropped on the last edge for an even total), the UI's
 * clockwise rule on the result (:84-101, 169-176) and read_polygon's / 100 (general/polygon.py:110-117) -- the route
 * reinforcementlearning4meshgeneration_amd.domains.density_domain(random_polygon_px(seed), base_length) restates on the
 * host, bit-identical (tests/test_gpu_domgen.py).  base_length is in PIXELS (45 = the 0.45 spacing of the uniform mode),
 * density the value every generated vertex carries.  Where the reference raises ZeroDivisionError -- an edge of 0.5 - 1.5
 * spacings gets round(...) == 0 interior points and (B - A) / 0 -- no environment can be built:
 *   seeds_host   [n_envs] nullable: the seed of every ring (NULL: seed0 + k), so that a caller can leave those seeds out
 *   raises_host  [n_envs] nullable: 1 where calculate_density raises for that ring; 2 where the polygon itself is not
 *                generated on the device (fewer than 5 distinct pixels: the host function would draw another one)
 *   out          nullable: NULL = probe only (fills raises_host, builds nothing)
 * Returns MESHENV_E_STATE, *out = NULL and raises_host filled if any ring raises (MeshVecEnv.from_random_density probes a
 * seed range first and then passes the seeds that are defined).  cos / sin of the edge directions come from the host
 * libm (integer pixel offsets: a finite table), so the rings are the reference's bit for bit.
 */
int meshenv_create_random_density(int device, int n_envs, uint64_t seed0, const uint64_t *seeds_host, int num_verts,
                                  double base_length, double density, const MeshEnvParams *params, void *stream, MeshEnv **out,
                                  uint8_t *raises_host);

/*
 * Density.calculate_density + clockwise rule + / 100 for EXPLICIT pixel polygons with per-vertex densities (handle-free,
 * synchronous; the drawn-domain route of ui/tk-ui.py):
 *   poly_offsets_host [n_polys+1], pixels_host [2*total] float64 (x, y), integer_pixels != 0: the coordinates are Python
 *   ints (the UI's event coordinates; then every value must be integral) -- the reference's arithmetic differs between
 *   int and float operands (exact int squares and an int 0 in atan2 against pow(x, 2.0) and -0.0),
 *   densities_host [total] nullable (1.0),
 *   count_host [n_polys] ring lengths, status_host [n_polys]: 0 ok, 1 the reference raises ZeroDivisionError (an edge of
 *   0.5 - 1.5 spacings, or two adjacent vertices of density 0), 2 more than 2048 ring points, 3 fewer than 3 distinct pixels; xy_host [2*cap_points] nullable: the rings of the polygons with
 *   status 0, back to back in polygon order (MESHENV_E_RANGE if they do not fit).  3..256 vertices per polygon.
 */
int meshenv_density_rings(int device, int n_polys, const int32_t *poly_offsets_host, const double *pixels_host, int integer_pixels,
                          const double *densities_host, double base_length, int32_t *count_host, uint8_t *status_host,
                          double *xy_host, int64_t cap_points);

/* Host-side readout of one domain of the handle's table (synchronises the stream): xy_host[2*cap_points] receives the
 * ring, *n_out its length, consts_host[3] (nullable) original_area, estimated_area_range[0]**2, [1]**2. */
int meshenv_get_domain(MeshEnv *h, int domain, double *xy_host, int cap_points, int32_t *n_out, double *consts_host);

void meshenv_destroy(MeshEnv *h);

const char *meshenv_last_error(const MeshEnv *h);

/* Rebind the handle to another HIP stream (e.g. torch.cuda.current_stream().cuda_stream). */
int meshenv_set_stream(MeshEnv *h, void *stream);

int meshenv_num_envs(const MeshEnv *h);
int meshenv_max_ring(const MeshEnv *h);
/* Environments per workgroup of the single-step kernel: 1 = k_step<false> (one wave per workgroup), 8 / 16 =
 * k_step_group<G> (chosen at creation from n_envs, see meshenv_create in csrc/meshenv_hip.hip). */
int meshenv_group_size(const MeshEnv *h);
/* Which kernel meshenv_step launches next, as a code.  csrc/meshenv_step_variant.h is the one table of the instantiations
 * behind the codes, the rule that selects them and the names below; the codes keep their numbers (2 is retired).
 *  0  k_step, one wave per env                      1  k_step_group<G>, G = meshenv_group_size envs per workgroup
 *  3  k_step after a front smoothing (meshenv_smooth with interior = 0, or a meshenv_move through smooth_pave) and until
 *     ALL envs are reset: rings may hold vertices off the 1e-4 lattice, the kernel breaks angle ties like the reference's libm
 *  4  k_step_group<16>, LDS packed by each ring's own length (mixed domains whose sixteen longest rings exceed one CU)
 *  5 / 6  1 / 0 for ring strides of at most 64 slots (every ring pass is one 64-lane pass)
 *  7 / 8  0 / 6 in the throughput regime (record-first staging, from 8192 envs)
 *  9 / 10  0 / 3 of handles with non-default geometry constants (MeshEnvParams), read at run time */
int meshenv_step_kernel(const MeshEnv *h);
/* Which kernel meshenv_rollout (n_steps > 1) launches: 0 = k_step<true>, 1 = ring stride <= 64, 2 = non-default geometry
 * constants, 3 / 4 = after a front smoothing with default / non-default constants. */
int meshenv_rollout_kernel(const MeshEnv *h);
/* The same two answers as the kernel's name, as rocprofv3 prints it ("meshenv::k_step<false, true, false, false, false>"):
 * a static string, NULL for a NULL handle. */
const char *meshenv_step_kernel_name(const MeshEnv *h);
const char *meshenv_rollout_kernel_name(const MeshEnv *h);
/* The smoothing kernels evaluate `x ** 2` like the reference's libm (CPython's float ** 2 is pow(x, 2.0), which glibc does
 * not round correctly: it differs from x * x in 0.085 % of the arguments) through a restatement of glibc's pow
 * (csrc/meshenv_libm.h) that the library validates against the libm of the running process at the first smoothing call.
 * Returns 1: validated, the smoothers square as the reference does; 0: this libm computes pow differently (or
 * MESHENV_LIBM_EXACT=0 is set), the smoothers use x * x and agree with the reference to one ulp per squaring instead of
 * bit for bit; -1: not checked yet (no smoothing call so far).  The reference has no counterpart: it IS that libm. */
int meshenv_libm_exact(const MeshEnv *h);
/* Every clockwise angle (Vertex.to_find_clockwise_angle, general/components.py:99-108) is -atan2(cross, dot) rounded to
 * 1e-4 rad.  The kernels take ocml's atan2, which is within an ulp of the libm the reference calls, and re-evaluate the
 * few angles that sit on a rounding boundary (k + 0.5) e-4 -- the front smoother constructs such angles -- with a
 * restatement of glibc's atan2 (csrc/meshenv_libm.h) whose table is read from the libm image of the running process and
 * which is validated against that libm's atan2 when the first handle is created.  Returns 1: validated, the quantised
 * angles are the reference's in every case; 0: table not found / another algorithm (the boundary cases then take a
 * correctly rounded atan2, which agrees with glibc's in 99.93 % of them), or MESHENV_LIBM_EXACT=0 (ocml only).
 * Host-only: needs no GPU. */
int meshenv_atan2_exact(void);

/*
 * reset(): rl/boundary_env.py:67-84 for every env whose mask byte is non-zero (all envs when
 * mask_dev is NULL).  obs_dev[n_envs*18] receives the first observation of the reset envs and the
 * current observation of the others.
 */
int meshenv_reset(MeshEnv *h, const uint8_t *mask_dev, float *obs_dev);

/*
 * reset(static=True): rl/boundary_env.py:67 -> find_next_state(static=static) -> PointEnvironment(static=True)
 * (general/components.py:1213-1218): observation entry 1 (row 0, second value) carries 0 instead of the area ratio.
 * is_static = 0 is meshenv_reset.  Also empties the move() API's not_valid_points of the reset envs
 * (rl/boundary_env.py:73).
 */
int meshenv_reset_static(MeshEnv *h, const uint8_t *mask_dev, float *obs_dev, int is_static);

/*
 * step(): rl/boundary_env.py:113-263 for all envs, one kernel launch.
 *   actions_dev[n_envs*3] float32   (rule type, x, y) as SB3 hands them over
 *   obs_dev[n_envs*18]    float32   next observation (after auto-reset: the first observation of
 *                                   the new episode, like SB3's DummyVecEnv)
 *   reward_dev[n_envs]    float64   the reference returns np.float64 (rl/boundary_env.py:263)
 *   done_dev[n_envs]      uint8
 *   complete_dev[n_envs]  uint8     info['is_complete']
 *   terminal_obs_dev      nullable; for envs with done != 0 receives the last observation of the
 *                         finished episode (SB3's infos[k]["terminal_observation"])
 *   auto_reset            non-zero: envs that finish are reset inside the same launch
 */
int meshenv_step(MeshEnv *h, const float *actions_dev, float *obs_dev, double *reward_dev, uint8_t *done_dev,
                 uint8_t *complete_dev, float *terminal_obs_dev, int auto_reset);

/*
 * n_steps consecutive step() calls in ONE launch (environments are independent, so a wave can
 * advance its env without any inter-wave synchronisation).  actions_dev is [n_steps][n_envs][3];
 * reward_dev/done_dev/complete_dev are [n_steps][n_envs]; obs_dev[n_envs*18] receives the
 * observation after the last step; auto_reset as in meshenv_step.  Used for open-loop (scripted /
 * random-policy) rollouts; a policy in the loop calls meshenv_step.
 */
int meshenv_rollout(MeshEnv *h, int n_steps, const float *actions_dev, float *obs_dev, double *reward_dev,
                    uint8_t *done_dev, uint8_t *complete_dev, int auto_reset);

/*
 * move(new_point, type): rl/boundary_env.py:265-432, the deterministic extraction API the reference's ANN / testbed
 * scripts drive, for all envs in one launch and for Python-float arguments:
 *   points_dev[n_envs*2]  float64  (radius fraction, angle): the candidate point is
 *                                  base_length * radius * r * (cos a, sin a) in the reference vertex's frame, rounded
 *                                  to 6 places, scale 1 (rl/boundary_env.py:266-269, 105)
 *   type_dev[n_envs]      float64  rule selector: <= 0.3 the rule -1 quad, >= 0.7 the rule +1 quad, else the new point
 *                                  (TYPE_THRESHOLD, rl/boundary_env.py:19, 286-310; no find_same_point here)
 *   obs_dev[n_envs*18]    float32  next observation, static form (see meshenv_reset_static)
 *   done_dev / complete_dev        done: ring <= 5 after a valid move; complete: ring <= 4
 *   code_dev[n_envs]      uint8    MESHENV_MOVE_*
 * The reward is always 0 in the reference and is not returned.  A rejected move appends the reference vertex to the
 * env's not_valid_points, which the next selection skips (general/mesh.py:284-288); a valid move empties the list.
 * current_area and failed_num are not touched (the reference's move() does not).  No auto-reset: reset the envs with
 * done != 0 or code >= MESHENV_MOVE_RAISES through meshenv_reset_static with a mask.
 */
enum {
    MESHENV_MOVE_OK = 0,
    MESHENV_MOVE_NONE = 1,            /* the observation is None (zeros): no reference vertex on a ring of <= 4 */
    MESHENV_MOVE_RAISES = 2,          /* ring <= 5 (or no reference vertex) on entry: the reference raises
                                         UnboundLocalError (`is_complete` unbound, rl/boundary_env.py:283-285, 432);
                                         nothing is changed, the cached observation is returned */
    MESHENV_MOVE_NEEDS_SMOOTHING = 3, /* only on handles without a usable element log (log_capacity = 0, overflow, or
                                         too large for the smoother's LDS): the smooth_pave below cannot be run and the
                                         episode ends instead, done = 1, complete = 0 */
    MESHENV_MOVE_SMOOTH_RAISES = 4    /* the reference raises out of this move(): inside that smooth_pave
                                         (MESHENV_SMOOTH_RAISES below) or, after a smooth_pave that accepted a NaN vertex
                                         (MESHENV_SMOOTH_NONFINITE), in the find_next_state that follows it -- in the
                                         second case not_valid_points has already been emptied, :416-422; done = 1, the
                                         caller resets */
};
/* No selectable reference vertex on a front of more than 4 vertices (every candidate is listed in not_valid_points):
 * the reference runs smooth_pave (front + interior smoothing, candidate rebuild; rl/boundary_env.py:405-412), ends the
 * episode if not_valid_points repeats the list of the previous such smoothing (first entry, last entry and length;
 * last_not_valid_points survives reset(), :416-420), empties the list and selects again (:422-426).  meshenv_move does
 * the same in the same call (the kernels of meshenv_smooth under a mask of those envs); such a move returns
 * MESHENV_MOVE_OK / MESHENV_MOVE_NONE like any other. */
int meshenv_move(MeshEnv *h, const double *points_dev, const double *type_dev, float *obs_dev, uint8_t *done_dev,
                 uint8_t *complete_dev, uint8_t *code_dev);

/* MeshGeneration.smooth_pave(boundary.vertices, updated_boundary.vertices, iteration=..., interior=...),
 * general/mesh.py:790-795, on the RUNNING episode (which = 0) of every env with mask_dev[e] != 0 (mask_dev NULL: all).  The
 * Vertex.segments graph the reference walks is rebuilt from the element log, so the handle needs log_capacity > 0.
 *
 * interior != 0 (the post-processing call of general/EBRD.py:393): smooth_fixed_vertices (general/mesh.py:1258-1288) --
 *   Gauss-Seidel relaxation of the generated vertices that are off the front, in boundary.vertices order, until the moved
 *   vertices' coordinate sum changes by <= 0.001 or `iteration` sweeps -- then find_reference_candidates(0)
 *   (general/mesh.py:233-261) on the front.  The front, the reference vertex and the observation are unchanged (as in the
 *   reference), the candidate list is the rebuilt one; the first step after the call must be a meshenv_step or meshenv_step_actor, not a meshenv_rollout (it commits
 *   the re-selection the rebuild parked: the reference re-selects at the end of every step, accepted or not).
 *   is_static and obs_dev are ignored.
 * interior == 0 (what move() runs when no reference vertex is selectable, rl/boundary_env.py:405-420):
 *   smooth_current_boundary_3 (general/mesh.py:939-1028) moves the generated vertices ON the front first, then the two
 *   steps above; because the front moved, the point environment is recomputed at once -- find_next_state(static =
 *   is_static != 0), the call move() makes right after smooth_pave -- and obs_dev [n_envs][18] (nullable) receives its
 *   observation (zeros where the reference returns None: status bit MESHENV_ST_NO_REFERENCE).
 *
 * which = 1 (interior != 0 only): the same relaxation on the ARCHIVED episode of every selected env (the mesh
 *   meshenv_get_last_episode reads, e.g. an episode that auto-reset ended by truncation); its front is recovered from the
 *   logs (vertices on edges used an odd number of times by domain ring + elements); no candidate list is involved;
 *   MESHENV_SMOOTH_NOT_FINISHED where nothing is archived yet.
 *
 * The vertex log (meshenv_get_elements, meshenv_element_quality) holds the moved coordinates afterwards.
 *   sweeps_dev [n_envs] int32, nullable: sweeps of the interior relaxation; MESHENV_SMOOTH_SKIPPED for masked-out envs;
 *              MESHENV_SMOOTH_LOG_OVERFLOW (status bit MESHENV_ST_LOG_OVERFLOW: graph incomplete) and
 *              MESHENV_SMOOTH_DEGREE (a vertex with more than 16 neighbours) leave the env untouched;
 *              MESHENV_SMOOTH_RAISES: the reference raises inside a vertex construction of the front smoother
 *              (math.sqrt of a negative number; a zero divisor between Python operands, i.e. two coincident DOMAIN
 *              vertices) -- the vertices moved before that point stay moved, nothing else ran.  A zero divisor with a
 *              NumPy-scalar operand (the coordinates of generated vertices are np.float64) only warns in the reference
 *              and yields nan: reproduced -- the nan position fails is_inside_boundary and the vertex stays where it
 *              is -- except where the reference ACCEPTS the nan position (every test against the surrounding polygon
 *              reads False for the original position too): MESHENV_SMOOTH_NONFINITE, the smoother stops at that vertex;
 *              the reference goes on with a NaN vertex and raises in its next find_next_state (int(nan),
 *              general/components.py:1249)
 *   diff_dev   [n_envs] float64, nullable: the last |sum - previous sum| (what the reference prints) */
enum {
    MESHENV_SMOOTH_SKIPPED = -1, MESHENV_SMOOTH_LOG_OVERFLOW = -2, MESHENV_SMOOTH_DEGREE = -3,
    MESHENV_SMOOTH_NOT_FINISHED = -4, /* meshenv_smooth_final on a front of more than 5 vertices */
    MESHENV_SMOOTH_INDEX_ERROR = -5,  /* the reference raises IndexError here (empty common-neighbour list) */
    MESHENV_SMOOTH_RAISES = -6,
    MESHENV_SMOOTH_NONFINITE = -7
};
int meshenv_smooth(MeshEnv *h, int which, const uint8_t *mask_dev, int iteration, int interior, int is_static,
                   int32_t *sweeps_dev, double *diff_dev, float *obs_dev);

/* MeshGeneration.smooth(boundary.vertices, lr_1, lr_2, iteration), general/mesh.py:1290-1392 -- the post-processing of a
 * FINISHED mesh (general/EBRD.py:391: front of <= 5 vertices) -- on every env with mask_dev[e] != 0:
 *   which = 0: the running episode, ended complete and not reset yet (step with auto_reset = 0, smooth, read, reset);
 *   which = 1: the archived episode (what meshenv_get_last_episode reads: the finished mesh auto-reset left behind); its
 *              front, of which smooth() only needs the membership, is recovered from the logs (the vertices on edges used
 *              an odd number of times by domain ring + elements; a front of 4 closed by the last element = that element).
 * Every generated vertex, front vertices included, by the number of elements around it -- 4th-vertex estimates for 1 and 2
 * (general/mesh.py:1305-1361), the Laplacian step otherwise -- until the coordinate sum of the whole vertex list changes by
 * <= 0.001 or `iteration` sweeps.  The reference's defaults are lr_1 = lr_2 = 0.999, iteration = 400.  The vertex log (and,
 * for which = 0, the front's coordinates) hold the result; the candidate list of the finished episode is not rebuilt -- the
 * next call on such an env is a reset.  sweeps_dev / diff_dev as meshenv_smooth, plus MESHENV_SMOOTH_NOT_FINISHED (front
 * > 5, nothing archived, archived episode truncated) and MESHENV_SMOOTH_INDEX_ERROR (env untouched). */
int meshenv_smooth_final(MeshEnv *h, int which, const uint8_t *mask_dev, int iteration, double lr_1, double lr_2,
                         int32_t *sweeps_dev, double *diff_dev);

/* Host-side readout of one env's not_valid_points (synchronises the stream): xy_host[2*cap_points], *count = length. */
int meshenv_get_not_valid(MeshEnv *h, int env, double *xy_host, int cap_points, int32_t *count);

/* The same list as vertex ids (the reference's list holds Vertex objects: identity), and the summary of
 * last_not_valid_points (rl/boundary_env.py:48,416-422: set where move() smooths, compared by first entry, last entry and
 * length, never cleared by reset()): last_host[4] = first id, last id, length, 1 if it was recorded in the running
 * episode (reset() deep-copies the domain, rl/boundary_env.py:69: vertices of an earlier episode are different objects).  ids_host / last_host nullable. */
int meshenv_get_not_valid_ids(MeshEnv *h, int env, int32_t *ids_host, int cap_ids, int32_t *count, int32_t *last_host);

/*
 * Multi-GPU exchange message.  With msg_dev != NULL every following meshenv_step / meshenv_rollout also writes
 * msg_dev[n_envs*21] float32 = (obs[18] | reward | done | complete) per env -- the buffer a rank hands to
 * all_gather -- straight from the step kernel (no separate pack kernels).  NULL switches it off.  The pointer
 * may be changed between steps (double buffering against an in-flight collective).
 */
#define MESHENV_MSG_DIM 21
int meshenv_set_packed_output(MeshEnv *h, float *msg_dev);

/* Per-env status bits (MESHENV_ST_*) after the last step/reset; status_dev[n_envs]. */
int meshenv_get_status(MeshEnv *h, uint8_t *status_dev);

/*
 * Host-side readout of one environment (synchronises the stream).  Any pointer may be NULL.
 *   ring_ids_host[max_ring]      global vertex ids of updated_boundary.vertices, in ring order
 *   ring_xy_host[2*max_ring]
 *   cand_key_host[max_ring]      cached candidate key per ring slot (NaN where not a candidate)
 *   cand_stamp_host[max_ring]    insertion stamp per ring slot (larger = nearer the list head
 *                                among equal keys; INT32_MIN where not a candidate)
 *   scalars_host[8]: ring length, reference ring index, n_elements (len(generated_meshes)),
 *                    failed_num, n_vertices (len(boundary.vertices)), status bits, domain, n0
 *   fscalars_host[2]: current_area, base_length
 */
int meshenv_get_state(MeshEnv *h, int env, int32_t *ring_ids_host, double *ring_xy_host, double *cand_key_host,
                      int32_t *cand_stamp_host, int32_t *scalars_host, double *fscalars_host);

/*
 * generated_meshes / boundary.vertices of one env (rl/boundary_env.py:192, general/mesh.py:589-590):
 *   quads_host[4*cap]      global vertex ids per element, in creation order
 *   vertex_xy_host[2*cap]  coordinates of all vertices ever (initial ring first, then new ones)
 * cap_elems / cap_verts are the capacities of the caller's buffers; *n_elem / *n_vert receive the
 * number of entries written.
 */
int meshenv_get_elements(MeshEnv *h, int env, int32_t *quads_host, int cap_elems, double *vertex_xy_host,
                         int cap_verts, int32_t *n_elem, int32_t *n_vert);

/*
 * The same for the last FINISHED episode of the env.  The reference's evaluation callback reads
 * env.generated_meshes after `done` and before it resets (rl/baselines/CustomizeCallback.py:131-133); under
 * auto-reset the kernel has already started the next episode by then, so every reset that ends an episode with at
 * least one element archives that episode's log (double-buffered in HBM, no copy).  *flags: bit 0 = is_complete,
 * bit 1 = the log overflowed log_capacity; *episodes: number of episodes archived so far (0 = nothing yet, n_elem 0).
 */
int meshenv_get_last_episode(MeshEnv *h, int env, int32_t *quads_host, int cap_elems, double *vertex_xy_host,
                             int cap_verts, int32_t *n_elem, int32_t *n_vert, int32_t *flags, int32_t *episodes);

/*
 * Per-element quality report, computed on the device for every env at once (one launch).
 *   which      0 = the running episodes, 1 = the archived (last finished) episodes
 *   elem_dev   [n_envs][log_capacity][MESHENV_QUALITY_DIM] float64, nullable: per element
 *                min corner angle (deg), max corner angle (deg), scaled Jacobian, stretch, taper, 'robust',
 *                area, 'default' -- Mesh.get_quality(type) / compute_area() of general/components.py:863-950, the
 *                in-repo forms of the five Verdict measures Measurement/quality_verdict.py:133-148 requests;
 *                rows >= count are left untouched
 *   stats_dev  [n_envs][MESHENV_QUALITY_DIM][4] float64, nullable: minimum, average, maximum, variance per
 *                measure over the env's elements (what DumpQualityStats prints, quality_verdict.py:77-90)
 *   count_dev  [n_envs] int32, nullable: number of elements reported per env
 * Stream-ordered on the handle's stream.
 */
#define MESHENV_QUALITY_DIM 8
int meshenv_element_quality(MeshEnv *h, int which, double *elem_dev, double *stats_dev, int32_t *count_dev);

/*
 * MeshGeneration.get_quality(element, index) (general/mesh.py:1728-1747; called as env.get_quality(env.generated_meshes[i], 4)
 * by rl/baselines/testbed.py:194-197, and by generate_meshes_canvas, general/mesh.py:1770-1778, for the labels of
 * save_meshes) for n arbitrary quads, on the device:
 *   quad_xy_dev [n][4][2] float64, vertices in Mesh.vertices order; out_dev [n] float64
 *   index 0 = Mesh.get_quality() 'default', 1 = compute_element_quality (general/mesh.py:1714-1726), 3 = 'stretch',
 *         4 = 'robust', 5 = 'strong' (general/components.py:863-930).
 * Indices 2 and 6 add compute_ele_boundary_quality of the ring right after the extraction; that value exists only
 * inside the step that extracted the element (it is the step's reward term) -> MESHENV_E_ARG.
 * Stream-ordered on the handle's stream.
 */
int meshenv_quad_quality(MeshEnv *h, int n, const double *quad_xy_dev, int index, double *out_dev);

/*
 * Work counters since creation (roofline accounting), summed over envs:
 *   out_host[0] env steps executed, [1] valid extractions, [2] sum of ring lengths over all steps,
 *   [3] sum of ring lengths over valid steps.
 */
int meshenv_counters(MeshEnv *h, uint64_t *out_host);

/*
 * Kernel timing with HIP events on the handle's stream (bench.py's roofline figure).  meshenv_set_timing(h, k),
 * k > 0: every other group of k consecutive meshenv_step / meshenv_rollout launches is bracketed by one event pair
 * and reported as (elapsed / k), the average launch duration inside the group including the launch-to-launch gap
 * (an event pair costs several microseconds of stream time on this stack, so bracketing single ~20 us launches would
 * both slow the loop and inflate the figure).  k = 0 switches timing off.  Arming creates a pool of
 * MESHENV_TIMING_POOL event pairs and clears the record; meshenv_kernel_times() synchronises and copies the
 * per-launch averages (milliseconds, in launch order) of the groups recorded since then -- at most the newest
 * MESHENV_TIMING_POOL -- into ms_host[cap] and clears the record.  Call it before changing k.
 */
#define MESHENV_TIMING_POOL 4096
int meshenv_set_timing(MeshEnv *h, int enable);
int meshenv_kernel_times(MeshEnv *h, float *ms_host, int cap, int32_t *n_out);

/*
 * Fused SAC actor forward -- the caller of the hot path, not part of the environment.
 * Architecture fixed to the reference's policy (rl/baselines/RL_Mesh.py:183-196: MlpPolicy, ReLU,
 * net_arch [128, 128, 128]; SB3's squashed-Gaussian actor): latent = MLP(obs[18]); mean / log_std = Linear(latent);
 * action = low + 0.5 * (tanh(mean + exp(clamp(log_std, -20, 2)) * noise) + 1) * (high - low); noise_dev = NULL gives
 * the deterministic action.  One launch instead of ~25, so obs -> action -> step stays on the GPU.
 * Weights: host pointers in torch.nn.Linear layout ([out][in], row-major), float32.
 */
typedef struct MeshActor MeshActor;
int meshenv_actor_create(int device, void *stream, MeshActor **out);
void meshenv_actor_destroy(MeshActor *a);
int meshenv_actor_set_stream(MeshActor *a, void *stream);
int meshenv_actor_load(MeshActor *a, const float *w1, const float *b1, const float *w2, const float *b2, const float *w3,
                       const float *b3, const float *w_mu, const float *b_mu, const float *w_log_std,
                       const float *b_log_std, const float *low, const float *high);
int meshenv_actor_forward(MeshActor *a, int n, const float *obs_dev, const float *noise_dev, float *actions_dev);
/*
 * The stochastic action with the noise drawn inside the kernel: eps[env][k] is a standard normal from Philox4x32-10
 * keyed by `seed` with counter (env, `counter`) and Box-Muller -- the caller passes a fresh `counter` per rollout step
 * (same seed + counter -> same actions).  eps_out_dev [n,3] (nullable) receives the noise that was used, so that
 * meshenv_actor_forward(obs, eps_out) reproduces the actions bit for bit.  Saves the separate random-number launch.
 */
int meshenv_actor_sample(MeshActor *a, int n, const float *obs_dev, uint64_t seed, uint64_t counter, float *actions_dev,
                         float *eps_out_dev);

/* One launch per vector step of the closed RL loop: meshenv_step(actions_dev, ...) followed by meshenv_actor_sample /
 * meshenv_actor_forward on the observations it produced -- i.e. obs_dev, reward_dev, done_dev, complete_dev,
 * terminal_obs_dev exactly as meshenv_step writes them, and actions_next_dev [n_envs][3] = the policy's actions for the
 * NEXT step (sample != 0: SAC's stochastic actor with in-kernel Philox noise keyed by (seed, counter), eps_out_dev nullable;
 * sample == 0: the mean action).  actions_next_dev must not alias actions_dev (ping-pong two buffers).  When the batch runs
 * on the CU-group kernel (256 * 16 envs, default parameters) both halves run
 * in ONE kernel (csrc/meshenv_fused.h: the same 16 envs per workgroup, the actor's forward after the step's barrier);
 * otherwise two launches are issued.  Results are identical either way.  Env and actor must share device and stream
 * (MESHENV_E_STATE otherwise: the stream is what orders the two halves). */
int meshenv_step_actor(MeshEnv *h, MeshActor *a, const float *actions_dev, float *obs_dev, double *reward_dev, uint8_t *done_dev,
                       uint8_t *complete_dev, float *terminal_obs_dev, int auto_reset, int sample, uint64_t seed, uint64_t counter,
                       float *actions_next_dev, float *eps_out_dev);

/*
 * Fused PPO / A2C / TD3 / DDPG policies (csrc/meshenv_policy.h) -- the rollout side of the reference's other algorithms
 * (rl/baselines/RL_Mesh.py:113-228), not part of the environment.  One MLP of two hidden layers on obs[18]:
 *   kind 0 (actor-critic, SB3 ActorCriticPolicy: PPO, A2C): pi tower -> action_net = mean, vf tower -> value_net = value;
 *          std = exp(log_std) (a state-independent [3] parameter), buffer_action = mean + std * eps,
 *          action = clamp(buffer_action, low, high), log_prob = sum over the 3 components of Normal(mean, std).log_prob
 *   kind 1 (deterministic, SB3 TD3Policy: actor.mu): scaled = tanh(mu(latent)); with noise
 *          scaled = clamp(scaled + sigma * eps, -1, 1); buffer_action = scaled, action = low + 0.5 (scaled + 1) (high - low)
 * hidden 64, 128 or 256 (both layers), activation 0 ReLU or 1 Tanh; any other shape fails with MESHENV_E_ARG and a message
 * naming the supported ones.  Weights: host pointers, torch.nn.Linear layout ([out][in], row-major), float32: the pi (or
 * actor) tower's two layers, its head (action_net [3][hidden] or mu [3][hidden]), the vf tower's two layers and value_net
 * [1][hidden] (NULL for kind 1), log_std (kind 0) or sigma (kind 1, nullable: no action noise), low and high [3].
 */
typedef struct MeshPolicy MeshPolicy;
int meshenv_policy_create(int device, void *stream, MeshPolicy **out);
void meshenv_policy_destroy(MeshPolicy *p);
int meshenv_policy_set_stream(MeshPolicy *p, void *stream);
const char *meshenv_policy_last_error(const MeshPolicy *p);   /* message of the handle's last failure */
int meshenv_policy_load(MeshPolicy *p, int kind, int hidden, int activation, const float *pi_w1, const float *pi_b1,
                        const float *pi_w2, const float *pi_b2, const float *head_w, const float *head_b, const float *vf_w1,
                        const float *vf_b1, const float *vf_w2, const float *vf_b2, const float *value_w, const float *value_b,
                        const float *log_std_or_sigma, const float *low, const float *high);
/*
 * One launch.  eps: noise_dev [n][3] (explicit N(0,1) draws), or sample != 0 (Philox4x32-10 keyed by seed, counter
 * (env, counter) -- the same stream as the SAC actor's sample entry point), or neither (eps = 0: the deterministic action).
 * Outputs, each nullable: actions_dev / buffer_actions_dev / eps_out_dev [n][3], log_prob_dev / value_dev [n] (kind 0 only:
 * kind 1 fails with MESHENV_E_ARG when they are given).  value_dev alone is the value-only mode: the vf tower by itself.
 * eps_out_dev fed back as noise_dev reproduces the outputs bit for bit.
 */
int meshenv_policy_forward(MeshPolicy *p, int n, const float *obs_dev, const float *noise_dev, int sample, uint64_t seed,
                           uint64_t counter, float *actions_dev, float *buffer_actions_dev, float *log_prob_dev, float *value_dev,
                           float *eps_out_dev);
/*
 * T vector steps of the closed loop in one call, no host synchronisation: for t < T the policy on obs_t (noise counter
 * counter + t when sample != 0, eps = 0 otherwise) and a step of every env on its actions; then the values of obs_T.
 *   obs_dev [T+1][n][18]: slice 0 = the current observation (input); slice t + 1 = the observation after step t
 *   actions_dev, buffer_actions_dev (nullable), eps_dev (nullable) [T][n][3]; log_prob_dev, value_dev [T][n] (nullable)
 *   reward_dev [T][n] float64, done_dev, complete_dev [T][n] uint8, terminal_obs_dev [T][n][18] (nullable): as the
 *       single step writes them
 *   terminal_value_dev [T][n] (nullable, needs terminal_obs_dev): V(terminal obs of step t) where done && !complete, else
 *       0 -- the bootstrap value of a truncated episode
 *   last_value_dev [n] (nullable): V(obs_T)
 * log_prob / value / terminal_value / last_value must be NULL for kind 1.  Bit-identical to T pairs of policy forward + step
 * on the same slices.  Env and policy must share device and stream (MESHENV_E_STATE otherwise).
 */
int meshenv_step_policy_multi(MeshEnv *h, MeshPolicy *p, int T, float *obs_dev, int sample, uint64_t seed, uint64_t counter,
                              float *actions_dev, float *buffer_actions_dev, float *log_prob_dev, float *value_dev, float *eps_dev,
                              double *reward_dev, uint8_t *done_dev, uint8_t *complete_dev, float *terminal_obs_dev,
                              float *terminal_value_dev, float *last_value_dev, int auto_reset);

/*
 * Generalised advantage estimation over T rows of rollout histories (csrc/meshenv_gae.h): SB3's
 * RolloutBuffer.compute_returns_and_advantage (GAE, SB3 2.x) with collect_rollouts' TimeLimit.truncated bootstrap
 * (rewards += gamma * V(terminal obs)) in front -- what examples/ppo_rollout.py::gae does in torch, bit-identical to that
 * float32 loop (g = (float)gamma, gl = (float)(gamma * gae_lambda), no fused multiply-add, denormals kept):
 *   r = (float)reward[t] (+ g * terminal_value[t] where terminal_value_dev is given), nnt = 1 - (done[t] != 0),
 *   delta = (r + (g * next_value) * nnt) - value[t] with next_value = value[t + 1], or last_value at t = T - 1,
 *   last = delta + (gl * nnt) * last, from t = T - 1 down to 0 with last = 0 after T - 1.
 * Every history is [T][n_envs] row-major, as meshenv_step_policy_multi writes it: reward_dev float64, value_dev float32,
 * done_dev uint8, terminal_value_dev float32 (nullable), last_value_dev [n_envs].  Outputs: advantage_dev = last,
 * return_dev = last + value[t] and buffer_reward_dev = r (the bootstrapped float32 reward the buffer stores; both nullable),
 * none of which may overlap an input or each other.  One launch on the handle's stream, no host synchronisation.
 * MESHENV_E_ARG for T < 1, a NULL required pointer, overlapping outputs, or a gamma / gae_lambda outside [0, 1] (NaN included).
 */
int meshenv_gae(MeshEnv *h, int T, const double *reward_dev, const float *value_dev, const uint8_t *done_dev,
                const float *terminal_value_dev, const float *last_value_dev, double gamma, double gae_lambda,
                float *advantage_dev, float *return_dev, float *buffer_reward_dev);

/*
 * The replay buffer of the off-policy algorithms (SAC, TD3) on the device (csrc/meshenv_replay.h).  Storage is one
 * caller-owned, 16-byte aligned float32 DEVICE array store_dev [rows][n_envs][R], R = meshenv_replay_record_floats(), one
 * packed record per transition: observation 0..17 | next observation 18..35 | action 36..38 | reward 39 | done 40 |
 * timeout 41 | zero padding.  pos / full are the caller's (SB3: ReplayBuffer.pos, .full); the calls are stateless, one
 * launch each on the handle's stream, no host synchronisation.
 */
int meshenv_replay_record_floats(void);
/*
 * T vector steps into rows (pos + t) % rows: SB3 2.x's OffPolicyAlgorithm._store_transition + ReplayBuffer.add, T times:
 *   observation      = obs0 at t = 0, obs_after[t - 1] beyond (what step t acted on)
 *   next observation = terminal_obs[t] where done[t], else obs_after[t]
 *   action           = actions[t], or 2.0f * ((a - low) / (high - low)) - 1.0f in float32 (SAC's policy.scale_action) when
 *                      action_low_high_host, a HOST array low[3], high[3], is given
 *   reward = (float)reward[t], done = done[t] != 0, timeout = handle_timeouts && done && !complete (TimeLimit.truncated)
 * obs0_dev [n][18]; obs_after_dev, terminal_obs_dev [T][n][18]; actions_dev [T][n][3]; reward_dev [T][n] float64; done_dev,
 * complete_dev [T][n] uint8 -- as meshenv_step_policy_multi (obs0 = obs slice 0, obs_after = slices 1..T) and
 * meshenv_step_actor_multi (obs_after = obs, obs0 = the observation before the call) leave them.  With T > rows only the
 * last rows steps are written, which is what T sequential adds leave.  The caller advances pos by T modulo rows.
 * MESHENV_E_ARG for T < 1, rows < 1, pos outside [0, rows), a NULL pointer other than action_low_high_host, a misaligned
 * store, or an input that overlaps the store.
 */
int meshenv_replay_add(MeshEnv *h, int T, const float *obs0_dev, const float *obs_after_dev, const float *terminal_obs_dev,
                       const float *actions_dev, const double *reward_dev, const uint8_t *done_dev, const uint8_t *complete_dev,
                       const float *action_low_high_host, int handle_timeouts, float *store_dev, int rows, int pos);
/*
 * batch transitions out of the store: SB3 2.x's ReplayBuffer.sample + _get_samples (optimize_memory_usage=False, no
 * VecNormalize), the ReplayBufferSamples fields as contiguous float32 arrays obs_out [batch][18], actions_out [batch][3],
 * next_obs_out [batch][18], dones_out [batch][1] = done * (1 - timeout), rewards_out [batch][1].  With rows_in_dev /
 * envs_in_dev (int32 [batch], both or neither) it is _get_samples on those indices; one outside [0, rows) x [0, n_envs) is
 * not read: its outputs are NaN and its rows_out -1.  Without them sample i draws row in [0, size) and env in [0, n_envs) from
 * Philox4x32-10 keyed by seed at counter words (i, counter, tag 1) by multiply-high (csrc/meshenv_replay.h; SB3 draws
 * from numpy's global stream instead).  size = ReplayBuffer.size().  rows_out_dev / envs_out_dev (nullable) receive the
 * indices used.  MESHENV_E_ARG for batch < 1, rows < 1, size outside [1, rows], a NULL store or output, only one of
 * rows_in / envs_in, a misaligned store, or outputs that overlap the store, the given indices or each other.
 */
int meshenv_replay_sample(MeshEnv *h, const float *store_dev, int rows, int size, int batch, uint64_t seed, uint64_t counter,
                          const int32_t *rows_in_dev, const int32_t *envs_in_dev, float *obs_out_dev, float *actions_out_dev,
                          float *next_obs_out_dev, float *dones_out_dev, float *rewards_out_dev, int32_t *rows_out_dev,
                          int32_t *envs_out_dev);

/*
 * The TD target of SAC / TD3 on the device (csrc/meshenv_target.h): the `with th.no_grad():` block of SB3 2.x's SAC.train /
 * TD3.train that follows replay_buffer.sample, one launch, from the tensors meshenv_replay_sample returns.
 *   kind 0, SAC (actor ReLU [128, 128, 128] with mu / log_std heads, twin critics ReLU [128, 128, 128], 21 -> 1):
 *     next_actions, next_log_prob = actor.action_log_prob(next_observations)        (log_std clamped to [-20, 2],
 *         a = tanh(mean + exp(log_std) * eps), SquashedDiagGaussianDistribution.log_prob with epsilon 1e-6)
 *     next_q_values = min(cat(critic_target(next_observations, next_actions), dim=1), dim=1)
 *     next_q_values = next_q_values - ent_coef * next_log_prob.reshape(-1, 1)
 *   kind 1, TD3 (actor_target ReLU [256, 256] + tanh, twin critics ReLU [256, 256]):
 *     noise = actions.clone().normal_(0, target_policy_noise).clamp(-target_noise_clip, target_noise_clip)
 *     next_actions = (actor_target(next_observations) + noise).clamp(-1, 1)
 *     next_q_values = min(cat(critic_target(next_observations, next_actions), dim=1), dim=1)
 *   kind 2, DDPG (csrc/meshenv_wide.h; the reference's DDPG('MlpPolicy', env), rl/baselines/RL_Mesh.py:113-228: SB3's TD3.train
 *     with n_critics = 1, actor_target ReLU [400, 300] + tanh, ONE critic ReLU [400, 300]): the statements of kind 1 with
 *     next_q_values = critic_target(next_observations, next_actions)[0]; SB3's DDPG passes target_policy_noise = 0.1 and
 *     target_noise_clip = 0.0, which makes the noise term +-0 -- the formula is evaluated as written
 *   all: target_q_values = rewards + (1 - dones) * gamma * next_q_values          (float32, in that order)
 * Any other kind fails with MESHENV_E_ARG and a message naming the supported ones.  gamma in [0, 1]; ent_coef is SB3's fixed
 * coefficient, used when meshenv_target_bind gets no log_ent_coef; policy_noise, noise_clip >= 0 (TD3).
 */
typedef struct MeshTarget MeshTarget;
int meshenv_target_create(int device, void *stream, int kind, float gamma, float ent_coef, float policy_noise, float noise_clip,
                          MeshTarget **out);
void meshenv_target_destroy(MeshTarget *t);
int meshenv_target_set_stream(MeshTarget *t, void *stream);
const char *meshenv_target_last_error(const MeshTarget *t);   /* message of the handle's last failure */
/*
 * Records the DEVICE pointers of the live float32, contiguous torch.nn.Linear parameters ([out][in] weight, [out] bias; the
 * caller checks dtype, layout and device).  Nothing is read yet.
 *   actor_dev  kind 0: w1 b1 w2 b2 w3 b3 mu_w mu_b log_std_w log_std_b (n_actor 10); kind 1: w1 b1 w2 b2 mu_w mu_b (6)
 *   q1_dev, q2_dev  critic_target.q_networks[0], [1]: kind 0: w1 b1 w2 b2 w3 b3 w4 b4 (n_critic 8); kind 1: 6; w1 is [H][21]
 *   kind 2: actor_dev w1 b1 w2 b2 mu_w mu_b (n_actor 6; w1 [400][18], w2 [300][400], mu_w [3][300]), q1_dev likewise
 *       (n_critic 6; w1 [400][21], w4 [1][300]) and q2_dev = NULL (a q2_dev fails with MESHENV_E_ARG)
 *   log_ent_coef_dev  kind 0: SAC's learned log_ent_coef [1] (ent_coef = exp of it: th.exp(self.log_ent_coef.detach())) or NULL
 * SB3's optimisers and polyak_update write in place, so the pointers stay valid; bind again after anything that reallocates.
 * MESHENV_E_ARG for a wrong count, a NULL entry, or log_ent_coef_dev with kind 1 or 2.
 */
int meshenv_target_bind(MeshTarget *t, const float *const *actor_dev, int n_actor, const float *const *q1_dev,
                        const float *const *q2_dev, int n_critic, const float *log_ent_coef_dev);
/* Copies every bound tensor (log_ent_coef included) into the kernel's layout: ONE launch on the handle's stream, no host
 * copy, no synchronisation.  A forward sees the values of the last refresh before it on the stream -- call it after
 * optimizer.step() / polyak_update.  MESHENV_E_STATE before meshenv_target_bind. */
int meshenv_target_refresh(MeshTarget *t);
/*
 * One launch.  next_obs_dev [n][18], rewards_dev, dones_dev [n] (= ReplayBufferSamples' [n][1]; dones is dones * (1 -
 * timeouts) already).  eps: noise_dev [n][3], or sample != 0 for Philox4x32-10 keyed by seed at counter words (sample
 * index, counter lo, counter hi, 2) -- tag 2 is this call's own (rollout noise 0, replay draw 1) -- or neither for eps = 0.
 * Outputs, each nullable and written only when given: target_dev [n] (needs rewards and dones), next_actions_dev [n][3] (in
 * [-1, 1], what the critics see), next_log_prob_dev [n] (kind 0), q1_dev, q2_dev [n], eps_out_dev [n][3] (needs noise).
 * MESHENV_E_STATE before the first refresh; MESHENV_E_ARG for n < 1, a missing input, noise and sample together,
 * next_log_prob_dev with kind 1 or 2, q2_dev with kind 2, eps_out_dev without noise, or no output.
 */
int meshenv_target_forward(MeshTarget *t, int n, const float *next_obs_dev, const float *rewards_dev, const float *dones_dev,
                           const float *noise_dev, int sample, uint64_t seed, uint64_t counter, float *target_dev,
                           float *next_actions_dev, float *next_log_prob_dev, float *q1_dev, float *q2_dev, float *eps_out_dev);

/*
 * The critic loss of SAC / TD3 and its gradients on the device (csrc/meshenv_critic_grad.h): the statements of SB3 2.x's
 * SAC.train / TD3.train that follow the TD target,
 *     current_q_values = self.critic(replay_data.observations, replay_data.actions)
 *     critic_loss = 0.5 * sum(F.mse_loss(current_q, target_q_values) for current_q in current_q_values)
 *     self.critic.optimizer.zero_grad(); critic_loss.backward()
 * for the twin critics of meshenv_target_create's kinds (kind 0: ReLU [128, 128, 128]; kind 1: ReLU [256, 256]; input
 * cat(obs, action) = 21, float32).  The optimiser step stays the caller's.  Any other kind fails with MESHENV_E_ARG.
 */
typedef struct MeshCriticGrad MeshCriticGrad;
int meshenv_critic_grad_create(int device, void *stream, int kind, MeshCriticGrad **out);
void meshenv_critic_grad_destroy(MeshCriticGrad *g);
int meshenv_critic_grad_set_stream(MeshCriticGrad *g, void *stream);
const char *meshenv_critic_grad_last_error(const MeshCriticGrad *g);   /* message of the handle's last failure */
/*
 * Records the DEVICE pointers of the LIVE critics' float32, contiguous torch.nn.Linear parameters (self.critic.q_networks,
 * not critic_target; per critic w1 b1 w2 b2 [w3 b3] out_w out_b: n_critic 8 for kind 0, 6 for kind 1; [H][H] weights
 * 16-byte aligned) and of the caller's flat gradient buffer grad_dev [n_grad]: per critic, in the same order and in
 * torch's [out][in] / [out] layout, w1 [H][21], b1 [H], w_l [H][H], b_l [H], out_w [H], out_b [1], each critic padded to a
 * multiple of 64 floats (n_grad = 2 * 36032 for kind 0, 2 * 71744 for kind 1).  The parameters are read at every backward
 * as they are then (optimisers write in place); bind again after anything that reallocates.  Allocates the handle's
 * workspace of 128 partial gradient sets (n_grad + 64 floats each) on the first call.
 */
int meshenv_critic_grad_bind(MeshCriticGrad *g, const float *const *q1_dev, const float *const *q2_dev, int n_critic,
                             float *grad_dev, int64_t n_grad);
/*
 * Two launches on the handle's stream, no host copy, no synchronisation.  obs_dev [n][18], actions_dev [n][3], target_dev
 * [n] (target_q_values: a constant, no gradient flows into it).  OVERWRITES grad_dev with the gradients of critic_loss and
 * writes critic_loss to loss_dev [1].  Optional: q1_dev, q2_dev [n] (current_q_values), acts1_dev / acts2_dev (both or
 * neither): per hidden layer a [n][H] buffer receiving that critic's post-ReLU activations (a > 0 is the mask the backward
 * pass used).  Deterministic: the sum over the batch has a fixed order, the same inputs give the same bits.
 * MESHENV_E_STATE before meshenv_critic_grad_bind; MESHENV_E_ARG for n < 1 or a missing input.
 */
int meshenv_critic_grad_backward(MeshCriticGrad *g, int n, const float *obs_dev, const float *actions_dev, const float *target_dev,
                                 float *loss_dev, float *q1_dev, float *q2_dev, float *const *acts1_dev, float *const *acts2_dev);

/*
 * The actor loss and the entropy-coefficient loss of SAC and their gradients on the device (csrc/meshenv_actor_grad.h): the
 * statements of SB3 2.x's SAC.train that follow the critic update,
 *     actions_pi, log_prob = self.actor.action_log_prob(replay_data.observations)
 *     ent_coef = th.exp(self.log_ent_coef.detach())
 *     ent_coef_loss = -(self.log_ent_coef * (log_prob + self.target_entropy).detach()).mean()
 *     q_values_pi = th.cat(self.critic(replay_data.observations, actions_pi), dim=1)
 *     min_qf_pi, _ = th.min(q_values_pi, dim=1, keepdim=True)
 *     actor_loss = (ent_coef * log_prob - min_qf_pi).mean()
 *     self.actor.optimizer.zero_grad(); actor_loss.backward()
 * for the recipe the reference runs (rl/baselines/RL_Mesh.py:179-205: SAC('MlpPolicy', batch_size=100), actor ReLU
 * [128, 128, 128] with mu / log_std heads, twin critics ReLU [128, 128, 128], float32).  SAC only; the optimiser steps stay
 * the caller's.  ent_coef: SB3's fixed coefficient, used when meshenv_actor_grad_bind gets no log_ent_coef; target_entropy:
 * self.target_entropy (-3 for the 3 actions).  MESHENV_E_ARG when either is not finite.
 */
typedef struct MeshActorGrad MeshActorGrad;
int meshenv_actor_grad_create(int device, void *stream, float ent_coef, float target_entropy, MeshActorGrad **out);
void meshenv_actor_grad_destroy(MeshActorGrad *g);
int meshenv_actor_grad_set_stream(MeshActorGrad *g, void *stream);
const char *meshenv_actor_grad_last_error(const MeshActorGrad *g);   /* message of the handle's last failure */
/*
 * Records the DEVICE pointers of the LIVE float32, contiguous torch.nn.Linear parameters (the caller checks dtype, layout
 * and device).  Nothing is read yet.
 *   actor_dev   self.actor: w1 b1 w2 b2 w3 b3 mu_w mu_b log_std_w log_std_b (n_actor 10)
 *   q1_dev, q2_dev   self.critic.q_networks[0], [1] (not critic_target): w1 b1 w2 b2 w3 b3 w4 b4 (n_critic 8); read only
 *   log_ent_coef_dev   self.log_ent_coef [1] (ent_coef = th.exp(self.log_ent_coef.detach()), taken at every backward), or NULL
 *   grad_dev [n_grad]   the caller's flat gradient buffer, n_grad = 36288: the actor's gradients in the order of actor_dev
 *       and in torch's [out][in] / [out] layout (w1 [128][18] first), then log_ent_coef.grad at float 36230, then padding
 * [128][128] and [3][128] weights 16-byte aligned.  Optimisers write in place, so the pointers stay valid; bind again after
 * anything that reallocates.  Allocates the handle's workspace of 128 partial gradient sets on the first call.
 */
int meshenv_actor_grad_bind(MeshActorGrad *g, const float *const *actor_dev, int n_actor, const float *const *q1_dev,
                            const float *const *q2_dev, int n_critic, const float *log_ent_coef_dev, float *grad_dev, int64_t n_grad);
/*
 * actor_loss.backward() and the ent_coef statements: two launches on the handle's stream, no host copy, no
 * synchronisation.  obs_dev [n][18] (replay_data.observations).  eps of actions_pi: noise_dev [n][3], or sample != 0 for
 * Philox4x32-10 keyed by seed at counter words (sample index, counter lo, counter hi, 3) -- tag 3 is this call's own
 * (rollout noise 0, replay draw 1, TD target 2) -- or neither for eps = 0.  OVERWRITES the actor's part of grad_dev with
 * the gradients of actor_loss and, with a bound log_ent_coef, float 36230 with that of ent_coef_loss; the critics'
 * parameters are read and receive nothing.  losses_dev [2]: actor_loss, ent_coef_loss (the second is written only with a
 * bound log_ent_coef).  eps_out_dev [n][3] (nullable, needs noise or sample) receives the eps used.  Optional, all of an
 * array or NULL: parts_dev[7] = actions_pi [n][3], log_prob [n], q1_pi [n], q2_pi
 * [n], dq_da [n][3] (the selected critic's dQ/da; q1 <= q2 selects critic 1), d_mu [n][3], d_log_std [n][3] (the head
 * gradients); acts_dev[9] = per network (actor, critic 1, critic 2) and hidden layer a [n][128] buffer receiving the
 * post-ReLU activations (a > 0 is the mask the backward pass used).  Deterministic: the sums over the batch have a fixed
 * order, the same inputs give the same bits.
 * MESHENV_E_STATE before meshenv_actor_grad_bind; MESHENV_E_ARG for n < 1 or a missing input, noise_dev with sample, or
 * eps_out_dev without either.
 */
int meshenv_actor_grad_backward(MeshActorGrad *g, int n, const float *obs_dev, const float *noise_dev, int sample, uint64_t seed,
                                uint64_t counter, float *losses_dev, float *eps_out_dev, float *const *parts_dev, float *const *acts_dev);

/*
 * Policy evaluation on the device (csrc/meshenv_eval.h): SB3 2.x's evaluate_policy loop (non-Monitor branch) -- the loop
 * the reference's evaluation callers run with a deterministic model.predict:
 *   rl/baselines/CustomizeCallback.py:27-141   every 1000 training steps, to pick best_model
 *   rl/baselines/testbed.py:150-212            per domain: is_complete, len(generated_meshes), get_quality(e, 4)
 *   v2/src/mesh_rl/evaluation/eval_loop.py:80-103   {"completed": [...], "n_elements": [...]}
 * plus the quality report of every finished mesh, taken while it is still archived (meshenv_get_last_episode: one
 * archived episode per env, replaced when the env's next episode ends).
 *
 * MeshEvalBuffers: caller-owned DEVICE memory.  Per env [n_envs]: target (episodes to record, >= 0, unchanged during an
 * evaluation), offset (first record slot: the exclusive prefix sum of target), and the accumulators count, length, seen,
 * return, return_raw; short_dev [1] = envs with count < target.  Per episode [sum of target], slot offset[env] + k holding
 * the env's k-th recorded episode:
 *   ep_env, ep_domain, ep_step (0-based vector step at which the episode ended), ep_length,
 *   ep_return      float64 sum of (double)(float)reward: SB3's value (SB3MeshVecEnv hands float32 rewards to
 *                  evaluate_policy, which adds them into np.zeros(n_envs))
 *   ep_return_raw  float64 sum of the float64 rewards
 *   ep_flags       bit 0 is_complete, bit 1 the element log overflowed log_capacity
 *   ep_n_elements  len(generated_meshes); 0 for an episode that ended without an element (reset_from_domain does not
 *                  archive it: the archive still holds an older episode, which is not scored); -1 with log_capacity = 0
 *   ep_archive     nullable: meshenv_get_last_episode's `episodes` value of the archived mesh (0: none), so that a caller
 *                  can tell whether the archive still holds that episode
 *   ep_quality     nullable [.][MESHENV_QUALITY_DIM][4]: meshenv_element_quality(which = 1) statistics of the finished mesh,
 *                  bit for bit as that call would return them right after the step (zeros where n_elements is 0); needs
 *                  log_capacity > 0 (MESHENV_E_STATE)
 * obs_dev [n][18], reward_dev [n], done_dev, complete_dev [n] (nullable, all or none): meshenv_evaluate's step buffers --
 * NULL uses buffers of the handle (allocated by the first call).  Envs past their target keep stepping and are not
 * recorded, as in SB3.
 */
typedef struct MeshEvalBuffers {
    int32_t struct_size;  /* sizeof(MeshEvalBuffers), for ABI checking */
    int32_t reserved;
    const int32_t *target_dev, *offset_dev;
    int32_t *count_dev, *length_dev, *seen_dev;
    double *return_dev, *return_raw_dev;
    int32_t *short_dev;
    int32_t *ep_env_dev, *ep_domain_dev, *ep_step_dev, *ep_length_dev, *ep_flags_dev, *ep_n_elements_dev, *ep_archive_dev;
    double *ep_return_dev, *ep_return_raw_dev, *ep_quality_dev;
    float *obs_dev;
    double *reward_dev;
    uint8_t *done_dev, *complete_dev;
} MeshEvalBuffers;

/* Start of an evaluation, one launch: count / length / return accumulators cleared, seen = the archive counter of every
 * env, short = envs with target > 0.  Call after the reset that starts the episodes (meshenv_evaluate does both). */
int meshenv_eval_begin(MeshEnv *h, const MeshEvalBuffers *bufs);

/* One launch after a vector step (meshenv_step, meshenv_step_actor, a step of meshenv_step_policy_multi -- any call whose
 * reward / done / complete of that step are passed here): adds the rewards, records the episodes that ended (slot
 * offset + count while count < target), scores their finished meshes when ep_quality_dev is given, and decrements
 * short_dev when an env reaches its target.  `step` is stored as ep_step.  Stream-ordered, no host synchronisation. */
int meshenv_eval_tally(MeshEnv *h, const MeshEvalBuffers *bufs, int step, const double *reward_dev, const uint8_t *done_dev,
                       const uint8_t *complete_dev);

/*
 * The whole loop in one call: resets every env (evaluate_policy's env.reset()), meshenv_eval_begin, then per vector step t
 *   policy (exactly one of policy / actor is given, the other NULL):
 *     meshenv_policy_forward(obs, noise counter counter + t when sample != 0, eps = 0 otherwise), meshenv_step (auto-reset on),
 *     meshenv_eval_tally(t)  --  = collect_rollout(T, seed, counter) after a reset: meshenv_step_policy_multi(counter)
 *   actor: the actions of step 0 come from meshenv_actor_sample / _forward on the reset observation with counter, then
 *     meshenv_step_actor(counter + t + 1), meshenv_eval_tally(t)  --  = actor(obs0, counter) followed by
 *     meshenv_step_actor_multi(counter + 1)
 * so the actions of vector step t are always drawn with noise counter counter + t.  Every check_every steps (and after the
 * last) the short counter is copied to a pinned host word of the handle and the stream is synchronised; the loop stops when
 * it is 0 or after max_steps steps.  The records do not depend on check_every (envs past their target are not recorded).
 * *steps_out = vector steps run, *short_out = envs still short of their target (0: finished).  max_steps is required: the
 * reference's loop has no cap, and an episode of rule-0 extractions alone need not end.
 * SYNCHRONISES the stream and is NOT graph-capturable.  Env and policy / actor must share device and stream
 * (MESHENV_E_STATE); MESHENV_E_ARG for both or neither of policy / actor, max_steps or check_every < 1, a missing buffer.
 */
int meshenv_evaluate(MeshEnv *h, MeshPolicy *policy, MeshActor *actor, int sample, uint64_t seed, uint64_t counter, int max_steps,
                     int check_every, const MeshEvalBuffers *bufs, int32_t *steps_out, int32_t *short_out);

/*
 * MeshGeneration.extract_samples_2(meshes, n_neighbor, n_radius, radius, index, quality_threshold), general/mesh.py:1438-1489
 * (the data-preparation step of the ANN scripts: general/EBRD.py:414, 579 with (2, 3, radius 4, index 1) and
 * general/post_processing.py:532 with (3, 3, radius 6, index 5)) for the generated mesh of EVERY env in one launch
 * (csrc/meshenv_samples.h): which = 0 the running episode's elements, 1 the archived (finished) episode.  Needs
 * log_capacity > 0.  Two calls:
 *   1. offsets_dev = NULL: count_dev [n_envs] int64 = samples of every env, status_dev [n_envs] uint8 (0 ok, 1 masked out,
 *      2 log overflow, 3 a vertex with more than 16 neighbours, 4 more than 32 close vertices in a sector: count 0);
 *   2. offsets_dev [n_envs + 1] int64 = where env k's samples start / end (the exclusive prefix sum of the counts; count_dev
 *      and status_dev as the first call left them), samples_dev
 *      [total][2 * (2 n_neighbor + n_radius)], outputs_dev [total][2], types_dev [total] float64: the three lists the
 *      reference returns, env after env, in the reference's order (element, corner, right path, sector tuple, left path).
 * Values: bit-identical to the reference's except the entries of the synthetic sector points, whose coordinates pass
 * through cos / sin of an unquantised angle (<= 2 ulp); reinforcementlearning4meshgeneration_amd.samples is the host
 * restatement (tests/test_gpu_samples.py, tests/test_samples_cpu.py).
 */
int meshenv_extract_samples(MeshEnv *h, int which, const uint8_t *mask_dev, int n_neighbor, int n_radius, double radius, int index,
                            double quality_threshold, int64_t *count_dev, uint8_t *status_dev, const int64_t *offsets_dev,
                            double *samples_dev, double *outputs_dev, double *types_dev);

/* T vector steps of the closed loop in one call: T x meshenv_step_actor on slices of [T]-shaped histories (one launch for
 * all T steps measured slower).
 *   actions_dev   [T+1][n][3]  slice 0 = the actions of the first step (input); slice t + 1 = the policy's actions on
 *                              the observations of step t (output: slice T feeds the next call)
 *   obs_dev [T][n][18], reward_dev [T][n], done_dev [T][n], complete_dev [T][n], terminal_obs_dev [T][n][18] (nullable),
 *   eps_out_dev [T][n][3] (nullable): slice t = what meshenv_step_actor would have written at step t; the noise counter of
 *   step t is counter + t.
 * Bit-identical to T calls of meshenv_step_actor(counter + t) on the slices.  The reference has no counterpart: its loop is SB3's
 * collect_rollouts calling policy and env.step() alternately (rl/baselines/RL_Mesh.py:186-228). */
int meshenv_step_actor_multi(MeshEnv *h, MeshActor *a, int T, float *actions_dev, float *obs_dev, double *reward_dev, uint8_t *done_dev,
                         uint8_t *complete_dev, float *terminal_obs_dev, int auto_reset, int sample, uint64_t seed, uint64_t counter,
                         float *eps_out_dev);

/*
 * Test hook: evaluate one device geometry primitive on n items (in_per_item doubles each) and copy the results
 * back, so the parity tests can compare the device primitives with the oracle's one by one.
 *   what 0 round(python float, 4)   1 round(np.float64, 4)   2 Vertex.to_find_clockwise_angle (6 doubles: s, p1, p2)
 *        3 Segment.is_cross (8 doubles: a1, a2, b1, b2)  4 collinearity class, fast + 2*exact (2 doubles: c, d)
 *        5 round(np.float32, 4)      6 Point2D.distance_to (4 doubles)   7 sqrt_pos == sqrt (1 double)
 *        8 quantised clockwise angle, fast form against exact (2 doubles: c, d): 0 equal, 1 guard band, 2 mismatch
 *        9 / 10 x / y of a front-smoother vertex construction (9 doubles: which = 0 middle_vertex, 1 side_vertex,
 *               2 indention_vertex (general/mesh.py:805-909), 3 Mesh.estimate_4th_vertex (factor, suggest_dist or < 0);
 *               vertex, p1, p2; angle; dist), NaN where it is undefined
 *        11-16 libm building blocks: pow(x, 2), the quantised angle of (c, d), the atan2 tie-breaker, atan2, sin, cos
 *        17 / 18 the x-slab and point_inside pre-filters against the unfiltered tests (7 doubles; any other
 *               in_per_item is MESHENV_E_ARG)
 *        19 one entry of the element quality record for an arbitrary quad (9 doubles: the four vertices (x, y) in
 *               Mesh.vertices order, then the record index 0-7 as in meshenv_element_quality; any other in_per_item
 *               is MESHENV_E_ARG): what meshenv_quad_quality does not expose -- the corner angles, scaled Jacobian,
 *               taper and area of degenerate, concave, inverted and non-finite quads (tests/test_gpu_quality_edges.py)
 */
int meshenv_selftest(int device, int what, int n, int in_per_item, const double *in_host, double *out_host);

#ifdef __cplusplus
}
#endif
#endif /* MESHENV_H */
