/*
 * meshenv_topology.h -- C-ABI of the topology report of the generated meshes (csrc/meshenv_topology.h, DESIGN.md section
 * 27): the `Singularity`, `num_vertices` and `num_elements` columns of the reference's results table
 * (general/post_processing.py:93-161), the valence histogram and the edge counts that tell a closed, conforming quad mesh
 * from one with a hole or a non-manifold edge.  Both calls enqueue on the handle's stream and return: no host copy, no
 * synchronisation.  The conventions are those of meshenv.h (return codes MESHENV_E_*, *_dev device pointers owned by the
 * caller, no CPU fallback); meshenv.h, MESHENV_ABI_VERSION and MeshEvalBuffers are unchanged.
 */
#ifndef MESHENV_TOPOLOGY_H
#define MESHENV_TOPOLOGY_H

#include <stdint.h>

#include "meshenv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MESHENV_TOPOLOGY_DIM 16                /* int32 words per report */

/* report[0] */
#define MESHENV_TOPO_OK 0
#define MESHENV_TOPO_MASKED 1                  /* mask_dev[env] == 0: the other 15 words and the valence row are untouched */
#define MESHENV_TOPO_LOG_OVERFLOW 2            /* the episode outgrew log_capacity: the mesh is not all there */
#define MESHENV_TOPO_DEGREE 3                  /* a vertex with more than 16 neighbours */
#define MESHENV_TOPO_NOT_ARCHIVED 4            /* which = 1 and the env has not finished an episode with elements yet */

/* One launch, one wavefront per env.  which = 0: the running episode of every env; 1: the last archived (finished) one.
 * mask_dev [n_envs] uint8, NULL = all envs.  report_dev [n_envs][16] int32:
 *    0  status (MESHENV_TOPO_*); words 1..15 are 0 for a status other than OK (and untouched for MASKED)
 *    1  n_elements
 *    2  n_vertices: vertices contained in at least one element (unused domain vertices are not counted)
 *    3  singularity: vertices of [2] whose element count is not 1, 2 or 4
 *    4..11  vertices with 1, 2, 3, 4, 5, 6, 7, >= 8 elements
 *   12  n_edges: distinct element edges
 *   13  boundary_edges: element edges used by exactly one element
 *   14  nonmanifold_edges: element edges used by more than two elements
 *   15  front_edges: edges of (domain ring + elements) used an odd number of times, the ring's own use counting once --
 *       the boundary of what is not meshed yet; 0 for a closed mesh
 * valence_dev (NULL = off) [n_envs][meshenv_max_ring + log_capacity] uint8: elements per vertex (saturating at 255) in the
 * vertex numbering of meshenv_get_elements, 0 behind the last vertex and for a status other than OK.
 * Elements are counted as logged: no removal of repeated elements (the environment cannot produce one).
 * MESHENV_E_ARG: h NULL, which not 0 / 1, report_dev NULL; MESHENV_E_STATE: the handle was created with log_capacity = 0. */
int meshenv_mesh_topology(MeshEnv *h, int which, const uint8_t *mask_dev, int32_t *report_dev, uint8_t *valence_dev);

/* Attaches ep_topology_dev [sum of target][16] int32 to the handle (NULL detaches).  While attached, every tally launch
 * -- meshenv_eval_tally and the loops of meshenv_evaluate / meshenv_evaluate_queued -- is followed by one launch that writes,
 * for each episode recorded in that step, the report of its archived mesh into the episode's slot (16 zeros for a record
 * without elements).  The buffer must cover the slots of the MeshEvalBuffers in use and outlive the attachment.  With
 * nothing attached every call enqueues exactly what it did before.
 * MESHENV_E_ARG: h NULL; MESHENV_E_STATE: a non-NULL buffer on a handle created with log_capacity = 0. */
int meshenv_eval_set_topology(MeshEnv *h, int32_t *ep_topology_dev);

/* TEST ENTRY POINT (as meshenv_selftest: no handle, host pointers, null stream, synchronises before it returns): the counting
 * part of the two kernels above on element logs the caller wrote, grid = n_meshes, one wavefront per mesh.  Mesh m is the
 * records elem_offsets_host[m] .. elem_offsets_host[m + 1] (elem_offsets_host[0] = 0, non-decreasing) of quads_host [total][4]
 * on a domain ring of n0_host[m] >= 3 vertices with n_new_host[m] >= 0 generated ones, in the vertex numbering of
 * meshenv_get_elements (domain vertex i -> i, k-th generated vertex -> n0 + k); the call stores generated ids as the log does.
 * THE CONTRACT FOR A RECORD -- of this call and of the element log the kernels read: four DISTINCT ids, each < n0 + n_new.
 * The report of a mesh with a record outside it is undefined.  (This call refuses an id outside [0, n0 + n_new); that the
 * four ids differ is left to the caller.)  Elements are counted as given: a repeated record counts twice.
 * report_host [n_meshes][16] and valence_host (NULL = off) [n_meshes][width] are copied to the device before the launch and
 * back after it, so a caller sees which words and bytes the kernel wrote.  Status is MESHENV_TOPO_OK or MESHENV_TOPO_DEGREE.
 * MESHENV_E_ARG: n_meshes <= 0, a NULL pointer other than valence_host, width <= 0 or > 65535 (16-bit vertex indices),
 * width < n0 + n_new of some mesh, offsets or ids as excluded above; MESHENV_E_HIP: the device refused something. */
int meshenv_topology_selftest(int device, int n_meshes, const int32_t *elem_offsets_host, const int32_t *quads_host,
                              const int32_t *n0_host, const int32_t *n_new_host, int width, int32_t *report_host,
                              uint8_t *valence_host);

#ifdef __cplusplus
}
#endif
#endif /* MESHENV_TOPOLOGY_H */
