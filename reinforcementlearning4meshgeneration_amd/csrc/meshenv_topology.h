// meshenv_topology.h -- the topological part of the reference's results table:
// general/post_processing.py:93-161 (calculate_metrics) scores a generated mesh by the element-quality measures
// (csrc/meshenv_quality.h) and by `Singularity`, `num_vertices`, `num_elements`.  Singularity = the mesh vertices whose
// element count is not 1, 2 or 4 (post_processing.py:145-151); the vertices are those of the exported *NODE list, i.e. the
// ones contained in at least one element.  Beside those three the report counts what tells a closed, conforming quad mesh
// from one with a hole or a non-manifold edge: the valence histogram, the element edges by their number of uses, and the
// edges that still bound unmeshed area.
//
// One wavefront per environment, one lane per vertex in steps of 64 over the n0 + n_new vertices (unified index: domain
// vertex i -> i, k-th generated vertex -> n0 + k, the ids meshenv_get_elements returns).  Every lane scans the element log
// in order (all lanes read the same 16-byte record) and keeps its neighbour slots, their use counts and its element count
// in registers -- the scan of build_segment_lists (csrc/meshenv_smooth.h), restated here because the report needs the
// per-slot use word and no adjacency in LDS: everything it returns is a sum over lanes.  The scan is O(V * E) compares per
// env (V, E <= a few hundred: a few 10^4 per env, spread over 64 lanes) against one 16-byte broadcast load per element.
//
// The reference removes elements with equal sorted vertex sets before it counts (post_processing.py:27-32, 81-89).  The
// environment cannot log such a pair -- the reference vertex of every extraction leaves the ring for good -- so this kernel
// does NOT dedup: a repeated record counts twice (tests/test_gpu_topology_crafted.py holds it to that).
#pragma once

#include "meshenv_eval.h"
#include "meshenv_smooth.h"

namespace meshenv {

constexpr int kTopologyDim = 16;

// report[0]
enum { kTopoOk = 0, kTopoMasked = 1, kTopoLogOverflow = 2, kTopoDegree = 3, kTopoNotArchived = 4 };
// report[1..15] with status 0
enum { kTopoElements = 1, kTopoVertices = 2, kTopoSingularity = 3, kTopoValence1 = 4, kTopoEdges = 12, kTopoBoundaryEdges = 13,
       kTopoNonManifoldEdges = 14, kTopoFrontEdges = 15 };

__device__ __forceinline__ int wave_sum_i32(int v)
{
#define STEP(CTRL, MASK) { v += dpp_i32<CTRL, MASK>(0, v); }
    MESHENV_DPP_REDUCE(STEP)
#undef STEP
    return lane_i32(v, 63);
}

// What one vertex sees of the mesh: its neighbours in first-occurrence order (slot j < d), per slot the number of elements
// that use the edge (2 bits, saturating at 3 = "more than two") and the parity of (ring + element) uses, and the number of
// elements that contain it.  A domain vertex starts with its two ring edges: no element use, odd parity.
struct VertexLinks {
    unsigned short nb[kSmoothMaxDeg];
    unsigned int uses;     // 2 bits per slot
    unsigned int parity;   // 1 bit per slot
    int d, n_mesh;
    bool too_many;         // more than kSmoothMaxDeg neighbours
};

// u_me: unified index of the lane's vertex; active = false: the lane has no vertex (it still walks the log with the wave)
__device__ __forceinline__ void scan_vertex_links(const int4 *__restrict__ quads, int n_elem, int n0, int u_me, bool active,
                                                  VertexLinks &L)
{
    const int me = u_me >= n0 ? (kNewBit | (u_me - n0)) : u_me;
#pragma unroll
    for (int j = 0; j < kSmoothMaxDeg; j++) L.nb[j] = 0;
    L.uses = 0u; L.parity = 0u; L.d = 0; L.n_mesh = 0; L.too_many = false;
    if (active && u_me < n0) {
        L.nb[0] = (unsigned short)(u_me == 0 ? n0 - 1 : u_me - 1);
        L.nb[1] = (unsigned short)(u_me == n0 - 1 ? 0 : u_me + 1);
        L.d = 2;
        L.parity = 3u;
    }
    for (int e = 0; e < n_elem; e++) {
        const int4 q = quads[e];
        const int p = q.x == me ? 0 : (q.y == me ? 1 : (q.z == me ? 2 : (q.w == me ? 3 : -1)));
        if (p < 0 || !active) continue;
        L.n_mesh += 1;
        // the two edges of the quad at position p: (p, p - 1) and (p + 1, p)
        const int first_g = p == 0 ? q.w : (p == 1 ? q.x : (p == 2 ? q.y : q.z));
        const int second_g = p == 0 ? q.y : (p == 1 ? q.z : (p == 2 ? q.w : q.x));
#pragma unroll
        for (int s = 0; s < 2; s++) {
            const int g = s == 0 ? first_g : second_g;
            const unsigned short u = (unsigned short)((g & kNewBit) ? n0 + (g & ~kNewBit) : g);
            int at = -1;
#pragma unroll
            for (int j = 0; j < kSmoothMaxDeg; j++) at = (at < 0 && j < L.d && L.nb[j] == u) ? j : at;
            if (at < 0) {
                if (L.d < kSmoothMaxDeg) {
#pragma unroll
                    for (int j = 0; j < kSmoothMaxDeg; j++)
                        if (j == L.d) L.nb[j] = u;
                    at = L.d;
                    L.d += 1;
                } else {
                    L.too_many = true;
                }
            }
            if (at >= 0) {
                if (((L.uses >> (2 * at)) & 3u) != 3u) L.uses += 1u << (2 * at);
                L.parity ^= 1u << at;
            }
        }
    }
}

// The counting: the report of ONE mesh, computed by a whole wave (every argument is wave-uniform, all 64 lanes take part).
// quads = n_elem records of the element log (generated ids carry kNewBit) on a domain ring of n0 vertices with n_new
// generated ones.  Contract for a record: four distinct ids, each < n0 + n_new; anything else is undefined.  report = the
// mesh's 16 words; valence_row (nullable) = its `width` bytes, width >= n0 + n_new.  code = the status the caller has
// arrived at: kTopoOk -> the mesh is counted (status kTopoOk or kTopoDegree); anything else -> nothing is read and the
// report is that status, words 1..15 and the valence row 0.  (The refusals of env_topology pass through here so that the
// function has one exit and one store: the two shipped kernels compile to what they were before the split.)
__device__ __forceinline__ void mesh_topology(const int4 *__restrict__ quads, int n_elem, int n0, int n_new,
                                              int32_t *__restrict__ report, uint8_t *__restrict__ valence_row, int width,
                                              int code = kTopoOk)
{
    const int lane = lane_id();
    int acc[kTopologyDim] = {};
    if (code == kTopoOk) {
        const int nv = n0 + n_new;
        bool too_many = false;
        for (int v0 = 0; v0 < nv; v0 += 64) {
            const int u_me = v0 + lane;
            const bool active = u_me < nv;
            VertexLinks L;
            scan_vertex_links(quads, n_elem, n0, u_me, active, L);
            too_many = too_many || L.too_many;
            const int nm = L.n_mesh;
            if (valence_row && active) valence_row[u_me] = (uint8_t)(nm > 255 ? 255 : nm);
            acc[kTopoVertices] += nm > 0 ? 1 : 0;
            acc[kTopoSingularity] += (nm > 0 && nm != 1 && nm != 2 && nm != 4) ? 1 : 0;
            const int bin = nm > 8 ? 8 : nm;
#pragma unroll
            for (int b = 1; b <= 8; b++) acc[kTopoValence1 + b - 1] += bin == b ? 1 : 0;
            // an edge is counted once, at its lower-index endpoint
#pragma unroll
            for (int j = 0; j < kSmoothMaxDeg; j++) {
                const bool mine = j < L.d && (int)L.nb[j] > u_me;
                const unsigned int c = (L.uses >> (2 * j)) & 3u;
                acc[kTopoEdges] += (mine && c != 0u) ? 1 : 0;
                acc[kTopoBoundaryEdges] += (mine && c == 1u) ? 1 : 0;
                acc[kTopoNonManifoldEdges] += (mine && c == 3u) ? 1 : 0;
                acc[kTopoFrontEdges] += (mine && ((L.parity >> j) & 1u) != 0u) ? 1 : 0;
            }
        }
        if (__ballot(too_many) != 0ULL) code = kTopoDegree;
        if (valence_row && code == kTopoOk)
            for (int i = nv + lane; i < width; i += 64) valence_row[i] = 0;
    }
    int r = 0;
    if (code == kTopoOk) {
#pragma unroll
        for (int k = kTopoVertices; k < kTopologyDim; k++) {
            const int s = wave_sum_i32(acc[k]);
            r = lane == k ? s : r;
        }
        r = lane == kTopoElements ? n_elem : r;
    } else {
        r = lane == 0 ? code : 0;
        if (valence_row) {
            __threadfence();   // kTopoDegree: the counts written above are overwritten, by other lanes
            for (int i = lane; i < width; i += 64) valence_row[i] = 0;
        }
    }
    if (lane < kTopologyDim) report[lane] = r;
}

// Reads the env: which = 0: the running episode; 1: the last archived (finished) episode -- element and vertex counts, log
// half, overflow, n0 -- and hands the log, or the status that keeps it from being read, to mesh_topology.  env and which are
// wave-uniform and all 64 lanes take part.  report = the env's 16 words; valence_row (nullable) = the env's `width` bytes
// (width >= n0 + n_new: ring stride + log capacity).  sc = S.scal[env].
__device__ __forceinline__ void env_topology(const DevState &S, const EnvScalars &sc, const DevCold &cold, int env, int which,
                                             int32_t *__restrict__ report, uint8_t *__restrict__ valence_row, int width)
{
    const int log_cap = S.prm.log_cap;
    int n_elem = uniform_i32(sc.n_elem), n_new = uniform_i32(sc.n_new);
    const int status = uniform_i32(sc.status);
    bool overflow = (status & kStLogOverflow) != 0;
    int half = (status >> 4) & 1;
    int code = kTopoOk;
    if (which) {
        const LastEpisode le = cold.last_ep[env];
        if (uniform_i32(le.episodes) <= 0) code = kTopoNotArchived;
        n_elem = uniform_i32(le.n_elem); n_new = uniform_i32(le.n_new);
        overflow = (uniform_i32(le.flags) & 2) != 0;
        half ^= 1;
    }
    if (code == kTopoOk && (overflow || n_elem > log_cap || n_new > log_cap)) code = kTopoLogOverflow;
    int n0 = 0;
    const int4 *quads = nullptr;
    if (code == kTopoOk) {
        n0 = uniform_i32(S.dom[uniform_i32(sc.dom)].n0);
        quads = reinterpret_cast<const int4 *>(cold.log_quads + ((size_t)env * 2 + half) * log_cap * 4);
    }
    mesh_topology(quads, n_elem, n0, n_new, report, valence_row, width, code);
}

// report [E][16]; valence (nullable) [E][width] uint8, width = ring stride of the public interface (meshenv_max_ring) +
// log capacity.  A masked env gets report[0] = 1 and nothing else.
__global__ void __launch_bounds__(64)
k_mesh_topology(DevState S, int which, const uint8_t *__restrict__ mask, int32_t *__restrict__ report,
                uint8_t *__restrict__ valence, int width)
{
    const int env = blockIdx.x;
    if (mask && mask[env] == 0) {
        if (lane_id() == 0) report[(size_t)env * kTopologyDim] = kTopoMasked;
        return;
    }
    const EnvScalars sc = S.scal[env];
    const DevCold cold = load_cold(S);
    env_topology(S, sc, cold, env, which, report + (size_t)env * kTopologyDim,
                 valence ? valence + (size_t)env * width : nullptr, width);
}

// Launched directly after k_eval_tally with the same arguments and the same shape (64 envs per workgroup, kEvalWaves waves).
// The envs recorded in this step are read off the tally's own outputs: count[env] > 0 and the step of the env's newest record
// = this step.  A record with elements gets the report of the archived mesh (the episode's next one has not ended yet), the
// others 16 zeros.  Every wave finds the recorded envs for itself (one lane per env) and takes every kEvalWaves-th.
__global__ void __launch_bounds__(64 * kEvalWaves) k_eval_topology(DevState S, EvalTallyArgs A, int32_t *__restrict__ ep_topology)
{
    const int lane = lane_id(), wave = uniform_i32(threadIdx.x >> 6);
    const int base = blockIdx.x * 64, env = base + lane;
    bool rec = false, scored = false;
    int slot = 0;
    if (env < A.n) {
        const int cnt = A.count[env];
        if (cnt > 0) {
            slot = A.offset[env] + cnt - 1;
            rec = A.ep_step[slot] == A.step;
            scored = rec && A.ep_n_elem[slot] > 0;
        }
    }
    unsigned long long todo = __ballot(rec);
    const unsigned long long scored_mask = __ballot(scored);
    if (!todo) return;
    const DevCold cold = *S.cold;
    for (int k = 0; todo; k++) {
        const int l = __builtin_ctzll(todo);
        todo &= todo - 1;
        if (k % kEvalWaves != wave) continue;
        int32_t *row = ep_topology + (size_t)lane_i32(slot, l) * kTopologyDim;
        if ((scored_mask >> l) & 1) env_topology(S, S.scal[base + l], cold, base + l, 1, row, nullptr, 0);
        else if (lane < kTopologyDim) row[lane] = 0;
    }
}

// meshenv_topology_selftest (include/meshenv_topology.h): mesh_topology on logs the caller wrote -- grid = meshes, one wavefront
// per mesh, mesh m = the records elem_offsets[m] .. elem_offsets[m + 1] of quads.
__global__ void __launch_bounds__(64)
k_topology_selftest(const int32_t *__restrict__ elem_offsets, const int4 *__restrict__ quads, const int32_t *__restrict__ n0,
                    const int32_t *__restrict__ n_new, int32_t *__restrict__ report, uint8_t *__restrict__ valence, int width)
{
    const int m = blockIdx.x;
    const int first = uniform_i32(elem_offsets[m]);
    mesh_topology(quads + first, uniform_i32(elem_offsets[m + 1]) - first, uniform_i32(n0[m]), uniform_i32(n_new[m]),
                  report + (size_t)m * kTopologyDim, valence ? valence + (size_t)m * width : nullptr, width);
}

}  // namespace meshenv
