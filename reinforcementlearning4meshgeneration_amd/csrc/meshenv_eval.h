// meshenv_eval.h -- policy evaluation on the device: SB3's evaluate_policy bookkeeping plus the finished-mesh report, one
// launch after each vector step (include/meshenv.h: meshenv_eval_tally, meshenv_evaluate).
//
// The reference's three evaluation callers (rl/baselines/CustomizeCallback.py:27-141, rl/baselines/testbed.py:150-212,
// v2/src/mesh_rl/evaluation/eval_loop.py:80-103) step a policy until each episode ends and then read the return, the
// length, info['is_complete'], len(env.generated_meshes) and the elements' quality.  Under auto-reset the finished mesh of
// an env survives only until its next episode ends (one archived log half per env, csrc/meshenv_state.h), so it is scored
// here, in the launch that follows the step that finished it.
//
// One lane per env, 64 envs per workgroup (wave 0; see k_eval_tally for the other waves).  Per lane: the accumulators (return as SB3 sums it -- float64 plus the float32
// reward SB3MeshVecEnv hands over -- and the float64 sum), the length, and on `done` one record at slot offset + count
// while count < target.  The quality statistics of the recorded envs are the whole wave's work: the done lanes are found
// by ballot and the workgroup's waves run env_quality (csrc/meshenv_quality.h, the body of k_element_quality) on them
// in turn, one env per wave at a time.
#pragma once

#include "meshenv_quality.h"

namespace meshenv {

constexpr int kEvalWaves = 8;  // waves per workgroup of k_eval_tally: they share the finished meshes of its 64 envs

struct EvalTallyArgs {
    int n, step;
    const double *reward;
    const uint8_t *done, *complete;
    const LastEpisode *last_ep;  // DevCold::last_ep, passed directly: one dependent load less per launch (NULL: no log)
    // per env [n]
    const int32_t *target, *offset;
    int32_t *count, *length, *seen;
    double *ret, *ret_raw;
    int32_t *short_envs;  // [1] envs with count < target
    // per episode [sum target]
    int32_t *ep_env, *ep_domain, *ep_step, *ep_length, *ep_flags, *ep_n_elem, *ep_archive;
    double *ep_return, *ep_return_raw, *ep_quality;
};

// Start of an evaluation: accumulators cleared, the archive counter of every env taken as seen, short = envs with target > 0
// (short_envs must be zero on entry).
__global__ void __launch_bounds__(64) k_eval_begin(DevState S, EvalTallyArgs A)
{
    const int lane = lane_id(), env = blockIdx.x * 64 + lane;
    bool wants = false;
    if (env < A.n) {
        A.count[env] = 0;
        A.length[env] = 0;
        A.ret[env] = 0.0;
        A.ret_raw[env] = 0.0;
        A.seen[env] = A.last_ep ? A.last_ep[env].episodes : 0;
        wants = A.target[env] > 0;
    }
    const unsigned long long m = __ballot(wants);  // one atomic per wave, not one per env
    if (lane == 0 && m) atomicAdd(A.short_envs, (int)__popcll(m));
}

// Workgroup = 64 envs, kEvalWaves waves.  Wave 0 does the bookkeeping (one lane per env) and leaves the recorded lanes and
// their slots in LDS; after the barrier every wave scores every kEvalWaves-th recorded env, so a step that ends the
// episodes of all 64 envs at once (identical envs under a deterministic policy) costs 8 serial reports, not 64.
__global__ void __launch_bounds__(64 * kEvalWaves) k_eval_tally(DevState S, EvalTallyArgs A)
{
    __shared__ int s_slot[64];
    __shared__ unsigned long long s_rec, s_scored;
    const int lane = lane_id(), wave = uniform_i32(threadIdx.x >> 6);
    const int base = blockIdx.x * 64, env = base + lane;
    if (wave == 0) {
        const bool live = env < A.n;
        bool rec = false, archived = false, reached = false;
        int slot = 0;
        if (live) {
            const double r = A.reward[env];
            const int len = A.length[env] + 1;
            const double ret = A.ret[env] + (double)(float)r;  // SB3: current_rewards (float64) += rewards (float32)
            const double raw = A.ret_raw[env] + r;
            // reset_from_domain archives an episode only when it has elements: a moved counter = this step's episode
            const LastEpisode le = A.last_ep ? A.last_ep[env] : LastEpisode{0, 0, 0, 0};
            const int seen = A.seen[env];
            if (A.last_ep && le.episodes != seen) A.seen[env] = le.episodes;
            if (A.done[env]) {
                archived = A.last_ep && le.episodes != seen;
                const int cnt = A.count[env], tgt = A.target[env];
                if (cnt < tgt) {
                    rec = true;
                    slot = A.offset[env] + cnt;
                    A.ep_env[slot] = env;
                    A.ep_domain[slot] = S.scal[env].dom;
                    A.ep_step[slot] = A.step;
                    A.ep_length[slot] = len;
                    A.ep_return[slot] = ret;
                    A.ep_return_raw[slot] = raw;
                    A.ep_flags[slot] = (A.complete[env] ? 1 : 0) | (archived ? (le.flags & 2) : 0);
                    A.ep_n_elem[slot] = A.last_ep ? (archived ? le.n_elem : 0) : -1;
                    if (A.ep_archive) A.ep_archive[slot] = archived ? le.episodes : 0;
                    A.count[env] = cnt + 1;
                    reached = cnt + 1 == tgt;
                }
                A.length[env] = 0;
                A.ret[env] = 0.0;
                A.ret_raw[env] = 0.0;
            } else {
                A.length[env] = len;
                A.ret[env] = ret;
                A.ret_raw[env] = raw;
            }
        }
        s_slot[lane] = slot;
        const unsigned long long rec_mask = __ballot(rec), scored_mask = __ballot(rec && archived);
        const unsigned long long reached_mask = __ballot(reached);  // envs that reached their target: one atomic per wave
        if (lane == 0 && reached_mask) atomicSub(A.short_envs, (int)__popcll(reached_mask));
        if (lane == 0) {
            s_rec = rec_mask;
            s_scored = scored_mask;
        }
    }
    if (!A.ep_quality) return;  // kernel argument: the whole workgroup leaves together
    __syncthreads();
    const unsigned long long rec = s_rec, scored = s_scored;
    unsigned long long todo = ((unsigned long long)(unsigned)uniform_i32((int)(rec >> 32)) << 32) |
                              (unsigned)uniform_i32((int)(unsigned)rec);
    if (!todo) return;
    const DevCold cold = *S.cold;
    for (int k = 0; todo; k++) {
        const int l = __builtin_ctzll(todo);
        todo &= todo - 1;
        if (k % kEvalWaves != wave) continue;
        double *row = A.ep_quality + (size_t)uniform_i32(s_slot[l]) * 4 * kQualityDim;
        if ((scored >> l) & 1) env_quality(S, S.scal[base + l], cold, base + l, 1, nullptr, row, nullptr);
        else if (lane < 4 * kQualityDim) row[lane] = 0.0;  // no archive of this episode: zeros, not the stale mesh
    }
}

}  // namespace meshenv
