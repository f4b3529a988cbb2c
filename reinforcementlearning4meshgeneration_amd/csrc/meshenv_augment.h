// meshenv_augment.h -- the synthetic training samples of the supervised mesher, generated on the device (gfx950, fp64).
//
// What it replaces: MeshAugmentation.sampling of general/data_augmentation.py ("A:"), the set `data_sampling` /
// `hyperparameter_search` of general/EBRD.py train on.  sampling(n, threshold) = sampling_4_type(0.5 n, ., 0.5) +
// sampling_4_type(0.25 n, ., 0) + sampling_4_type(0.25 n, ., 1) (A:131-176); sampling_4_type (A:223-289) walks eleven angle bins
// k = 0.4 .. 2.4 with the quota Q = ceil(n_t / 11) each and, until the bin's count reaches Q, draws angle = random(k - 0.2, k),
// obs = sample_state(angle, type) (A:29-63), skips the proposal if check_obs_quality(obs) (A:291-315), and otherwise scores
// every action of sample_action (A:65-77: twenty random ones for type 0.5, the one copied from obs for 0 and 1) with
// compute_quality (A:470-513) against estimate_max_quality(method=3) (A:447-468).  The count is incremented BEFORE the append and
// the loop leaves at Q, so a bin yields Q - 1 rows.  sampling_main (A:956-986) runs `pool` such samplers and concatenates.
//
// It is rejection sampling (95 % of the proposals fail check_obs_quality, half of the rest give an invalid element, 0.2-0.8 %
// are accepted), so: one lane per proposal, an ordered compaction, one lane per (survivor, action), an ordered selection.
//   k_aug_propose   lane = proposal p of bin g = (w, t, b): its uniforms, obs, check_obs_quality -> flag[slot][p - p0]
//   k_aug_compact   workgroup = bin: the flags of the round -> the survivors' proposal offsets in proposal order, their number
//   k_aug_score     lane = (survivor s, action a) of bin g: obs and action again from the stream, the element, the four
//                   qualities, the accept flag -> acc[slot][s * A + a].  Lanes past the bin's survivors leave at once, so no
//                   wave carries the dead 95 % in its exec mask
//   k_aug_select    workgroup = bin: scans acc in (s, a) order and writes the first rows[g] - count[g] accepted candidates at
//                   their final row offsets (float64 and / or float32), then count[g], next_p[g] and the bin's tallies
// A round covers P proposals of every unfinished bin; the next one continues at proposal index p0 + P.  The host reads count[]
// once per round, to know when to stop and which bins are left: the round's lanes (bins x round_size) are spread over the
// unfinished bins only, so P grows as bins finish (a bin of the narrowest angles at threshold 0.8 accepts one proposal in
// 10^5 and would otherwise crawl on at round_size proposals a round).  Unfinished bins are numbered 0 .. n_active - 1
// ("slots", active[slot] = g) and the round's buffers are laid out by slot.  The rows of a bin are the first Q - 1 accepted
// candidates in (proposal, action) order of the bin's stream, whatever P, the slots and the grid are.  No floating-point
// atomics, no atomics at all.
//
// Random numbers: Philox4x32-10 (csrc/meshenv_actor.h) under a tag of its own.
//   counter words  c0 = p                       proposal index within the bin's stream (32 bits)
//                  c1 = (j >> 1) | b << 8 | t << 16   j = index of the uniform within the proposal (0 .. 56), b = bin 0 .. 10,
//                                               t = type index 0, 1, 2 for types 0.5, 0, 1 (the order sampling() concatenates)
//                  c2 = w                       worker 0 .. pool - 1
//                  c3 = kAugPhiloxTag = 5       (0 rollout noise, 1 replay draw, 2 TD target, 3 SAC actor gradient, 4 warm-up actions)
//   key            (seed lo, seed hi)
//   uniform j      numpy's 53-bit map ((a >> 5) * 2^26 + (b >> 6)) / 2^53 of words (a, b) = (0, 1) of the block for even j,
//                  (2, 3) for odd j
//   draw order     the reference's call order: j = 0 the bin angle, 1 .. 16 sample_state's sixteen in textual order, then for
//                  type 0.5 (radius, angle) of action a at 17 + 2 a, 18 + 2 a: 57 uniforms, 17 for types 0 and 1
// random(lo, hi) = u * (hi - lo) + lo, unfused (-ffp-contract=off), operands in the reference's order.
//
// The geometry is that of meshenv_geom.h / meshenv_quality.h, unchanged and only called: to_find_clockwise_angle with its
// 4-decimal rounding (cw), Segment.is_cross, Segment.distance(Vertex), Mesh.get_quality('strong') (quad_quality_index(., 5)).
// The ten points of a candidate live in LDS ([point][lane], 11 x 64 x 16 bytes a wave) so that the segment loops index them
// without private-memory arrays.
#pragma once

#include "meshenv_actor.h"
#include "meshenv_geom.h"
#include "meshenv_quality.h"

namespace meshenv {

constexpr uint32_t kAugPhiloxTag = 5u;
constexpr int kAugBins = 11;
constexpr int kAugTypes = 3;
constexpr int kAugMaxActions = 20;
constexpr int kAugMaxUniforms = 57;
constexpr int kAugThreads = 64;      // the geometry kernels: one wave per workgroup, 11 KB of LDS
constexpr int kAugScanThreads = 256; // the two scans
constexpr int kAugPoints = 11;       // n_points[0..6], r_points[0..2], the generated vertex
constexpr double kAugLam = 0.618;    // A:247

__device__ __forceinline__ double aug_bin_key(int b)
{
    // float(k) of the keys '0.4', '0.6', ..., '2.4' (A:116-126)
    constexpr double k[kAugBins] = {0.4, 0.6, 0.8, 1.0, 1.2, 1.4, 1.6, 1.8, 2.0, 2.2, 2.4};
    double v = k[0];
#pragma unroll
    for (int i = 1; i < kAugBins; i++) v = b == i ? k[i] : v;
    return v;
}
__device__ __forceinline__ int aug_actions(int t) { return t == 0 ? kAugMaxActions : 1; }
__device__ __forceinline__ double aug_type_label(int t) { return t == 0 ? 0.5 : (t == 1 ? 0.0 : 1.0); }

// ------------------------------------------------------------------------------------------------------------- uniforms
// the two sources of a proposal's uniforms: the bin's Philox stream, or an array the caller recorded (meshenv_augment_propose)
struct AugPhilox {
    uint32_t p, c1, w, k0, k1;
    __device__ __forceinline__ double at(int j) const
    {
        uint32_t r[4];
        philox4x32(p, c1 | (uint32_t)(j >> 1), w, kAugPhiloxTag, k0, k1, r);
        const uint32_t a = (j & 1) ? r[2] : r[0], b = (j & 1) ? r[3] : r[1];
        return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) / 9007199254740992.0;  // exact: 53 bits
    }
};
__device__ __forceinline__ AugPhilox aug_philox(uint64_t seed, int w, int t, int b, uint32_t p)
{
    AugPhilox s;
    s.p = p;
    s.c1 = ((uint32_t)b << 8) | ((uint32_t)t << 16);
    s.w = (uint32_t)w;
    s.k0 = (uint32_t)seed;
    s.k1 = (uint32_t)(seed >> 32);
    return s;
}
struct AugRecorded {
    const double *u;
    __device__ __forceinline__ double at(int j) const { return u[j]; }
};

__device__ __forceinline__ double aug_random(double u, double lo, double hi) { return u * (hi - lo) + lo; }  // A:317-318

// ------------------------------------------------------------------------------------------------------------ proposals
// angle and obs[18] of a proposal: sample_state, A:29-63.  Returns the angle.
template <typename U>
__device__ __forceinline__ double aug_sample_state(const U &src, int t, int b, double *o)
{
    const double k = aug_bin_key(b);
    const double angle = aug_random(src.at(0), k - 0.2, k);  // A:235
    const double third = 1.0 / 3 * angle, two_thirds = 2.0 / 3 * angle;
    o[0] = aug_random(src.at(1), 0.01, 0.45);
    o[1] = 0.0;
    o[2] = aug_random(src.at(2), 0.1, 0.77);
    {
        const double u = src.at(3);
        const double a05 = aug_random(u, -0.5, 0.9) * kPi;      // type 0.5
        const double a0 = aug_random(u, -0.5 * kPi, angle);     // type 0
        const double a1 = aug_random(u, 0.01, angle);           // type 1
        o[3] = t == 0 ? a05 : (t == 1 ? a0 : a1);
    }
    o[4] = aug_random(src.at(4), 0.33, 1.0);
    o[5] = aug_random(src.at(5), -0.5, 0.9) * kPi;
    o[6] = aug_random(src.at(6), 0.15, 1.0);
    o[7] = aug_random(src.at(7), 0.0, third);
    o[8] = aug_random(src.at(8), 0.15, 1.0);
    o[9] = aug_random(src.at(9), third, two_thirds);
    o[10] = aug_random(src.at(10), 0.15, 1.0);
    o[11] = aug_random(src.at(11), two_thirds, angle);
    o[12] = aug_random(src.at(12), 0.33, 1.0);
    o[13] = aug_random(src.at(13), 0.1, 1.5) * kPi;
    o[14] = aug_random(src.at(14), 0.1, 0.77);
    {
        const double u = src.at(15);
        const double wide = aug_random(u, 0.01, 1.5) * kPi;     // types 0.5 and 1
        const double a0 = aug_random(u, 0.01, angle);           // type 0
        o[15] = t == 1 ? a0 : wide;
    }
    o[16] = aug_random(src.at(16), 0.01, 0.45);
    o[17] = angle;
    return angle;
}

// action a of the proposal: sample_action, A:65-77
template <typename U>
__device__ __forceinline__ void aug_sample_action(const U &src, int t, int a, const double *o, double angle, double *act)
{
    act[0] = aug_type_label(t);
    if (t == 0) {
        act[1] = aug_random(src.at(17 + 2 * a), 0.01, 0.56);
        act[2] = aug_random(src.at(18 + 2 * a), 0.01, angle);
    } else {
        act[1] = t == 1 ? o[14] : o[2];
        act[2] = t == 1 ? o[15] : o[3];
    }
}

// -------------------------------------------------------------------------------------------------------------- geometry
// The points of this lane, [point][lane] in LDS: 0..6 = n_points (the origin is 3), 7..9 = r_points, 10 = the generated vertex
// (sample_2_vertices, A:356-383; check_obs_quality builds the same lists, A:292-295).
struct AugPts {
    double *x, *y;  // this lane's column
    __device__ __forceinline__ P2 at(int k) const { return mkp(x[k * kAugThreads], y[k * kAugThreads]); }
    __device__ __forceinline__ void set(int k, P2 p) const
    {
        x[k * kAugThreads] = p.x;
        y[k * kAugThreads] = p.y;
    }
};

__device__ __forceinline__ P2 aug_polar(double r, double a)
{
    const SinCos sc = sincos_nc(a);
    return mkp(r * sc.c, r * sc.s);
}

__device__ __forceinline__ void aug_points(const AugPts &P, const double *o)
{
    // obs pair i -> slot: pairs 0..2 are n_points[4..6], 3..5 r_points, 6..8 n_points[0..2]
#pragma unroll
    for (int i = 0; i < 9; i++) P.set(i < 3 ? 4 + i : (i < 6 ? 4 + i : i - 6), aug_polar(o[2 * i], o[2 * i + 1]));
    P.set(3, mkp(0.0, 0.0));
}

// the far end of "other segment" s = 1..8: s <= 6 the front segment (n[s], n[s-1]), 7 and 8 the radius segments
// (r[1], r[0]) and (r[2], r[1])
__device__ __forceinline__ int aug_seg_head(int s) { return s <= 6 ? s : s + 1; }

// check_obs_quality, A:291-315
__device__ __forceinline__ bool aug_obs_rejected(const AugPts &P)
{
    bool crossed = false;
#pragma unroll 1
    for (int i = 1; i <= 6 && !crossed; i++) {
        const P2 a1 = P.at(i), a2 = P.at(i - 1);
#pragma unroll 1
        for (int s = i + 2 < 7 ? i + 2 : 7; s <= 8 && !crossed; s++) {  // front segments j >= i + 2, both radius segments
            const int h = aug_seg_head(s);
            crossed = is_cross(a1, a2, P.at(h), P.at(h - 1));
        }
    }
    if (crossed) return true;
    double lmin = 0, lmax = 0;
#pragma unroll 1
    for (int i = 1; i <= 6; i++) {
        const double l = dist(P.at(i), P.at(i - 1));
        lmin = (i == 1 || l < lmin) ? l : lmin;
        lmax = (i == 1 || l > lmax) ? l : lmax;
    }
    return lmax / lmin >= 5;
}

struct AugScore {
    bool valid;
    double ele, boundary, max_ele, max_boundary;
};

// slot of quad vertex i: kind 0 -> n[1], n[4], n[3], n[2]; kind 1 -> n[2], n[5], n[4], n[3]; otherwise the generated vertex,
// n[4], n[3], n[2] (A:479-500)
__device__ __forceinline__ int aug_quad_slot(unsigned quad, int i) { return (int)((quad >> (4 * (i & 3))) & 15u); }

// compute_quality (A:470-513) and estimate_max_quality(method=3) (A:447-468) of one candidate whose points are in P
__device__ __forceinline__ AugScore aug_score(const AugPts &P, double kind, double act_r, double act_a)
{
    AugScore R;
    const bool has_new = !(kind == 0.0) && !(kind == 1.0);
    const unsigned quad = kind == 0.0 ? 0x2341u : (kind == 1.0 ? 0x3452u : 0x234Au);
    if (has_new) P.set(10, aug_polar(act_r, act_a));
    P2 m[4];
#pragma unroll
    for (int i = 0; i < 4; i++) m[i] = P.at(aug_quad_slot(quad, i));
    // Mesh.is_valid(0), C:730-749: segments_crossed (C:806-818), then every corner within [0.01 pi, 0.99 pi]
    bool valid = !is_cross(m[0], m[1], m[2], m[3]);
    if (valid) valid = !is_cross(m[0], m[3], m[1], m[2]);
    if (valid) {
#pragma unroll 1
        for (int i = 0; i < 4 && valid; i++) {
            const double d = cw(P.at(aug_quad_slot(quad, i)), P.at(aug_quad_slot(quad, i + 1)), P.at(aug_quad_slot(quad, i + 3)));
            valid = !(d > 0.99 * kPi || d < 0.01 * kPi);
        }
    }
    // check_intersection, A:521-537: a side against every front / radius segment that shares no vertex object with it
    if (valid) {
#pragma unroll 1
        for (int i = 0; i < 4 && valid; i++) {
            const int ia = aug_quad_slot(quad, i), ib = aug_quad_slot(quad, i + 3);
            const P2 a1 = P.at(ia), a2 = P.at(ib);
#pragma unroll 1
            for (int s = 1; s <= 8 && valid; s++) {
                const int h = aug_seg_head(s);
                const bool shares = ia == h || ia == h - 1 || ib == h || ib == h - 1;  // slot 10 and the radius slots never match
                if (!shares) valid = !is_cross(a1, a2, P.at(h), P.at(h - 1));
            }
        }
    }
    // check_internal_element, A:539-552: from each of r[0..2], n[0], n[6] the segment to the centroid crosses a side
    if (valid) {
        const P2 c = mkp(((((0.0 + m[0].x) + m[1].x) + m[2].x) + m[3].x) / 4, ((((0.0 + m[0].y) + m[1].y) + m[2].y) + m[3].y) / 4);
#pragma unroll 1
        for (int k = 0; k < 5 && valid; k++) {
            const P2 v = P.at(k < 3 ? 7 + k : (k == 3 ? 0 : 6));
            bool crossed = false;
#pragma unroll 1
            for (int i = 0; i < 4 && !crossed; i++) crossed = is_cross(v, c, P.at(aug_quad_slot(quad, i)), P.at(aug_quad_slot(quad, i + 3)));
            valid = crossed;
        }
    }
    R.valid = valid;
    R.ele = 0.0;
    R.boundary = 0.0;
    if (valid) {
        R.ele = quad_quality_index(m, 5);  // Mesh.get_quality('strong')
        // compute_boundary_quality, A:554-642
        if (has_new) {
            const P2 v = m[0], left = m[3], right = m[1];  // left = n[2], right = n[4]
            const double left_angle = cw(left, P.at(1), v), right_angle = cw(right, v, P.at(5));
            const bool la = left_angle < kPi / 2, ra = right_angle < kPi / 2;
            const double amin = la ? ((ra && right_angle < left_angle) ? right_angle : left_angle) : right_angle;
            const double q1 = (la || ra) ? 2 * amin / kPi : 1.0;
            const double dsum = dist(v, left) + dist(v, right);
            double m_d = seg_point_distance(P.at(0), P.at(1), v);
            double d = seg_point_distance(P.at(6), P.at(5), v);
            m_d = d < m_d ? d : m_d;
            d = seg_point_distance(P.at(7), P.at(8), v);
            m_d = d < m_d ? d : m_d;
            d = seg_point_distance(P.at(8), P.at(9), v);
            m_d = d < m_d ? d : m_d;
            const double q2 = m_d < dsum ? m_d / dsum : 1.0;
            const double target = dsum / 2;
            const double mean = ((((0.0 + dist(P.at(2), P.at(1))) + dist(v, P.at(2))) + dist(P.at(4), v)) + dist(P.at(5), P.at(4))) / 4;
            const double smooth = (target < mean ? target : mean) / (target > mean ? target : mean);
            R.boundary = pow(q1 * q2 * smooth, 1.0 / 3);
        } else {
            const int lo = kind == 0.0 ? 1 : 2, hi = lo + 3;
            const P2 pl = P.at(lo), ph = P.at(hi), pl1 = P.at(lo - 1), ph1 = P.at(hi + 1);
            const double left_angle = cw(pl, pl1, ph), right_angle = cw(ph, pl, ph1);
            const bool la = left_angle < kPi / 2, ra = right_angle < kPi / 2;
            const double amin = la ? ((ra && right_angle < left_angle) ? right_angle : left_angle) : right_angle;
            const double aq = (la || ra) ? 2 * amin / kPi : 1.0;
            const double target = dist(pl, ph);
            const double mean = (((0.0 + dist(pl, pl1)) + dist(ph, pl)) + dist(ph1, ph)) / 3;
            const double smooth = (target < mean ? target : mean) / (target > mean ? target : mean);
            R.boundary = sqrt(aq * smooth);
        }
    }
    {
        // estimate_max_quality(method=3), A:447-468: the corner at the origin between n[2] and n[4]
        const P2 o = P.at(3), left = P.at(2), right = P.at(4);
        const double angle = cw(o, left, right);
        const double rem = (2 * kPi - angle) / 3;
        const double aq = (rem < angle ? rem : angle) / (rem > angle ? rem : angle);
        const double l1 = dist(o, left), l2 = dist(o, right);
        const double area = l2 * l1 * sin_nc(angle);
        const double ra = sqrt(area);  // NaN where the reference raises (a reflex corner)
        double product = 1.0;
        product *= (ra - l1 > 0) ? l1 / ra : 1.0 / (l1 / ra);
        product *= (ra - l2 > 0) ? l2 / ra : 1.0 / (l2 / ra);
        const double eq = pow(product, 0.25);
        const double d0 = seg_point_distance(P.at(7), P.at(8), o), d1 = seg_point_distance(P.at(8), P.at(9), o);
        const double dmax = d1 > d0 ? d1 : d0;
        const double ratio = dmax / ((sqrt(2.0) / 2 + 0.5) * (l1 + l2));
        R.max_ele = sqrt(aq * eq);
        R.max_boundary = sqrt(ratio < 1.0 ? ratio : 1.0);
    }
    return R;
}

// A:247-255.  False for a NaN on either side, as the comparison is in Python.
__device__ __forceinline__ bool aug_accept(const AugScore &R, double threshold)
{
    const double quality = (1 - kAugLam) * R.ele + kAugLam * R.boundary;
    const double max_quality = (1 - kAugLam) * R.max_ele + kAugLam * R.max_boundary;
    return quality / max_quality >= threshold && R.ele / R.max_ele >= threshold;
}

#define MESHENV_AUG_LDS(P)                                            \
    __shared__ double aug_lds_x[kAugPoints * kAugThreads];            \
    __shared__ double aug_lds_y[kAugPoints * kAugThreads];            \
    AugPts P;                                                         \
    P.x = aug_lds_x + threadIdx.x;                                    \
    P.y = aug_lds_y + threadIdx.x

// --------------------------------------------------------------------------------------------- the two public test entries
// meshenv_augment_propose: recorded uniforms [B][57] -> angle [B], obs [B][18], actions [B][20][3] (rows past the type's
// count zero), rejected [B]
__global__ void __launch_bounds__(kAugThreads)
k_aug_propose_recorded(int n, const double *__restrict__ uniforms, const int32_t *__restrict__ t_index,
                       const int32_t *__restrict__ b_index, double *__restrict__ angle_out, double *__restrict__ obs_out,
                       double *__restrict__ act_out, uint8_t *__restrict__ rejected_out)
{
    MESHENV_AUG_LDS(P);
    const int i = blockIdx.x * kAugThreads + threadIdx.x;
    if (i >= n) return;
    const int t = t_index[i], b = b_index[i];
    AugRecorded src;
    src.u = uniforms + (size_t)i * kAugMaxUniforms;
    double o[18];
    const double angle = aug_sample_state(src, t, b, o);
    angle_out[i] = angle;
#pragma unroll
    for (int k = 0; k < 18; k++) obs_out[(size_t)i * 18 + k] = o[k];
    const int na = aug_actions(t);
#pragma unroll 1
    for (int a = 0; a < kAugMaxActions; a++) {
        double act[3] = {0.0, 0.0, 0.0};
        if (a < na) aug_sample_action(src, t, a, o, angle, act);
        double *dst = act_out + ((size_t)i * kAugMaxActions + a) * 3;
        dst[0] = act[0];
        dst[1] = act[1];
        dst[2] = act[2];
    }
    aug_points(P, o);
    rejected_out[i] = aug_obs_rejected(P) ? 1 : 0;
}

// meshenv_augment_score: obs [B][18], act [B][3] -> rejected, valid [B], q [B][4] = ele, boundary, max_ele, max_boundary,
// accept [B] (threshold <= 0: not written)
__global__ void __launch_bounds__(kAugThreads)
k_aug_score_rows(int n, const double *__restrict__ obs, const double *__restrict__ act, double threshold,
                 uint8_t *__restrict__ rejected_out, uint8_t *__restrict__ valid_out, double *__restrict__ q_out,
                 uint8_t *__restrict__ accept_out)
{
    MESHENV_AUG_LDS(P);
    const int i = blockIdx.x * kAugThreads + threadIdx.x;
    if (i >= n) return;
    double o[18];
#pragma unroll
    for (int k = 0; k < 18; k++) o[k] = obs[(size_t)i * 18 + k];
    aug_points(P, o);
    rejected_out[i] = aug_obs_rejected(P) ? 1 : 0;
    const AugScore R = aug_score(P, act[(size_t)i * 3], act[(size_t)i * 3 + 1], act[(size_t)i * 3 + 2]);
    valid_out[i] = R.valid ? 1 : 0;
    q_out[(size_t)i * 4 + 0] = R.ele;
    q_out[(size_t)i * 4 + 1] = R.boundary;
    q_out[(size_t)i * 4 + 2] = R.max_ele;
    q_out[(size_t)i * 4 + 3] = R.max_boundary;
    if (accept_out) accept_out[i] = aug_accept(R, threshold) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------------ the sampler
// Bin g = (w * 3 + t) * 11 + b.  Per bin on the device: rows[g] = Q - 1 (what the bin owes), row0[g] (its first output row),
// count[g] (rows written), next_p[g] (the proposal index the next round starts at), tally[g][2] (proposals drawn, candidates
// scored), n_surv[g].  Per slot of the round: active[slot] = g, acc_at[slot] = the slot's offset into acc[] (a multiple of 64:
// P is), acc_at[n_active] = the end.
struct AugRound {
    int n_active;          // unfinished bins = slots of this round
    int P;                 // proposals per unfinished bin this round, a multiple of 64
    uint64_t seed;
    double threshold;
    const int32_t *rows;
    const int64_t *row0;
    int32_t *count;
    uint32_t *next_p;
    const int32_t *active; // [n_active]
    const int64_t *acc_at; // [n_active + 1]
    unsigned long long *tally;
    uint8_t *flag;         // [n_active][P]    1 = the proposal passed check_obs_quality
    int32_t *surv;         // [n_active][P]    proposal offsets of the survivors, in order
    int32_t *n_surv;       // [n_bins]
    uint8_t *acc;          // [acc_at[slot] + s * A + a]
    double *x64, *y64;     // [R][18], [R][3]; either pair may be NULL
    float *x32, *y32;
};

__device__ __forceinline__ void aug_bin_of(int g, int &w, int &t, int &b)
{
    b = g % kAugBins;
    t = (g / kAugBins) % kAugTypes;
    w = g / (kAugBins * kAugTypes);
}

__global__ void __launch_bounds__(kAugThreads)
k_aug_propose(AugRound A)
{
    MESHENV_AUG_LDS(P);
    const int slot = blockIdx.y, g = A.active[slot];
    const int k = blockIdx.x * kAugThreads + threadIdx.x;
    if (k >= A.P) return;
    int w, t, b;
    aug_bin_of(g, w, t, b);
    const AugPhilox src = aug_philox(A.seed, w, t, b, A.next_p[g] + (uint32_t)k);
    double o[18];
    aug_sample_state(src, t, b, o);
    aug_points(P, o);
    A.flag[(size_t)slot * A.P + k] = aug_obs_rejected(P) ? 0 : 1;
}

// exclusive prefix of v over the workgroup's kAugScanThreads threads and the workgroup's total; `part` = 4 ints of LDS
__device__ __forceinline__ int aug_block_scan(int v, int *part, int &total)
{
    int incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d, 64);
        if ((int)(threadIdx.x & 63) >= d) incl += o;
    }
    const int wave = threadIdx.x >> 6;
    __syncthreads();  // the previous chunk's readers are done with part[]
    if ((threadIdx.x & 63) == 63) part[wave] = incl;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < kAugScanThreads / 64; i++) {
        const int s = part[i];
        before += i < wave ? s : 0;
        total += s;
    }
    return before + incl - v;
}

__global__ void __launch_bounds__(kAugScanThreads)
k_aug_compact(AugRound A)
{
    __shared__ int part[kAugScanThreads / 64];
    const int slot = blockIdx.x, g = A.active[slot];
    int base = 0;
    for (int k0 = 0; k0 < A.P; k0 += kAugScanThreads) {
        const int k = k0 + threadIdx.x;
        const int f = k < A.P ? A.flag[(size_t)slot * A.P + k] : 0;
        int total;
        const int at = aug_block_scan(f, part, total);
        if (f) A.surv[(size_t)slot * A.P + base + at] = k;
        base += total;
    }
    if (threadIdx.x == 0) A.n_surv[g] = base;
}

__global__ void __launch_bounds__(kAugThreads)
k_aug_score(AugRound A)
{
    MESHENV_AUG_LDS(P);
    // the workgroup's slot: the last one whose candidates start at or before this workgroup's first lane (wave-uniform)
    const long long first = (long long)blockIdx.x * kAugThreads;
    int slot = 0;
    for (int lo = 0, hi = A.n_active - 1; lo <= hi;) {
        const int mid = (lo + hi) >> 1;
        if (A.acc_at[mid] <= first) {
            slot = mid;
            lo = mid + 1;
        } else {
            hi = mid - 1;
        }
    }
    const int g = A.active[slot];
    int w, t, b;
    aug_bin_of(g, w, t, b);
    const int na = aug_actions(t);
    const long long L = first - A.acc_at[slot] + threadIdx.x;
    if (L >= (long long)A.n_surv[g] * na) return;  // whole waves past the survivors leave here
    const int s = (int)(L / na), a = (int)(L - (long long)s * na);
    const AugPhilox src = aug_philox(A.seed, w, t, b, A.next_p[g] + (uint32_t)A.surv[(size_t)slot * A.P + s]);
    double o[18], act[3];
    const double angle = aug_sample_state(src, t, b, o);
    aug_sample_action(src, t, a, o, angle, act);
    aug_points(P, o);
    const AugScore R = aug_score(P, act[0], act[1], act[2]);
    A.acc[A.acc_at[slot] + L] = aug_accept(R, A.threshold) ? 1 : 0;
}

__global__ void __launch_bounds__(kAugScanThreads)
k_aug_select(AugRound A)
{
    __shared__ int part[kAugScanThreads / 64];
    const int slot = blockIdx.x, g = A.active[slot];
    const int have = A.count[g], owed = A.rows[g];
    int w, t, b;
    aug_bin_of(g, w, t, b);
    const int na = aug_actions(t);
    const long long n_cand = (long long)A.n_surv[g] * na;
    const uint32_t p0 = A.next_p[g];
    int base = have;
    for (long long l0 = 0; l0 < n_cand && base < owed; l0 += kAugScanThreads) {  // base is workgroup-uniform
        const long long L = l0 + threadIdx.x;
        const int f = L < n_cand ? A.acc[A.acc_at[slot] + L] : 0;
        int total;
        const int r = base + aug_block_scan(f, part, total);
        if (f && r < owed) {
            const int s = (int)(L / na), a = (int)(L - (long long)s * na);
            const AugPhilox src = aug_philox(A.seed, w, t, b, p0 + (uint32_t)A.surv[(size_t)slot * A.P + s]);
            double o[18], act[3];
            const double angle = aug_sample_state(src, t, b, o);
            aug_sample_action(src, t, a, o, angle, act);
            const size_t row = (size_t)(A.row0[g] + r);
            if (A.x64) {
#pragma unroll
                for (int k = 0; k < 18; k++) A.x64[row * 18 + k] = o[k];
#pragma unroll
                for (int k = 0; k < 3; k++) A.y64[row * 3 + k] = act[k];
            }
            if (A.x32) {
#pragma unroll
                for (int k = 0; k < 18; k++) A.x32[row * 18 + k] = (float)o[k];
#pragma unroll
                for (int k = 0; k < 3; k++) A.y32[row * 3 + k] = (float)act[k];
            }
        }
        base += total;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        A.count[g] = base < owed ? base : owed;
        A.next_p[g] = p0 + (uint32_t)A.P;
        A.tally[2 * g] += (unsigned long long)A.P;
        A.tally[2 * g + 1] += (unsigned long long)n_cand;
    }
}

}  // namespace meshenv
