/*
 * oracle/meshenv_ref.c -- TEST INFRASTRUCTURE, NOT PRODUCT CODE (see meshenv_ref.h).
 *
 * Scalar restatement of the reference's BoudaryEnv step()/reset().  Line cites
 * "B:" = v2/src/mesh_rl/legacy/boundary_env_legacy.py (== rl/boundary_env.py, +17 lines),
 * "M:" = .../mesh_legacy.py (== general/mesh.py, +26), "C:" = .../components_legacy.py
 * (== general/components.py, +8), "D:" = .../data_legacy.py.
 *
 * Numerics rules (all verified against the reference run in this container,
 * CPython 3.10.12 + numpy 2.2.6 + glibc libm):
 *   - build with -ffp-contract=off: Python never fuses a*b+c;
 *   - Python `x ** 2` on a float is libm pow(x, 2.0), which is NOT always x*x
 *     (0.085 % of random doubles differ by 1 ulp) -> SQ() calls pow();
 *   - round(python_float, 4) is correctly-rounded decimal rounding (round4_py);
 *     round(np.float64, 4) is rint(x*1e4)/1e4 (round4_np); round(np.float32, 4)
 *     is the same in float32 (round4_npf).  New vertices carry np.float64
 *     coordinates (B:123 rounds a numpy array element), domain vertices carry
 *     Python floats/ints, and the result type of `a - b` follows NumPy
 *     promotion, so which rounding applies depends on vertex provenance;
 *   - np.float32 <op> python_float compares in float32 (NEP 50 weak scalars);
 *   - builtin sum() is a plain left-to-right loop starting from int 0.
 */
#include "meshenv_ref.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#define PI 3.141592653589793 /* math.pi */

/* Transcendental call counters of the calling thread (bench.py reports the reference algorithm's fp64 atan2 / sin /
 * cos count per env-step next to the roofline).  One thread-local increment per libm call. */
static __thread uint64_t g_math_calls[3];
static inline double c_atan2(double y, double x) { g_math_calls[0]++; return atan2(y, x); }
static inline double c_sin(double x) { g_math_calls[1]++; return sin(x); }
static inline double c_cos(double x) { g_math_calls[2]++; return cos(x); }
void meshenv_ref_math_calls(uint64_t *out /*[3]: atan2, sin, cos*/, int reset)
{
    for (int i = 0; i < 3; i++) {
        out[i] = g_math_calls[i];
        if (reset) g_math_calls[i] = 0;
    }
}
#define atan2 c_atan2
#define sin c_sin
#define cos c_cos

typedef struct {
    double x, y;
} P2;

struct RefEnv {
    int n0, n;
    P2 *ring;          /* updated_boundary.vertices */
    int32_t *rid;      /* ring slot -> global vertex id (index in boundary.vertices) */
    uint8_t *cand;     /* slot is in candidate_vertices */
    double *key;       /* cached key (degrees) */
    int64_t *stamp;    /* insertion order; larger = nearer the list head among equal keys */
    int64_t counter;
    int ref;           /* ring index of current_point_environment.reference_point, -1 = None */
    double bl;         /* current_point_environment.base_length */
    int n_elem, failed, n_vert;
    double cur_area;
    /* domain */
    P2 *ring0;
    double orig_area, min_l, crit_l;
    /* move() API: not_valid_points (B:47, reference points of rejected moves; matched by distance < 0.001, M:428-433) */
    P2 *nv;
    int32_t *nv_id;    /* global vertex id of each listed vertex (the list holds Vertex objects: identity) */
    int n_nv;
    /* last_not_valid_points (B:48, 416-422): set only where move() smooths, NOT cleared by reset() -- first / last entry
     * and length are all the reference compares; a vertex is the same object only within one episode (reset() deep-copies) */
    int32_t last_first, last_last, last_count, last_epoch, epoch;
    /* the geometry constants of MeshEnvParams (include/meshenv.h); meshenv_ref_create sets the reference's literals */
    double radius, max_ref_angle, key_lambda, min_degree, max_degree, same_point_eps, ray_length;
    /* logs */
    int cap_v, cap_e;
    P2 *vtab;
    int32_t *quads;
};

/* ------------------------------------------------------------------ rounding */

double meshenv_ref_round4_py(double x)
{
    if (!isfinite(x)) return x;
    double ax = fabs(x);
    double y = ax * 1e4;
    if (y >= 4503599627370496.0) return x;
    double e = fma(ax, 1e4, -y); /* exact: ax*1e4 == y + e */
    double f = floor(y);
    double t = (y - f) - 0.5;
    double s = t + e;
    double r;
    if (s > 0) r = f + 1;
    else if (s < 0) r = f;
    else r = (fmod(f, 2.0) == 0.0) ? f : f + 1;
    return copysign(r / 1e4, x);
}

double meshenv_ref_round4_np(double x) { return rint(x * 1e4) / 1e4; }

float meshenv_ref_round4_npf(float x) { return rintf(x * 1e4f) / 1e4f; }

#define round4_py meshenv_ref_round4_py
#define round4_np meshenv_ref_round4_np
#define round4_npf meshenv_ref_round4_npf

/* ---------------------------------------------------------------- primitives */

static inline double SQ(double v) { return pow(v, 2.0); } /* Python `v ** 2` */

/* Point2D.distance_to, C:25-26 */
static inline double dist(P2 a, P2 b) { return sqrt(SQ(a.x - b.x) + SQ(a.y - b.y)); }

/* Vertex.to_find_clockwise_angle, C:99-108 */
static double cw(P2 s, P2 p1, P2 p2)
{
    double v1x = p1.x - s.x, v1y = p1.y - s.y;
    double v2x = p2.x - s.x, v2y = p2.y - s.y;
    double theta = -atan2(v1x * v2y - v1y * v2x, v1x * v2x + v1y * v2y);
    if (copysign(1.0, theta) >= 0) return round4_py(theta);
    return round4_py(2 * PI + theta);
}

double meshenv_ref_cw(double sx, double sy, double ax, double ay, double bx, double by)
{
    P2 s = {sx, sy}, a = {ax, ay}, b = {bx, by};
    return cw(s, a, b);
}

/* cross_product, C:490-491 */
static inline double crossp(double ax, double ay, double bx, double by) { return ax * by - bx * ay; }

/* Segment.straddle, C:499-524; self = (p1,p2), another = (q1,q2) */
static int straddle(P2 p1, P2 p2, P2 q1, P2 q2)
{
    double s1 = round4_py(sin(cw(p1, q1, p2)));
    double s2 = round4_py(sin(cw(p1, q2, p2)));
    if (s1 == s2 && s2 == 0) {
        double l1 = dist(p1, p2), l2 = dist(q1, q2);
        if (l1 > l2) {
            P2 m = {(p2.x + p1.x) / 2, (p2.y + p1.y) / 2};
            double a = dist(m, q2), b = dist(m, q1);
            if ((b < a ? b : a) <= l1 / 2) return 1;
        } else {
            P2 m = {(q2.x + q1.x) / 2, (q2.y + q1.y) / 2};
            double a = dist(m, p2), b = dist(m, p1);
            if ((b < a ? b : a) <= l2 / 2) return 1;
        }
        return 0;
    }
    double v1x = q1.x - p1.x, v1y = q1.y - p1.y;
    double v2x = q2.x - p1.x, v2y = q2.y - p1.y;
    double vmx = p2.x - p1.x, vmy = p2.y - p1.y;
    return crossp(v1x, v1y, vmx, vmy) * crossp(v2x, v2y, vmx, vmy) <= 0;
}

/* Segment.is_cross, C:526-541 */
static int is_cross(P2 a1, P2 a2, P2 b1, P2 b2) { return straddle(a1, a2, b1, b2) && straddle(b1, b2, a1, a2); }

int meshenv_ref_is_cross(const double *a1, const double *a2, const double *b1, const double *b2)
{
    P2 A1 = {a1[0], a1[1]}, A2 = {a2[0], a2[1]}, B1 = {b1[0], b1[1]}, B2 = {b2[0], b2[1]};
    return is_cross(A1, A2, B1, B2);
}

/* Python list index with negative wrap, for k in [-n, 2n) */
static inline int RI(int k, int n) { return ((k % n) + n) % n; }

/* ------------------------------------------------------- candidate list (a5) */

/* MeshGeneration.check_boundary_point, M:228-257; returns 0 for None */
static int check_boundary_point(const RefEnv *e, int index, double *out)
{
    int n = e->n;
    P2 v = e->ring[index];
    double w0 = e->key_lambda, w1 = 1 - e->key_lambda;
    double a0 = cw(v, e->ring[(index + 1) % n], e->ring[RI(index - 1, n)]);
    if (a0 >= e->max_ref_angle || a0 == 0) return 0;
    double sum_angle = 0;
    sum_angle += a0 * w0;
    double a1 = cw(v, e->ring[(index + 2) % n], e->ring[RI(index - 2, n)]);
    sum_angle += a1 * w1;
    *out = sum_angle * (180.0 / PI); /* math.degrees */
    return 1;
}

/* find_reference_candidates, M:259-287: stable sort by key -> ties in ring order */
static void find_reference_candidates(RefEnv *e)
{
    for (int i = 0; i < e->n; i++) {
        double k;
        if (check_boundary_point(e, i, &k)) {
            e->cand[i] = 1;
            e->key[i] = k;
            e->stamp[i] = -(int64_t)i;
        } else {
            e->cand[i] = 0;
        }
    }
    e->counter = 0;
}

/* add_reference_candidates, M:206-226: insert before the first entry with key >= new key */
static void add_candidate(RefEnv *e, int pos)
{
    double k;
    if (check_boundary_point(e, pos, &k)) {
        e->cand[pos] = 1;
        e->key[pos] = k;
        e->stamp[pos] = ++e->counter;
    }
}

/* is_vertex_inside_list, M:428-433 */
static int in_not_valid(const RefEnv *e, P2 v)
{
    for (int k = 0; k < e->n_nv; k++)
        if (dist(e->nv[k], v) < 0.001) return 1;
    return 0;
}

/* find_reference_point, M:295-316: list head; with not_valid_points (use_nv, the move() API) the first list entry that
 * is not within 0.001 of one of them */
static int select_reference_nv(const RefEnv *e, int use_nv)
{
    int best = -1;
    for (int i = 0; i < e->n; i++) {
        if (!e->cand[i]) continue;
        if (use_nv && e->n_nv > 0 && in_not_valid(e, e->ring[i])) continue;
        if (best < 0 || e->key[i] < e->key[best] ||
            (e->key[i] == e->key[best] && e->stamp[i] > e->stamp[best]))
            best = i;
    }
    return best;
}

/* -------------------------------------------------------- observation (a6) */

/* PointEnvironment.get_neighbors + get_radius_points, C:1081-1090, 1192-1290;
 * find_next_state, B:521-588 */
static int find_next_state_opt(RefEnv *e, float *obs, int is_static, int use_nv);

/* is_static: PointEnvironment(static=True), C:1213-1218 -- row 0 carries 0 instead of the area ratio */
static int find_next_state_opt(RefEnv *e, float *obs, int is_static, int use_nv)
{
    e->ref = select_reference_nv(e, use_nv);
    if (e->ref < 0) {
        memset(obs, 0, 18 * sizeof(float));
        return 1;
    }
    const int n = e->n, idx = e->ref;
    const P2 *ring = e->ring;
    const P2 ref = ring[idx];
    const P2 right = ring[RI(idx - 1, n)];
    const P2 left = ring[(idx + 1) % n];
    const double area_ratio = e->cur_area / e->orig_area;

    /* neighbors = [idx+3, idx+2, idx+1, idx, idx-1, idx-2, idx-3]; C:435-444 */
    P2 nb[7];
    for (int i = 0; i < 4; i++) nb[i] = ring[(idx + 3 - i) % n];
    for (int i = 1; i <= 3; i++) nb[3 + i] = ring[RI(idx - i, n)];
    double sum = 0;
    for (int i = 1; i < 7; i++) sum += dist(nb[i], nb[i - 1]);
    const double bl = round4_py(sum / 6);
    e->bl = bl;
    const double target_length = bl * e->radius;
    const double theta = cw(ref, left, right);

    float r[9][2];
    for (int i = 0; i < 9; i++) r[i][0] = r[i][1] = 1.0f;

    r[0][0] = (float)((dist(ref, right) / e->radius) / bl);
    r[0][1] = is_static ? 0.0f : (float)area_ratio;
    r[8][0] = (float)((dist(ref, left) / e->radius) / bl);
    r[8][1] = (float)theta;
    for (int i = 1; i < 3; i++) {
        P2 pr = ring[RI(idx - i - 1, n)];
        double a = cw(ref, pr, right);
        r[i][0] = (float)((dist(ref, pr) / e->radius) / bl);
        r[i][1] = (float)(a < PI ? a : fmax(a, 1.5 * PI) - 2 * PI);
        P2 pl = ring[(idx + 1 + i) % n];
        a = cw(ref, pl, right);
        r[8 - i][0] = (float)((dist(ref, pl) / e->radius) / bl);
        r[8 - i][1] = (float)fmin(a, theta + PI / 2);
    }

    P2 refp1 = {ref.x + 1, ref.y};
    const double rot = cw(ref, right, refp1);
    for (int i = 0; i < 3; i++) {
        double a = ((2 * i + 1) * theta) / 6;
        r[3 + i][1] = (float)fmin(a, theta + PI / 2);
    }
    /* Vertex.rotate about the origin, C:154-168 */
    double px = target_length * cos(theta / 2), py = target_length * sin(theta / 2);
    double qx = (0.0 + cos(rot) * px) - sin(rot) * py;
    double qy = (0.0 + sin(rot) * px) + cos(rot) * py;
    const P2 ps = {ref.x + qx, ref.y + qy};

    double shortest = 1.0;
    int shortest_i = 0;
    const int i_right = RI(idx - 1, n), i_left = (idx + 1) % n;
    for (int i = idx - 1; i > idx - n; i--) {
        const int ii = RI(i, n);
        const P2 v = ring[ii];
        const double d = dist(ref, v);
        if (ii == i_right || ii == i_left) continue;
        const double angle = cw(ref, v, right);
        if (angle == 0) continue;
        const double kf = angle / (theta / 3);
        if (kf < 3.0 && d < target_length) { /* int(kf) < 3  <=>  kf < 3 for kf >= 0 */
            const int k = (int)kf;
            const float cnd = (float)((d / e->radius) / bl);
            if (r[k + 3][0] > cnd) {
                r[k + 3][0] = cnd;
                r[k + 3][1] = (float)fmin(angle, theta + PI / 2);
            }
        }
        /* Segment(ref, ps).intersection_vertex(Segment(ring[i], ring[i+1])), C:657-676 */
        const P2 a = v, b = ring[RI(i + 1, n)];
        const double ux = ps.x - ref.x, uy = ps.y - ref.y;
        const double wx = b.x - a.x, wy = b.y - a.y;
        double s, h;
        if (wy == 0) {
            if (uy == 0) continue;
            s = (a.y - ref.y) / uy;
            h = (ref.x - a.x + s * ux) / wx;
        } else if (wx == 0) {
            if (ux == 0) continue;
            s = (a.x - ref.x) / ux;
            h = (ref.y - a.y + s * uy) / wy;
        } else {
            s = ((ref.x - a.x) / wx - (ref.y - a.y) / wy) / (uy / wy - ux / wx);
            h = (ref.x - a.x + s * ux) / wx;
        }
        if (0 < s && s < 1 && 0 < h && h < 1) {
            P2 vv = {ref.x + s * ux, ref.y + s * uy};
            double val = (dist(ref, vv) / e->radius) / bl;
            if (shortest > val) {
                shortest = val;
                shortest_i = i;
            }
        }
    }
    if (shortest != 1 && (float)shortest < r[4][0]) {
        for (int i = 0; i < 3; i++) {
            P2 v = ring[RI(i - 1 + shortest_i, n)];
            r[3 + i][0] = (float)((dist(ref, v) / e->radius) / bl);
            r[3 + i][1] = (float)cw(ref, v, right);
        }
    }
    for (int i = 0; i < 9; i++) {
        obs[2 * i] = round4_npf(r[i][0]);
        obs[2 * i + 1] = round4_npf(r[i][1]);
    }
    return 0;
}

/* ----------------------------------------------------- point in polygon (a7) */

static inline double round4_by(int is_np, double v) { return is_np ? round4_np(v) : round4_py(v); }

/* is_point_inside_area -> calculate_crossing_segments, M:565-572, 74-128 */
static int is_point_inside_area(const RefEnv *e, P2 p)
{
    const int n = e->n, n0 = e->n0;
    const P2 *ring = e->ring;
    const P2 far = {e->ray_length, p.y};
    int count = 0;
    for (int i = 0; i < n; i++) {
        const int im1 = RI(i - 1, n), im2 = RI(i - 2, n), ip1 = (i + 1) % n;
        const int np_i = e->rid[i] >= n0, np_im1 = e->rid[im1] >= n0;
        const double orientation = round4_by(np_i || np_im1, ring[i].y - ring[im1].y);
        if (orientation == 0) continue;
        if (!is_cross(ring[i], ring[im1], p, far)) continue;
        if (round4_np(ring[i].y - p.y) == 0) {
            const double next_o = round4_by(e->rid[ip1] >= n0 || np_i, ring[ip1].y - ring[i].y);
            if (next_o == 0) continue;
            else if (next_o * orientation < 0) continue;
            else if (orientation < 0) count += 1;
        } else if (round4_np(ring[im1].y - p.y) == 0) {
            const double pre_o = round4_by(np_im1 || e->rid[im2] >= n0, ring[im1].y - ring[im2].y);
            if (pre_o == 0) continue;
            else if (pre_o * orientation < 0) continue;
            else if (orientation < 0) continue;
            else count += 1;
        } else {
            count += 1;
        }
    }
    return count % 2 != 0;
}

/* ---------------------------------------------------- quad validity (a9, a10) */

/* Mesh.is_valid(0), C:738-757 + segments_crossed C:814-826 */
static int quad_is_valid(const RefEnv *e, const P2 *m)
{
    if (is_cross(m[0], m[1], m[2], m[3])) return 0;
    if (is_cross(m[0], m[3], m[1], m[2])) return 0;
    for (int i = 0; i < 4; i++) {
        double degree = cw(m[i], m[(i + 1) % 4], m[(i + 3) % 4]);
        if (degree > e->max_degree || degree < e->min_degree) return 0;
    }
    return 1;
}

/* check_intersection_with_boundary, M:536-556.  mpos[k] = ring slot of quad vertex k (-1: not in ring),
 * r = position of the reference vertex inside the quad. */
static int intersects_boundary(const RefEnv *e, const P2 *m, const int *mpos, int r)
{
    const int n = e->n;
    const P2 *ring = e->ring;
    const P2 ref = m[r];
    double max_dist = -1;
    for (int k = 0; k < 4; k++)
        if (k != r) {
            double d = dist(ref, m[k]);
            if (d > max_dist) max_dist = d;
        }
    const P2 c0a = m[(r + 3) % 4], c0b = m[(r + 2) % 4]; /* (m[r-1], m[r-2]) */
    const P2 c1a = m[(r + 2) % 4], c1b = m[(r + 1) % 4]; /* (m[r-2], m[r-3]) */
#define IN_QUAD(slot) ((slot) == mpos[0] || (slot) == mpos[1] || (slot) == mpos[2] || (slot) == mpos[3])
    for (int i = 0; i < n; i++) {
        if (IN_QUAD(i)) continue;
        if (!(dist(ref, ring[i]) < max_dist)) continue;
        const int ip = RI(i - 1, n), in = (i + 1) % n;
        for (int c = 0; c < 2; c++) {
            const P2 ca = c ? c1a : c0a, cb = c ? c1b : c0b;
            if (!IN_QUAD(ip) && is_cross(ca, cb, ring[i], ring[ip])) return 1;
            if (!IN_QUAD(in) && is_cross(ca, cb, ring[i], ring[in])) return 1;
        }
    }
#undef IN_QUAD
    return 0;
}

/* ------------------------------------------------------------- reward (a12) */

/* Mesh.compute_area, C:943-958 */
static double quad_area(const P2 *m)
{
    double e0 = dist(m[0], m[3]), e1 = dist(m[1], m[0]), e2 = dist(m[2], m[1]), e3 = dist(m[3], m[2]);
    double c1 = cw(m[0], m[1], m[3]);
    double c3 = cw(m[2], m[3], m[1]);
    return 0.5 * e0 * e1 * sin(c1) + 0.5 * e2 * e3 * sin(c3);
}

/* Mesh.get_quality('robust'), C:881-892 */
static double quad_robust(const P2 *m)
{
    /* Python's min() / max() of a list start from its first entry (a NaN there stays, a later one is passed over) */
    double mn = 0;
    for (int i = 0; i < 4; i++) {
        double l = dist(m[(i + 3) % 4], m[i]);
        if (i == 0 || l < mn) mn = l;
    }
    double d0 = dist(m[0], m[2]), d1 = dist(m[1], m[3]);
    double q1 = sqrt(2.0) * mn / (d1 > d0 ? d1 : d0);
    double amin = 0, amax = 0;
    for (int i = 0; i < 4; i++) {
        double a = cw(m[i], m[(i + 1) % 4], m[(i + 3) % 4]);
        if (i == 0 || a < amin) amin = a;
        if (i == 0 || a > amax) amax = a;
    }
    double q2 = amin / amax;
    return sqrt(q1 * q2);
}

/* Segment.distance(Vertex), C:678-692; segment = (p1, p2) */
static double seg_point_distance(P2 p1, P2 p2, P2 v)
{
    double a = p1.x, b = p1.y;
    double A = p2.x - p1.x, B = p2.y - p1.y;
    double s = (A * v.x + B * v.y - B * b - A * a) / (SQ(A) + SQ(B));
    if (0 <= s && s <= 1) {
        P2 t = {a + s * A, b + s * B};
        return dist(v, t);
    } else if (s < 0) {
        return dist(v, p1);
    }
    return dist(v, p2);
}

/* compute_boundary_quality(add_v), M:355-408; index = ring slot of the new vertex */
static double boundary_quality_new(const RefEnv *e, int index)
{
    const int n = e->n;
    const P2 *ring = e->ring;
    const P2 add_v = ring[index];
    double amin = INFINITY;
    int have = 0;
    for (int t = 0; t < 2; t++) {
        int i = t == 0 ? 1 : -1;
        int c = RI(index + i, n);
        double angle = cw(ring[c], ring[RI(index + i + 1, n)], ring[RI(index + i - 1, n)]);
        if (angle < PI / 3) {
            if (angle < amin) amin = angle;
            have = 1;
        }
    }
    double q1 = have ? 3 * amin / PI : 1;

    const int w0 = index, w1 = (index + 1) % n, w2 = (index + 2) % n, w3 = RI(index - 1, n), w4 = RI(index - 2, n);
    double dst = dist(add_v, ring[w1]) + dist(add_v, ring[w3]);
    double m_d = INFINITY;
    int have_d = 0, prev_added = 0; /* `i - 1 in close_vs` */
    for (int i = 0; i < n; i++) {
        int added = 0;
        if (!(i == w0 || i == w1 || i == w2 || i == w3 || i == w4)) {
            if (dist(add_v, ring[i]) < dst) {
                if (!prev_added) {
                    added = 1;
                    double d = seg_point_distance(ring[(i + 1) % n], ring[i], add_v);
                    if (d < m_d) m_d = d;
                    have_d = 1;
                }
            }
        }
        prev_added = added;
    }
    double targt_len = dst / 2;
    double sum = 0;
    for (int i = 0; i < 4; i++) sum += dist(ring[RI(index - 2 + i, n)], ring[RI(index - 1 + i, n)]);
    double mean_dist = sum / 4;
    double smoothness = (targt_len < mean_dist ? targt_len : mean_dist) / (targt_len > mean_dist ? targt_len : mean_dist);
    double q2 = 1;
    if (have_d) q2 = (m_d < 0.5 * dst) ? m_d / (0.5 * dst) : 1;
    return pow(smoothness * q1 * q2, 1.0 / 3);
}

/* compute_ele_boundary_quality else-branch, M:418-452; t0/t1 = ring slots of the two kept quad
 * vertices in quad order */
static double boundary_quality_kept(const RefEnv *e, int t0, int t1)
{
    const int n = e->n;
    const P2 *ring = e->ring;
    double amin = INFINITY;
    int have = 0;
    int ts[2] = {t0, t1};
    for (int k = 0; k < 2; k++) {
        int index = ts[k];
        double angle = cw(ring[index], ring[(index + 1) % n], ring[RI(index - 1, n)]);
        if (angle < PI / 3) {
            if (angle < amin) amin = angle;
            have = 1;
        }
    }
    int index = t0 < t1 ? t0 : t1;
    double targt_len = dist(ring[t0], ring[t1]);
    double sum = 0;
    for (int i = 0; i < 5; i++) sum += dist(ring[RI(index - 2 + i, n)], ring[RI(index - 1 + i, n)]);
    double mean_dist = sum / 5;
    double smoothness = (targt_len < mean_dist ? targt_len : mean_dist) / (targt_len > mean_dist ? targt_len : mean_dist);
    double angle_quality = have ? 3 * amin / PI : 1;
    return pow(angle_quality * smoothness, 0.5);
}

/* get_speed_penalty, B:451-467 */
static double speed_penalty(const RefEnv *e, double mesh_area)
{
    double min_area = SQ(e->min_l), critical_area = SQ(e->crit_l);
    if (min_area <= mesh_area && mesh_area < critical_area) return (mesh_area - critical_area) / (critical_area - min_area);
    if (mesh_area < min_area) return -1;
    return 0;
}

/* ------------------------------------------------------------- ring edits */

static void ring_delete(RefEnv *e, int pos)
{
    int n = e->n;
    memmove(e->ring + pos, e->ring + pos + 1, (size_t)(n - pos - 1) * sizeof(P2));
    memmove(e->rid + pos, e->rid + pos + 1, (size_t)(n - pos - 1) * sizeof(int32_t));
    memmove(e->cand + pos, e->cand + pos + 1, (size_t)(n - pos - 1));
    memmove(e->key + pos, e->key + pos + 1, (size_t)(n - pos - 1) * sizeof(double));
    memmove(e->stamp + pos, e->stamp + pos + 1, (size_t)(n - pos - 1) * sizeof(int64_t));
    e->n = n - 1;
}

static int ring_find(const RefEnv *e, int32_t gid)
{
    for (int i = 0; i < e->n; i++)
        if (e->rid[i] == gid) return i;
    return -1;
}

static void log_quad(RefEnv *e, const int32_t *ids)
{
    if (e->n_elem < e->cap_e) memcpy(e->quads + 4 * e->n_elem, ids, 4 * sizeof(int32_t));
    e->n_elem += 1;
}

/* generated_meshes.append (B:209) + update_boundary (M:601-669) + the candidate list patch, shared by step() and move().
 * Returns the boundary-quality term of the reward (computed on the post-update ring) when want_reward, else 0. */
static double extract_element(RefEnv *e, const P2 *m, const int *mpos, int new_vertex, int index, P2 new_point,
                              int want_reward)
{
    const int n = e->n;
    (void)m;
    int32_t qids[4];
    for (int k = 0; k < 4; k++) qids[k] = mpos[k] < 0 ? e->n_vert : e->rid[mpos[k]];
    log_quad(e, qids); /* generated_meshes.append, B:209 */

    /* update_boundary, M:601-669 */
    double b_reward = 0.0;
    if (new_vertex) {
        const int id = index;
        e->ring[id] = new_point;
        e->rid[id] = e->n_vert;
        e->cand[id] = 0;
        if (e->n_vert < e->cap_v) e->vtab[e->n_vert] = new_point;
        e->n_vert += 1;
        int pos[4] = {(id + 1) % n, RI(id - 1, n), (id + 2) % n, RI(id - 2, n)};
        for (int k = 0; k < 4; k++) e->cand[pos[k]] = 0;
        for (int k = 0; k < 4; k++) add_candidate(e, pos[k]);
        if (want_reward) b_reward = boundary_quality_new(e, id);
    } else {
        int32_t keep0 = e->rid[mpos[0]], keep1 = e->rid[mpos[3]];
        int32_t rem0 = e->rid[mpos[1]], rem1 = e->rid[mpos[2]];
        ring_delete(e, ring_find(e, rem0));
        ring_delete(e, ring_find(e, rem1));
        const int nn = e->n;
        int t0 = ring_find(e, keep0), t1 = ring_find(e, keep1);
        int id = t0 > t1 ? t0 : t1;
        int pos[4] = {id % nn, RI(id - 1, nn), (id + 1) % nn, RI(id - 2, nn)};
        for (int k = 0; k < 4; k++) e->cand[pos[k]] = 0;
        for (int k = 0; k < 4; k++) add_candidate(e, pos[k]);
        if (want_reward) b_reward = boundary_quality_kept(e, t0, t1);
    }
    return b_reward;
}

/* ---------------------------------------------------------------- API */

RefEnv *meshenv_ref_create(int n0, const double *xy, double original_area, double est_min_l,
                           double est_crit_l, int cap_new)
{
    RefEnv *e = (RefEnv *)calloc(1, sizeof(RefEnv));
    e->n0 = n0;
    e->ring = (P2 *)malloc(sizeof(P2) * n0);
    e->ring0 = (P2 *)malloc(sizeof(P2) * n0);
    e->rid = (int32_t *)malloc(sizeof(int32_t) * n0);
    e->cand = (uint8_t *)malloc(n0);
    e->key = (double *)malloc(sizeof(double) * n0);
    e->stamp = (int64_t *)malloc(sizeof(int64_t) * n0);
    e->nv = (P2 *)malloc(sizeof(P2) * (size_t)(n0 + 8));
    e->nv_id = (int32_t *)malloc(sizeof(int32_t) * (size_t)(n0 + 8));
    e->n_nv = 0;
    e->last_count = 0;
    e->epoch = 0;
    for (int i = 0; i < n0; i++) {
        e->ring0[i].x = xy[2 * i];
        e->ring0[i].y = xy[2 * i + 1];
    }
    e->orig_area = original_area;
    e->min_l = est_min_l;
    e->crit_l = est_crit_l;
    e->cap_v = n0 + cap_new;
    e->cap_e = cap_new + n0;
    e->vtab = (P2 *)malloc(sizeof(P2) * e->cap_v);
    e->quads = (int32_t *)malloc(sizeof(int32_t) * 4 * e->cap_e);
    /* the reference's literals: B:52, M:26, M:213, C:722, C:721, B:601, M:540 */
    const double def[7] = {4, PI * 0.972, 0.618, 0.01 * PI, 0.99 * PI, 0.001, 10000};
    meshenv_ref_set_params(e, def);
    return e;
}

void meshenv_ref_set_params(RefEnv *e, const double *p)
{
    e->radius = p[0];
    e->max_ref_angle = p[1];
    e->key_lambda = p[2];
    e->min_degree = p[3];
    e->max_degree = p[4];
    e->same_point_eps = p[5];
    e->ray_length = p[6];
    float obs[18];
    meshenv_ref_reset(e, obs);
}

void meshenv_ref_destroy(RefEnv *e)
{
    if (!e) return;
    free(e->ring); free(e->ring0); free(e->rid); free(e->cand); free(e->key); free(e->stamp);
    free(e->vtab); free(e->quads); free(e->nv); free(e->nv_id); free(e);
}

/* B:84-101 */
int meshenv_ref_reset(RefEnv *e, float *obs) { return meshenv_ref_reset_static(e, obs, 0); }

int meshenv_ref_reset_static(RefEnv *e, float *obs, int is_static)
{
    e->n = e->n0;
    for (int i = 0; i < e->n0; i++) {
        e->ring[i] = e->ring0[i];
        e->vtab[i] = e->ring0[i];
        e->rid[i] = i;
    }
    e->n_vert = e->n0;
    e->n_elem = 0;
    e->failed = 0;
    e->cur_area = e->orig_area;
    e->n_nv = 0; /* self.not_valid_points = [], B:90 */
    e->epoch += 1;
    find_reference_candidates(e);
    return find_next_state_opt(e, obs, is_static, 0);
}

/* B:130-280 */
int meshenv_ref_step(RefEnv *e, const float *action, float *obs, double *reward_out, uint8_t *done_out,
                     uint8_t *complete_out)
{
    int done = 0, failed = 1, no_reference = 0;
    double reward = 0;
    const float rule_type = action[0];

    /* action_2_point -> detransformation, B:633-642, B:115-123, D:112-137.
     * p0 = neighbors[3] = ref, p1 = neighbors[4] = ring[ref-1] of the last observation. */
    P2 new_point = {0, 0};
    const int index = e->ref;
    if (index >= 0) {
        const int n = e->n;
        const double px = (double)round4_npf(action[1]);
        const double py = (double)round4_npf(action[2]);
        const P2 p0 = e->ring[index], p1 = e->ring[RI(index - 1, n)];
        const double theta = 2 * PI - atan2(p1.y - p0.y, p1.x - p0.x);
        double ox = cos(theta) * px + sin(theta) * py;
        double oy = -sin(theta) * px + cos(theta) * py;
        ox *= e->bl;
        oy *= e->bl;
        ox += p0.x;
        oy += p0.y;
        new_point.x = round4_np(ox);
        new_point.y = round4_np(oy);
    }

    if (index < 0) {
        /* the reference's find_next_state returned None and this step() would raise; the documented replacement
         * behaviour (include/meshenv.h, MESHENV_ST_NO_REFERENCE) is: reward -1, episode ends as truncated */
        reward = -1;
        done = 1;
        no_reference = 1;
    } else if (e->n <= 5) {
        reward = 10; /* B:158-160 */
        done = 1;
    } else {
        const int n = e->n;
        P2 m[4];
        int mpos[4];
        int have_mesh = 1, rule, r, new_vertex = 0;
        if (rule_type <= -0.5f) {
            rule = -1;
        } else if (rule_type >= 0.5f) {
            rule = 1;
        } else {
            rule = 0;
            if (is_point_inside_area(e, new_point)) {
                int same = -1; /* find_same_point, B:616-619 */
                for (int i = 0; i < n; i++)
                    if (dist(e->ring[i], new_point) < e->same_point_eps) {
                        same = i;
                        break;
                    }
                if (same >= 0) rule = -1; /* existing point: the rule -1 quad, B:185-192 */
                else new_vertex = 1;
            } else {
                reward += e->n_elem ? -1.0 / e->n_elem : -1;
                have_mesh = 0;
            }
        }
        if (have_mesh) {
            if (new_vertex) { /* [new, i-1, i, i+1], B:194-199 */
                mpos[0] = -1; mpos[1] = RI(index - 1, n); mpos[2] = index; mpos[3] = (index + 1) % n;
                r = 2;
            } else if (rule == -1) { /* [i-1, i, i+1, i+2], B:164-170 */
                mpos[0] = RI(index - 1, n); mpos[1] = index; mpos[2] = (index + 1) % n; mpos[3] = (index + 2) % n;
                r = 1;
            } else { /* [i-2, i-1, i, i+1], B:173-179 */
                mpos[0] = RI(index - 2, n); mpos[1] = RI(index - 1, n); mpos[2] = index; mpos[3] = (index + 1) % n;
                r = 2;
            }
            for (int k = 0; k < 4; k++) m[k] = mpos[k] < 0 ? new_point : e->ring[mpos[k]];

            if (quad_is_valid(e, m) && !intersects_boundary(e, m, mpos, r)) {
                const double b_reward = extract_element(e, m, mpos, new_vertex, index, new_point, 1);
                const double mesh_area = quad_area(m);
                e->cur_area -= mesh_area;
                /* get_quality(mesh, 2), M:1759-1766 */
                const double e_reward = quad_robust(m);
                const double quality = e_reward + 1 * (b_reward - 1);
                reward += quality + speed_penalty(e, mesh_area);
                failed = 0;
                if (e->n <= 5) { /* B:249-261 */
                    reward += 10;
                    done = 1;
                    if (e->n == 4) log_quad(e, e->rid);
                }
            } else {
                reward += e->n_elem ? -1.0 / e->n_elem : -1; /* B:265 */
            }
        }
    }
    int is_complete = no_reference ? 0 : 1;
    int none = find_next_state_opt(e, obs, 0, 1); /* B:267: find_next_state(self.not_valid_points, ...) */
    if (!failed) {
        e->failed = 0;
    } else {
        e->failed += 1;
        if (e->failed >= 100) {
            done = 1;
            is_complete = 0;
        }
    }
    *reward_out = reward;
    *done_out = (uint8_t)done;
    *complete_out = (uint8_t)is_complete;
    return none;
}


/* round(python_float, 6): correctly-rounded decimal rounding, as round4_py with scale 1e6 */
static double round6_py(double x)
{
    if (!isfinite(x)) return x;
    double ax = fabs(x);
    double y = ax * 1e6;
    if (y >= 4503599627370496.0) return x;
    double er = fma(ax, 1e6, -y); /* exact: ax*1e6 == y + er */
    double f = floor(y);
    double t = (y - f) - 0.5;
    double s = t + er;
    double r;
    if (s > 0) r = f + 1;
    else if (s < 0) r = f;
    else r = (fmod(f, 2.0) == 0.0) ? f : f + 1;
    return copysign(r / 1e6, x);
}

/* move(new_point, type), B:282-449, for Python-float arguments: new_point = (radius fraction, angle), `type` the rule
 * selector with TYPE_THRESHOLD = 0.3 (B:19).  No reward (the reference returns 0), no current_area / failed_num
 * bookkeeping; rejected reference vertices accumulate in not_valid_points and are skipped by the next selection; the
 * observation is the static one.
 * Returns MESHENV_REF_MOVE_*: OK, NONE (obs is None; only possible with ring <= 4 here), RAISES (ring <= 5 on entry:
 * the reference leaves `is_complete` unbound and raises UnboundLocalError; nothing is changed).  When no reference vertex is
 * left while the ring has more than 4 vertices the reference runs smooth_pave (front + interior smoothing, candidate
 * rebuild; B:405-412), ends the episode if not_valid_points repeats the list of the previous smoothing (B:416-420;
 * last_not_valid_points survives reset()), empties the list and selects again (B:422-426): done here as well;
 * SMOOTH_RAISES where the reference raises inside smooth_pave, NEEDS_SMOOTHING only if the element log overflowed. */
int meshenv_ref_move(RefEnv *e, const double *point, double type, float *obs, uint8_t *done_out, uint8_t *complete_out)
{
    if (e->n <= 5 || e->ref < 0) return MESHENV_REF_MOVE_RAISES;
    const int n = e->n, index = e->ref;
    /* B:283-287 */
    const double x = ((e->bl * e->radius) * point[0]) * cos(point[1]);
    const double y = ((e->bl * e->radius) * point[0]) * sin(point[1]);
    const double px = round6_py(x), py = round6_py(y);
    const P2 p0 = e->ring[index], p1 = e->ring[RI(index - 1, n)];
    const double theta = 2 * PI - atan2(p1.y - p0.y, p1.x - p0.x);
    double ox = cos(theta) * px + sin(theta) * py;
    double oy = -sin(theta) * px + cos(theta) * py;
    ox *= 1; /* is_move: the scale is 1, B:122 */
    oy *= 1;
    ox += p0.x;
    oy += p0.y;
    const P2 new_point = {round4_np(ox), round4_np(oy)};

    int done = 0, not_valid = 1, none = 0;
    const P2 reference_point = e->ring[index];
    P2 m[4];
    int mpos[4], have_mesh = 1, r = 2, new_vertex = 0;
    if (type <= 0.3) { /* B:303-310 */
        mpos[0] = RI(index - 1, n); mpos[1] = index; mpos[2] = (index + 1) % n; mpos[3] = (index + 2) % n;
        r = 1;
    } else if (type >= 1 - 0.3) { /* B:312-319 */
        mpos[0] = RI(index - 2, n); mpos[1] = RI(index - 1, n); mpos[2] = index; mpos[3] = (index + 1) % n;
    } else if (is_point_inside_area(e, new_point)) { /* B:320-326: no find_same_point here */
        mpos[0] = -1; mpos[1] = RI(index - 1, n); mpos[2] = index; mpos[3] = (index + 1) % n;
        new_vertex = 1;
    } else {
        have_mesh = 0;
    }
    if (have_mesh) {
        for (int k = 0; k < 4; k++) m[k] = mpos[k] < 0 ? new_point : e->ring[mpos[k]];
        if (quad_is_valid(e, m) && !intersects_boundary(e, m, mpos, r)) {
            not_valid = 0;
            extract_element(e, m, mpos, new_vertex, index, new_point, 0);
            none = find_next_state_opt(e, obs, 1, 1); /* B:362, still with the old not_valid_points */
            if (e->n <= 5) { /* B:364-368 */
                done = 1;
                if (e->n == 4) log_quad(e, e->rid);
            }
        }
    }
    if (not_valid) { /* B:375-378; `reference_point not in list` is object identity (Vertex has no __eq__): compare ids --
                      * a coincident twin of a listed vertex is another object and is appended as well */
        int listed = 0;
        for (int k = 0; k < e->n_nv; k++)
            if (e->nv_id[k] == e->rid[index]) listed = 1;
        if (!listed) {
            e->nv[e->n_nv] = reference_point;
            e->nv_id[e->n_nv++] = e->rid[index];
        }
        none = find_next_state_opt(e, obs, 1, 1);
    } else {
        e->n_nv = 0; /* B:382 */
    }
    int is_complete, rc = none ? MESHENV_REF_MOVE_NONE : MESHENV_REF_MOVE_OK;
    if (e->n > 4) {
        is_complete = 0;
        if (none) { /* B:405-426: smooth_pave, then a fresh selection with an empty not_valid_points */
            int32_t sweeps = 0;
            int src = meshenv_ref_smooth_front(e);
            if (src == -4) { /* a NaN vertex was accepted: B:416-422 run, then find_next_state raises (C:1257) */
                e->last_count = e->n_nv;
                if (e->n_nv > 0) { e->last_first = e->nv_id[0]; e->last_last = e->nv_id[e->n_nv - 1]; }
                e->last_epoch = e->epoch;
                e->n_nv = 0;
                src = -3;
            }
            if (src == -3) { *done_out = 1; *complete_out = 0; return MESHENV_REF_MOVE_SMOOTH_RAISES; } /* the caller resets */
            if (src == 0) src = meshenv_ref_smooth_interior(e, 400, &sweeps, NULL);
            if (src != 0) { /* log overflow: the graph cannot be rebuilt -- the episode ends here (not a reference path) */
                *done_out = 1; *complete_out = 0;
                return MESHENV_REF_MOVE_NEEDS_SMOOTHING;
            }
            if (e->last_count > 0 && e->n_nv > 0) {
                const int32_t f = e->nv_id[0], l = e->nv_id[e->n_nv - 1];
                /* reset() deep-copies the domain (B:69): every vertex of an earlier episode is a different object */
                const int same_episode = e->last_epoch == e->epoch;
                if (same_episode && f == e->last_first && l == e->last_last && e->n_nv == e->last_count) done = 1;
            }
            e->last_count = e->n_nv;
            if (e->n_nv > 0) { e->last_first = e->nv_id[0]; e->last_last = e->nv_id[e->n_nv - 1]; }
            e->last_epoch = e->epoch;
            e->n_nv = 0;
            none = find_next_state_opt(e, obs, 1, 1);
            if (none) done = 1;
            rc = none ? MESHENV_REF_MOVE_NONE : MESHENV_REF_MOVE_OK;
        }
    } else {
        is_complete = 1;
    }
    *done_out = (uint8_t)done;
    *complete_out = (uint8_t)is_complete;
    return rc;
}

/* ------------------------------------------------- smoothing: smooth_pave(..., interior=True)
 *
 * general/mesh.py:790-795 with interior=True: smooth_fixed_vertices (M:1258-1288) over the vertices of boundary.vertices
 * that are not on the current front, then find_reference_candidates(target_angle=0).  The reference walks the
 * Vertex.segments graph; here the graph is rebuilt from the element log:
 *   - only generated vertices move (`if vertex in self.original_vertices: continue`), and a generated vertex receives
 *     segments only from Mesh.connect_vertices (C:832-837) of the elements that contain it: for i = 0..3 the pair
 *     (vertices[i], vertices[i-1]) gets a new Segment unless one exists already, appended to both ends' lists;
 *   - get_connected_vertices (C:115-124) lists the other end of every segment in list order, so the neighbours of a
 *     generated vertex are the partners of those pairs in element order, first occurrence only.
 * The sweep is Gauss-Seidel in boundary.vertices order (domain ring first, generated vertices in creation order): every
 * vertex sees the new position of its predecessors; x accumulates (neighbour.x + vertex.x) term by term from an int 0;
 * the stop rule compares the running sum of the moved vertices' x + y with the previous sweep's (<= 0.001) or stops
 * after `iteration` sweeps.  Returns 0, or -1 when the element / vertex log overflowed (graph incomplete) or a vertex
 * has more than MESHENV_REF_MAX_DEG neighbours. */
#define MESHENV_REF_MAX_DEG 16
int meshenv_ref_smooth_interior(RefEnv *e, int iteration, int32_t *sweeps_out, double *diff_out)
{
    if (e->n_elem > e->cap_e || e->n_vert > e->cap_v) return -1;
    const int nv = e->n_vert, n_new = nv - e->n0;
    int32_t *adj = (int32_t *)malloc(sizeof(int32_t) * (size_t)(n_new > 0 ? n_new : 1) * MESHENV_REF_MAX_DEG);
    int32_t *deg = (int32_t *)calloc((size_t)(n_new > 0 ? n_new : 1), sizeof(int32_t));
    uint8_t *on_front = (uint8_t *)calloc((size_t)nv, 1);
    int rc = 0;
    for (int k = 0; k < e->n_elem && rc == 0; k++) {
        const int32_t *q = e->quads + 4 * k;
        for (int i = 0; i < 4 && rc == 0; i++) {
            const int32_t a = q[i], b = q[(i + 3) & 3];
            /* has_segment_with_vertex is symmetric (a segment sits in both ends' lists): test on a generated end */
            const int32_t g = a >= e->n0 ? a : b, o = a >= e->n0 ? b : a;
            if (g < e->n0) continue; /* two domain vertices: their lists are never read */
            int found = 0;
            for (int j = 0; j < deg[g - e->n0]; j++) found |= adj[(g - e->n0) * MESHENV_REF_MAX_DEG + j] == o;
            if (found) continue;
            const int32_t ends[2] = {a, b};
            for (int s = 0; s < 2; s++) {
                const int32_t v = ends[s], w = ends[1 - s];
                if (v < e->n0) continue;
                if (deg[v - e->n0] >= MESHENV_REF_MAX_DEG) { rc = -1; break; }
                adj[(v - e->n0) * MESHENV_REF_MAX_DEG + deg[v - e->n0]++] = w;
            }
        }
    }
    for (int i = 0; i < e->n; i++) on_front[e->rid[i]] = 1;
    double sum_coordinates = 0.0, diffs = 100.0;
    int it = 0;
    while (rc == 0 && diffs > 0.001 && it < iteration) {
        it += 1;
        double new_sum = 0.0;
        for (int v = e->n0; v < nv; v++) {
            if (on_front[v]) continue;
            const int d = deg[v - e->n0];
            if (d == 0) continue;
            double x = 0.0, y = 0.0;
            for (int j = 0; j < d; j++) {
                const P2 c = e->vtab[adj[(v - e->n0) * MESHENV_REF_MAX_DEG + j]];
                x += c.x + e->vtab[v].x;
                y += c.y + e->vtab[v].y;
            }
            e->vtab[v].x = x / (double)(2 * d);
            e->vtab[v].y = y / (double)(2 * d);
            new_sum += e->vtab[v].x + e->vtab[v].y;
        }
        diffs = fabs(new_sum - sum_coordinates);
        sum_coordinates = new_sum;
    }
    free(adj); free(deg); free(on_front);
    if (rc != 0) return rc;
    find_reference_candidates(e); /* M:795; the point environment (reference vertex, observation) is left as it was */
    if (sweeps_out) *sweeps_out = it;
    if (diff_out) *diff_out = diffs;
    return 0;
}

/* ------------------------------------------------- smoothing of a finished mesh: MeshGeneration.smooth(vertices)
 *
 * general/mesh.py:1290-1392, the call general/EBRD.py:391 makes once the front is down to <= 5 vertices
 * (env.smooth(env.boundary.vertices), lr_1 = lr_2 = 0.999).  Every generated vertex, in boundary.vertices order, by the
 * number of elements that contain it (find_related_meshes, M:556-564):
 *   1 element : two neighbours -> the 4th-vertex estimate from their common neighbour (M:1307-1326); else a 0.999 pull
 *   2 elements: one interior + two front neighbours -> mean of two 4th-vertex estimates (M:1338-1361); else the pull
 *   otherwise : the Laplacian step of smooth_fixed_vertices
 * and the stop rule sums x + y over ALL of `vertices` (domain ring included), M:1384-1387.  Needs the Vertex.segments
 * lists of every vertex: the domain ring's own segments first (general/mesh.py:1926-1930: for i: Segment(v[i-1], v[i])
 * appended to v[i-1] and v[i]), then Mesh.connect_vertices of every element (C:832-837).
 * Returns 0; -1 log overflow / degree overflow; -2 where the reference would raise IndexError (M:1311 on an empty list). */
typedef struct {
    int32_t *adj, *deg;
} Graph;

static int graph_has(const Graph *g, int v, int w)
{
    for (int j = 0; j < g->deg[v]; j++)
        if (g->adj[v * MESHENV_REF_MAX_DEG + j] == w) return 1;
    return 0;
}

static int graph_add(Graph *g, int v, int w)
{
    if (g->deg[v] >= MESHENV_REF_MAX_DEG) return -1;
    g->adj[v * MESHENV_REF_MAX_DEG + g->deg[v]++] = w;
    return 0;
}

/* Mesh.estimate_4th_vertex, C:980-990 -> Segment.get_ray_segment / build_ray, C:588-610 */
static P2 estimate_4th_vertex(P2 origin, P2 left, P2 right, double factor, int has_suggest, double suggest_dist)
{
    double distance = (dist(origin, left) + dist(origin, right)) * factor;
    if (has_suggest) {
        double lim = 0.6 * suggest_dist;
        if (lim < distance) distance = lim; /* min(distance, 0.6 * suggest_dist) */
    }
    P2 r1 = {(origin.x + origin.x) / 2, (origin.y + origin.y) / 2};
    P2 r2 = {(left.x + right.x) / 2, (left.y + right.y) / 2};
    double theta = atan2(r2.y - r1.y, r2.x - r1.x);
    P2 out = {r1.x + distance * cos(theta), r1.y + distance * sin(theta)};
    return out;
}

/* Boundary2D.compute_dist(candidates, point)[0][0], C:369-376: the nearest candidate (stable sort: first among equals) */
static int nearest_of(const RefEnv *e, const int *cand, int n_cand, int point)
{
    int best = -1;
    double bd = 0.0;
    for (int j = 0; j < n_cand; j++) {
        if (cand[j] == point) continue;
        double d = dist(e->vtab[point], e->vtab[cand[j]]);
        if (best < 0 || d < bd) { best = cand[j]; bd = d; }
    }
    return best;
}

/* [v for v in a.get_connected_vertices() if v in b.get_connected_vertices()], C:162-165, minus `skip` */
static int common_vertices(const Graph *g, int a, int b, int skip, int *out)
{
    int m = 0;
    for (int j = 0; j < g->deg[a]; j++) {
        int v = g->adj[a * MESHENV_REF_MAX_DEG + j];
        if (v != skip && graph_has(g, b, v)) out[m++] = v;
    }
    return m;
}

int meshenv_ref_smooth_final(RefEnv *e, int iteration, double lr_1, double lr_2, int32_t *sweeps_out, double *diff_out,
                             int64_t *branch_out)
{
    if (e->n_elem > e->cap_e || e->n_vert > e->cap_v) return -1;
    const int nv = e->n_vert, n0 = e->n0;
    Graph g;
    g.adj = (int32_t *)malloc(sizeof(int32_t) * (size_t)nv * MESHENV_REF_MAX_DEG);
    g.deg = (int32_t *)calloc((size_t)nv, sizeof(int32_t));
    int32_t *nmesh = (int32_t *)calloc((size_t)nv, sizeof(int32_t));
    uint8_t *on_front = (uint8_t *)calloc((size_t)nv, 1);
    int rc = 0;
    for (int i = 0; i < n0 && rc == 0; i++) { /* the domain ring's segments */
        int a = (i + n0 - 1) % n0;
        rc |= graph_add(&g, a, i);
        rc |= graph_add(&g, i, a);
    }
    for (int k = 0; k < e->n_elem && rc == 0; k++) {
        const int32_t *q = e->quads + 4 * k;
        for (int i = 0; i < 4; i++) nmesh[q[i]] += 1;
        for (int i = 0; i < 4 && rc == 0; i++) {
            const int a = q[i], b = q[(i + 3) & 3];
            if (graph_has(&g, a, b)) continue;
            rc |= graph_add(&g, a, b);
            rc |= graph_add(&g, b, a);
        }
    }
    for (int i = 0; i < e->n; i++) on_front[e->rid[i]] = 1;
    int64_t br[3] = {0, 0, 0};
    double sum_coordinates = 0.0, diffs = 100.0;
    int it = 0;
    while (rc == 0 && diffs > 0.001 && it < iteration) {
        it += 1;
        for (int v = n0; v < nv && rc == 0; v++) {
            const int d = g.deg[v];
            const int32_t *cn = g.adj + v * MESHENV_REF_MAX_DEG;
            const int nm = nmesh[v];
            int pull = 0;
            br[nm == 1 ? 0 : (nm == 2 ? 1 : 2)] += 1;
            if (nm == 1) {
                if (d == 2) {
                    int com[MESHENV_REF_MAX_DEG];
                    int m = common_vertices(&g, cn[0], cn[1], v, com);
                    int origin = nearest_of(e, com, m, v);
                    if (origin < 0) { rc = -2; break; }
                    /* nearest front vertex to origin, not a neighbour of v and not v */
                    int best = -1;
                    double bd = 0.0;
                    for (int i = 0; i < e->n; i++) {
                        int w = e->rid[i];
                        if (w == cn[0] || w == cn[1] || w == v || w == origin) continue; /* compute_dist skips the point itself */
                        double dd = dist(e->vtab[origin], e->vtab[w]);
                        if (best < 0 || dd < bd) { best = w; bd = dd; }
                    }
                    if (best < 0) continue;
                    e->vtab[v] = estimate_4th_vertex(e->vtab[origin], e->vtab[cn[0]], e->vtab[cn[1]], 0.5, 1, bd);
                } else {
                    pull = 1;
                }
            } else if (nm == 2) {
                int ub[MESHENV_REF_MAX_DEG], in[MESHENV_REF_MAX_DEG], nu = 0, ni = 0;
                for (int j = 0; j < d; j++) {
                    if (on_front[cn[j]]) ub[nu++] = cn[j];
                    else in[ni++] = cn[j];
                }
                if (ni == 1 && nu == 2) {
                    int com[MESHENV_REF_MAX_DEG];
                    int m = common_vertices(&g, in[0], ub[0], v, com);
                    int c1 = nearest_of(e, com, m, v);
                    m = common_vertices(&g, in[0], ub[1], v, com);
                    int c2 = nearest_of(e, com, m, v);
                    if (c1 < 0 || c2 < 0) { rc = -2; break; }
                    P2 e1 = estimate_4th_vertex(e->vtab[c1], e->vtab[ub[0]], e->vtab[in[0]], 0.7, 0, 0.0);
                    P2 e2 = estimate_4th_vertex(e->vtab[c2], e->vtab[ub[1]], e->vtab[in[0]], 0.7, 0, 0.0);
                    e->vtab[v].x = (e1.x + e2.x) / 2;
                    e->vtab[v].y = (e1.y + e2.y) / 2;
                } else {
                    pull = 1;
                }
            } else {
                if (d == 0) continue;
                double x = 0.0, y = 0.0;
                for (int j = 0; j < d; j++) {
                    x += e->vtab[cn[j]].x + e->vtab[v].x;
                    y += e->vtab[cn[j]].y + e->vtab[v].y;
                }
                e->vtab[v].x = x / (double)(2 * d);
                e->vtab[v].y = y / (double)(2 * d);
            }
            if (pull) {
                const double lr = nm == 1 ? lr_1 : lr_2;
                for (int j = 0; j < d; j++) {
                    e->vtab[v].x = lr * e->vtab[v].x + (1 - lr) * e->vtab[cn[j]].x;
                    e->vtab[v].y = lr * e->vtab[v].y + (1 - lr) * e->vtab[cn[j]].y;
                }
            }
        }
        double new_sum = 0.0;
        for (int v = 0; v < nv; v++) new_sum += e->vtab[v].x + e->vtab[v].y;
        diffs = fabs(new_sum - sum_coordinates);
        sum_coordinates = new_sum;
    }
    free(g.adj); free(g.deg); free(nmesh); free(on_front);
    if (rc != 0) return rc;
    /* front vertices may have moved: the ring holds copies */
    for (int i = 0; i < e->n; i++) e->ring[i] = e->vtab[e->rid[i]];
    find_reference_candidates(e); /* M:1392 */
    if (sweeps_out) *sweeps_out = it;
    if (diff_out) *diff_out = diffs;
    if (branch_out) { branch_out[0] = br[0]; branch_out[1] = br[1]; branch_out[2] = br[2]; }
    return 0;
}

/* ------------------------------------------------- the front smoother: smooth_current_boundary_3, M:939-1028
 *
 * smooth_pave(..., interior=False) (M:790-795) runs it before smooth_fixed_vertices; move() enters smooth_pave when no
 * reference vertex is selectable (B:405-412).  Every generated vertex ON the front, in ring order and in place, by its
 * interior angle: <= 90 -> middle_vertex on the bisector for a target angle raised in steps of 5 until the new position
 * keeps every surrounding element on its side (is_inside_boundary over clockwise_vertices); (90, 180] -> side_vertex
 * next to a sharp (< 45) neighbour corner, else find_indention_vertex; (180, 270] -> find_indention_vertex; beyond ->
 * inner_vertex then find_indention_vertex.  Returns 0, -1 (log / degree overflow), -3 where a vertex construction
 * raises in the reference: the vertices moved before that stay moved.
 *
 * What raises (checked against the reference run side by side, oracle/check_move_vs_reference.py): math.sqrt of a
 * negative number or of -inf (ValueError; math.sqrt(nan) returns nan) -- and a zero divisor ONLY when both operands are
 * Python numbers.  Coordinates of domain vertices are Python floats / ints, coordinates of generated vertices are
 * np.float64 (B:123 rounds a NumPy array element; the same provenance rule as round4_by above: id >= n0 <=> NumPy), and
 * `python_float / np.float64(0.0)` is NumPy's division: a RuntimeWarning and inf / nan, execution continues.  The zero
 * divisors of this code are coordinate differences of two coincident vertices (A == 0 and B == 0 at once), where the
 * numerator W = dist * |p - q| * cos(..) is 0 as well, so the quotient is nan, every comparison on the candidate
 * position is False, is_inside_boundary rejects it for every trial and the vertex stays where it is (M:1048-1066) --
 * unless every entry of the surrounding polygon already reads >= pi for the original position, in which case the
 * reference assigns nan coordinates and goes on; that continuation (a NaN vertex in the front, int(nan) raising in the
 * next get_radius_points: ValueError, C:1257) is not restated step by step: a non-finite accepted position ends the
 * front smoother with -4, which move() turns into what the reference does next -- B:416-422 (the not_valid_points
 * bookkeeping) and then the raise out of find_next_state: the same return as -3, with the list already cleared
 * (tests/golden/move_rand7023_c1.npz, move 996). */
typedef struct {
    RefEnv *e;
    Graph g;
    int raised;
} Front;

static double py_sqrt(Front *f, double v)
{
    if (v < 0) { f->raised = 1; return 0.0; } /* ValueError: math domain error (nan passes: math.sqrt(nan) = nan) */
    return sqrt(v);
}

/* a / b where the divisor's type follows its operands: is_np != 0 -> NumPy scalar division (IEEE: inf / nan, a warning) */
static double py_div(Front *f, double a, double b, int is_np)
{
    if (b == 0 && !is_np) { f->raised = 1; return 0.0; } /* ZeroDivisionError */
    return a / b;
}

static double deg2rad(double a) { return a * (PI / 180.0); } /* math.radians */
static double rad2deg(double a) { return a * (180.0 / PI); } /* math.degrees */

/* the two intersections of the circle |p - (a, b)| = dist with the line A x + B y = W + A a + B b, M:841-858 / 889-904 */
static void circle_line(Front *f, double a, double b, double A, double B, double W, double dist, int np_A, P2 *v1, P2 *v2)
{
    if (B == 0) {
        double wa = py_div(f, W, A, np_A); /* W is a Python float (math.sqrt / math.cos products) */
        double r = py_sqrt(f, SQ(dist) - SQ(wa));
        v1->x = wa + a; v2->x = wa + a;
        v1->y = b + r; v2->y = b - r;
    } else if (A == 0) {
        double wb = W / B;
        double r = py_sqrt(f, SQ(dist) - SQ(wb));
        v1->x = a + r; v2->x = a - r;
        v1->y = wb + b; v2->y = wb + b;
    } else {
        double M = -A / B;
        double N = (W + A * a + B * b) / B;
        double t = 2 * M * b - 2 * M * N + 2 * a;
        double disc = fabs(SQ(t) - 4 * (SQ(M) + 1) * (SQ(N - b) + SQ(a) - SQ(dist)));
        double den = 2 * (SQ(M) + 1);
        v1->x = (t + sqrt(disc)) / den;
        v2->x = (t - sqrt(disc)) / den;
        v1->y = M * v1->x + N;
        v2->y = M * v2->x + N;
    }
}

/* M:805-832 */
static P2 middle_vertex(Front *f, P2 vertex, P2 left, P2 right, double target_angle)
{
    P2 m = {(left.x + right.x) / 2, (left.y + right.y) / 2};
    double A = right.x - left.x, B = right.y - left.y;
    double D = dist(left, m) / tan(deg2rad(target_angle / 2));
    P2 v1, v2;
    if (B == 0) {
        v1.x = m.x; v2.x = m.x; v1.y = m.y + D; v2.y = m.y - D;
    } else if (A == 0) {
        v1.x = m.x + D; v2.x = m.x - D; v1.y = m.y; v2.y = m.y;
    } else {
        double M = -A / B;
        double N = A * m.x / B + m.y;
        double t = -2 * M * N + 2 * m.x + 2 * M * m.y;
        double disc = fabs(SQ(t) - 4 * (SQ(M) + 1) * (SQ(N - m.y) + SQ(m.x) - SQ(D)));
        double den = 2 * (SQ(M) + 1);
        v1.x = (t + sqrt(disc)) / den;
        v2.x = (t - sqrt(disc)) / den;
        v1.y = M * v1.x + N;
        v2.y = M * v2.x + N;
    }
    (void)f;
    return dist(v1, vertex) < dist(v2, vertex) ? v1 : v2;
}

/* M:834-863 */
static P2 side_vertex(Front *f, P2 vertex, P2 next_v, P2 nn_v, double angle, double d, int np_A)
{
    double W = d * dist(next_v, nn_v) * cos(deg2rad(angle));
    P2 v1, v2;
    circle_line(f, next_v.x, next_v.y, nn_v.x - next_v.x, nn_v.y - next_v.y, W, d, np_A, &v1, &v2);
    return dist(v1, vertex) < dist(v2, vertex) ? v1 : v2;
}

/* M:882-909 */
static P2 indention_vertex(Front *f, P2 vertex, P2 left, P2 right, double angle, double d, int np_A)
{
    double W = d * dist(vertex, left) * cos(deg2rad(angle));
    P2 v1, v2;
    circle_line(f, vertex.x, vertex.y, left.x - vertex.x, left.y - vertex.y, W, d, np_A, &v1, &v2);
    return cw(v1, left, right) < cw(v2, left, right) ? v1 : v2;
}

/* clockwise_vertices, M:1080-1101: the neighbours of `inner` sorted by clockwise angle (selection sort as written), each
 * followed by the common neighbour it shares with its successor.  out: vertex ids; returns the length. */
static int clockwise_vertices(Front *f, int inner, int *out)
{
    const RefEnv *e = f->e;
    const Graph *g = &f->g;
    int vs[MESHENV_REF_MAX_DEG];
    const int n = g->deg[inner];
    for (int j = 0; j < n; j++) vs[j] = g->adj[inner * MESHENV_REF_MAX_DEG + j];
    for (int i = 1; i < n; i++) {
        double max_angle = -1;
        int flag = i;
        for (int j = i; j < n; j++) {
            double a = cw(e->vtab[inner], e->vtab[vs[j]], e->vtab[vs[i - 1]]);
            if (a > max_angle) { max_angle = a; flag = j; }
        }
        if (flag != i) { int t = vs[i]; vs[i] = vs[flag]; vs[flag] = t; }
    }
    int m = 0;
    for (int i = 0; i < n; i++) {
        const int cur = vs[i], prev = vs[(i + n - 1) % n];
        int inter = -1;
        for (int j = 0; j < g->deg[cur] && inter < 0; j++) {
            int w = g->adj[cur * MESHENV_REF_MAX_DEG + j];
            if (w != inner && graph_has(g, prev, w)) inter = w;
        }
        out[m++] = prev;
        if (inter >= 0) out[m++] = inter;
    }
    return m;
}

/* is_inside_boundary, M:1069-1078 */
static int is_inside_boundary(const RefEnv *e, P2 original, P2 moved, const int *b, int nb, int left, int right)
{
    for (int i = 0; i < nb; i++) {
        const int bi = b[i], bp = b[(i + nb - 1) % nb];
        if ((left == bi || left == bp) && (right == bi || right == bp)) continue;
        if ((cw(moved, e->vtab[bi], e->vtab[bp]) < PI) != (cw(original, e->vtab[bi], e->vtab[bp]) < PI)) return 0;
    }
    return 1;
}

/* M:911-937; ids: vertex, _next_v, next_v, nn_v */
static P2 find_side_vertex(Front *f, int v, int _next, int next, int nn, double v_angle)
{
    const RefEnv *e = f->e;
    const P2 pv = e->vtab[v];
    const double d = (dist(pv, e->vtab[_next]) + dist(pv, e->vtab[next]) + dist(e->vtab[next], e->vtab[nn])) / 3;
    double target = 45;
    for (;;) {
        P2 nv = side_vertex(f, pv, e->vtab[next], e->vtab[nn], target, d, next >= e->n0 || nn >= e->n0);
        if (f->raised) return pv;
        if (target <= v_angle) return pv;
        int cb[2 * MESHENV_REF_MAX_DEG];
        int nb = clockwise_vertices(f, v, cb);
        if (is_inside_boundary(e, pv, nv, cb, nb, _next, next)) return nv;
        target -= 5;
    }
}

/* M:1030-1067; index = ring slot of the vertex */
static P2 find_indention_vertex(Front *f, int index, double v_angle)
{
    RefEnv *e = f->e;
    const int n = e->n;
    const int v = e->rid[index], left = e->rid[(index + 1) % n], right = e->rid[RI(index - 1, n)];
    const int l2 = e->rid[(index + 2) % n], r2 = e->rid[RI(index - 2, n)];
    const P2 pv = e->vtab[v];
    const double d = (dist(pv, e->vtab[left]) + dist(pv, e->vtab[right])) / 2;
    int near = 0;
    /* Boundary2D.get_closet_points(front, vertex, [r2, right, left, l2], d): any other front vertex within d */
    for (int i = 0; i < n && !near; i++) {
        int w = e->rid[i];
        if (w == v || w == r2 || w == right || w == left || w == l2) continue;
        if (dist(pv, e->vtab[w]) <= d) near = 1;
    }
    /* find_closest_segments, M:1103-1112: a front segment (not at the vertex) whose foot point lies inside it, within d.
     * Both loops of the reference run to the end whatever they find, so a zero-length segment between two domain vertices
     * raises (C:647, Python operands) even when a near vertex was already seen; with a generated endpoint the quotient is
     * 0 / np.float64(0) = nan and the segment is simply not "inner". */
    for (int i = 0; i < n; i++) {
        int p1 = e->rid[RI(i - 1, n)], p2 = e->rid[i];
        if (p1 == v || p2 == v) continue;
        const P2 a = e->vtab[p1], b = e->vtab[p2];
        double A = b.x - a.x, B = b.y - a.y;
        double s = py_div(f, A * pv.x + B * pv.y - B * a.y - A * a.x, SQ(A) + SQ(B), p1 >= e->n0 || p2 >= e->n0);
        if (f->raised) return pv;
        P2 t = {a.x + s * A, a.y + s * B};
        if (0 <= s && s <= 1 && dist(pv, t) <= d) near = 1;
    }
    if (!near) return pv;
    int times = 4;
    for (;;) {
        P2 nv = indention_vertex(f, pv, e->vtab[left], e->vtab[right], (360 - v_angle) / 2, d / times, v >= e->n0 || left >= e->n0);
        if (f->raised) return pv;
        if (times >= 10) return pv;
        int cb[2 * MESHENV_REF_MAX_DEG];
        int nb = clockwise_vertices(f, v, cb);
        if (is_inside_boundary(e, pv, nv, cb, nb, left, right)) return nv;
        times += 1;
    }
}

static int build_full_graph(const RefEnv *e, Graph *g)
{
    const int nv = e->n_vert, n0 = e->n0;
    int rc = 0;
    g->adj = (int32_t *)malloc(sizeof(int32_t) * (size_t)nv * MESHENV_REF_MAX_DEG);
    g->deg = (int32_t *)calloc((size_t)nv, sizeof(int32_t));
    for (int i = 0; i < n0 && rc == 0; i++) {
        int a = (i + n0 - 1) % n0;
        rc |= graph_add(g, a, i);
        rc |= graph_add(g, i, a);
    }
    for (int k = 0; k < e->n_elem && rc == 0; k++) {
        const int32_t *q = e->quads + 4 * k;
        for (int i = 0; i < 4 && rc == 0; i++) {
            const int a = q[i], b = q[(i + 3) & 3];
            if (graph_has(g, a, b)) continue;
            rc |= graph_add(g, a, b);
            rc |= graph_add(g, b, a);
        }
    }
    return rc;
}

/* the three vertex constructions as plain functions (unit tests against the reference's methods, tests/test_oracle_smooth.py):
 * which = 0 middle_vertex(vertex, left, right, target_angle), 1 side_vertex(vertex, next, nn, angle, dist),
 * 2 indention_vertex(vertex, left, right, angle, dist), 3 Mesh.estimate_4th_vertex(origin, left, right, factor,
 * suggest_dist; dist < 0: None; general/components.py:980-990).  in[8] = vertex, p1, p2 (x, y each), angle, dist; returns 1 where
 * the construction is undefined (the reference raises). */
int meshenv_ref_front_construction(int which, const double *in, double *out_xy)
{
    Front f;
    f.e = NULL; f.g.adj = NULL; f.g.deg = NULL; f.raised = 0;
    P2 v = {in[0], in[1]}, a = {in[2], in[3]}, b = {in[4], in[5]}, r;
    if (which == 0) r = middle_vertex(&f, v, a, b, in[6]);
    else if (which == 1) r = side_vertex(&f, v, a, b, in[6], in[7], 0);
    else if (which == 2) r = indention_vertex(&f, v, a, b, in[6], in[7], 0);
    else r = estimate_4th_vertex(v, a, b, in[6], in[7] >= 0, in[7]); /* 3: Mesh.estimate_4th_vertex(origin, left, right, factor, suggest_dist | None) */
    out_xy[0] = r.x; out_xy[1] = r.y;
    return f.raised;
}

int meshenv_ref_smooth_front(RefEnv *e)
{
    if (e->n_elem > e->cap_e || e->n_vert > e->cap_v) return -1;
    Front f;
    f.e = e;
    f.raised = 0;
    if (build_full_graph(e, &f.g) != 0) { free(f.g.adj); free(f.g.deg); return -1; }
    const int n = e->n;
    for (int i = 0; i < n && !f.raised; i++) {
        const int v = e->rid[i];
        if (v < e->n0) continue;
        const int nxt = e->rid[(i + 1) % n], prv = e->rid[RI(i - 1, n)];
        const double v_angle = rad2deg(cw(e->vtab[v], e->vtab[nxt], e->vtab[prv]));
        P2 nv = e->vtab[v];
        if (v_angle <= 90) {
            double target = v_angle >= 45 ? v_angle : 45;
            for (;;) {
                P2 cand = middle_vertex(&f, e->vtab[v], e->vtab[nxt], e->vtab[prv], target);
                if (target >= 135) break;
                int cb[2 * MESHENV_REF_MAX_DEG];
                int nb = clockwise_vertices(&f, v, cb);
                if (is_inside_boundary(e, e->vtab[v], cand, cb, nb, nxt, prv)) { nv = cand; break; }
                target += 5;
            }
        } else if (v_angle <= 180) {
            const int nn_r = e->rid[RI(i - 2, n)], nn_l = e->rid[(i + 2) % n];
            /* compute_boundary_angle, C:467-473 */
            const double left_angle = rad2deg(cw(e->vtab[nxt], e->vtab[nn_l], e->vtab[v]));
            const double right_angle = rad2deg(cw(e->vtab[prv], e->vtab[v], e->vtab[nn_r]));
            if (right_angle < 45) nv = find_side_vertex(&f, v, nxt, prv, nn_r, right_angle);
            else if (left_angle < 45) nv = find_side_vertex(&f, v, prv, nxt, nn_l, left_angle);
            else nv = find_indention_vertex(&f, i, v_angle);
        } else if (v_angle <= 270) {
            nv = find_indention_vertex(&f, i, v_angle);
        } else {
            /* inner_vertex(vertex, 45), M:865-880 */
            const P2 l = e->vtab[nxt], r = e->vtab[prv], pv = e->vtab[v];
            P2 m = {(l.x + r.x) / 2, (l.y + r.y) / 2};
            double d = dist(m, r) * tan(deg2rad(45));
            double A = pv.x - m.x, B = pv.y - m.y;
            double q = py_div(&f, SQ(d), SQ(A) + SQ(B), 1); /* A = vertex.x - m.x: the vertex is a generated one (NumPy) */
            if (f.raised) break;
            double sc = py_sqrt(&f, q);
            if (f.raised) break;
            if (!isfinite(m.x + sc * A) || !isfinite(m.y + sc * B)) { f.raised = 2; break; } /* see the header */
            e->vtab[v].x = m.x + sc * A;
            e->vtab[v].y = m.y + sc * B;
            e->ring[i] = e->vtab[v];
            nv = find_indention_vertex(&f, i, v_angle);
        }
        if (f.raised) break;
        if (!isfinite(nv.x) || !isfinite(nv.y)) { f.raised = 2; break; } /* see the header */
        e->vtab[v] = nv;
        e->ring[i] = nv;
    }
    free(f.g.adj); free(f.g.deg);
    /* not_valid_points holds the Vertex objects themselves: a listed front vertex that moved is tested (M:428-433) at its
     * new position from now on */
    for (int k = 0; k < e->n_nv; k++) e->nv[k] = e->vtab[e->nv_id[k]];
    return f.raised == 2 ? -4 : (f.raised ? -3 : 0);
}

/* smooth_pave(boundary.vertices, updated_boundary.vertices, iteration=..., interior=False), M:790-795, followed by the
 * find_next_state that move() runs right after it (B:420; is_static selects its observation form): front smoother,
 * interior relaxation, candidate list rebuilt, reference vertex and observation of the smoothed state.  Returns the
 * "observation is None" flag (>= 0), or the negative codes of the parts. */
int meshenv_ref_smooth_pave_full(RefEnv *e, int iteration, int is_static, float *obs, int32_t *sweeps_out)
{
    int rc = meshenv_ref_smooth_front(e);
    if (rc == -4) rc = -3; /* the reference raises either way: inside smooth_pave, or in the find_next_state after it */
    if (rc != 0) return rc;
    rc = meshenv_ref_smooth_interior(e, iteration, sweeps_out, NULL);
    if (rc != 0) return rc;
    return find_next_state_opt(e, obs, is_static, 0);
}

int meshenv_ref_not_valid_count(const RefEnv *e) { return e->n_nv; }

int meshenv_ref_ring_len(const RefEnv *e) { return e->n; }

void meshenv_ref_get_ring(const RefEnv *e, int32_t *ids, double *xy)
{
    for (int i = 0; i < e->n; i++) {
        if (ids) ids[i] = e->rid[i];
        if (xy) {
            xy[2 * i] = e->ring[i].x;
            xy[2 * i + 1] = e->ring[i].y;
        }
    }
}

int meshenv_ref_get_candidates(const RefEnv *e, int32_t *ids, double *keys)
{
    /* selection sort into (key asc, stamp desc) order: O(n^2), test-only */
    int n = e->n, m = 0;
    uint8_t *used = (uint8_t *)calloc((size_t)n, 1);
    for (;;) {
        int best = -1;
        for (int i = 0; i < n; i++) {
            if (!e->cand[i] || used[i]) continue;
            if (best < 0 || e->key[i] < e->key[best] || (e->key[i] == e->key[best] && e->stamp[i] > e->stamp[best]))
                best = i;
        }
        if (best < 0) break;
        used[best] = 1;
        ids[m] = e->rid[best];
        keys[m] = e->key[best];
        m++;
    }
    free(used);
    return m;
}

int meshenv_ref_ref_id(const RefEnv *e) { return e->ref < 0 ? -1 : e->rid[e->ref]; }

void meshenv_ref_get_scalars(const RefEnv *e, int32_t *n_elem, int32_t *failed_num, int32_t *n_vert,
                             double *current_area)
{
    *n_elem = e->n_elem;
    *failed_num = e->failed;
    *n_vert = e->n_vert;
    *current_area = e->cur_area;
}

void meshenv_ref_get_elements(const RefEnv *e, int32_t *quads, double *vertex_xy, int32_t *n_elem,
                              int32_t *n_vert)
{
    int ne = e->n_elem < e->cap_e ? e->n_elem : e->cap_e;
    int nv = e->n_vert < e->cap_v ? e->n_vert : e->cap_v;
    if (quads) memcpy(quads, e->quads, sizeof(int32_t) * 4 * (size_t)ne);
    if (vertex_xy)
        for (int i = 0; i < nv; i++) {
            vertex_xy[2 * i] = e->vtab[i].x;
            vertex_xy[2 * i + 1] = e->vtab[i].y;
        }
    *n_elem = ne;
    *n_vert = nv;
}

/* ------------------------------------------------- element quality report
 * The per-element measures of Mesh.get_quality(type) (general/components.py:863-933), the in-repo analogues of the
 * five Verdict metrics Measurement/quality_verdict.py:133-148 asks VTK for.  xy = the 4 vertices in Mesh.vertices
 * order.  out[0..7] = min corner angle (deg), max corner angle (deg), 's_jacobian', 'stretch', 'taper', 'robust',
 * compute_area()[0], 'default'. */
void meshenv_ref_element_quality(const double *xy, double *out)
{
    P2 m[4];
    for (int i = 0; i < 4; i++) { m[i].x = xy[2 * i]; m[i].y = xy[2 * i + 1]; }
    /* corner angles as in 'robust' (components.py:878-881); math.degrees(x) = x * (180 / pi) */
    /* (min() / max() of a Python list start from its first entry: a NaN there stays, a later one is passed over) */
    double amin = 0, amax = 0, err = 0;
    for (int i = 0; i < 4; i++) {
        double a = cw(m[i], m[(i + 1) % 4], m[(i + 3) % 4]);
        if (i == 0 || a < amin) amin = a;
        if (i == 0 || a > amax) amax = a;
        double e = fabs(a - PI / 2); /* get_ave_error_angle, components.py:855-861 */
        if (i == 0 || e > err) err = e;
    }
    out[0] = amin * (180.0 / PI);
    out[1] = amax * (180.0 / PI);
    /* 's_jacobian', components.py:891-906: p0..p3 = vertices[0], [-1], [-2], [-3] */
    {
        P2 p0 = m[0], p1 = m[3], p2 = m[2], p3 = m[1];
        double l0x = p1.x - p0.x, l0y = p1.y - p0.y, l1x = p2.x - p1.x, l1y = p2.y - p1.y;
        double l2x = p3.x - p2.x, l2y = p3.y - p2.y, l3x = p0.x - p3.x, l3y = p0.y - p3.y;
        double a3 = crossp(l2x, l2y, l3x, l3y), a2 = crossp(l1x, l1y, l2x, l2y);
        double a1 = crossp(l0x, l0y, l1x, l1y), a0 = crossp(l3x, l3y, l0x, l0y);
        double n0 = sqrt(SQ(l0x) + SQ(l0y)), n1 = sqrt(SQ(l1x) + SQ(l1y));
        double n2 = sqrt(SQ(l2x) + SQ(l2y)), n3 = sqrt(SQ(l3x) + SQ(l3y));
        /* a zero edge makes its two terms 0 / 0 and the reference raises ZeroDivisionError: the IEEE value is that NaN,
         * the value of the first term with a zero denominator (min() alone passes over a NaN that is not the first term) */
        double t0 = a0 / (n0 * n3), t1 = a1 / (n0 * n1), t2 = a2 / (n1 * n2), t3 = a3 / (n2 * n3);
        double j = t0;
        if (t1 < j) j = t1;
        if (t2 < j) j = t2;
        if (t3 < j) j = t3;
        out[2] = n0 * n3 == 0 ? t0 : (n0 * n1 == 0 ? t1 : (n1 * n2 == 0 ? t2 : (n2 * n3 == 0 ? t3 : j)));
        /* 'taper', components.py:885-890 */
        double x1x = (p1.x - p0.x) + (p2.x - p3.x), x1y = (p1.y - p0.y) + (p2.y - p3.y);
        double x2x = (p2.x - p1.x) + (p3.x - p0.x), x2y = (p2.y - p1.y) + (p3.y - p0.y);
        double x12x = (p0.x - p1.x) + (p2.x - p3.x), x12y = (p0.y - p1.y) + (p2.y - p3.y);
        double len1 = sqrt(SQ(x1x) + SQ(x1y)), len2 = sqrt(SQ(x2x) + SQ(x2y));
        out[4] = sqrt(SQ(x12x) + SQ(x12y)) / (len2 < len1 ? len2 : len1);
    }
    /* 'stretch', components.py:870-872 */
    {
        double mn = 0;
        for (int i = 0; i < 4; i++) {
            double l = dist(m[(i + 3) % 4], m[i]);
            if (i == 0 || l < mn) mn = l;
        }
        double d0 = dist(m[0], m[2]), d1 = dist(m[1], m[3]);
        out[3] = sqrt(2.0) * mn / (d1 > d0 ? d1 : d0);
    }
    out[5] = quad_robust(m);
    out[6] = quad_area(m);
    /* 'default', components.py:864-869 with get_aspect_ratio 839-844 */
    {
        double mx = 0, mn = 0;
        for (int i = 0; i < 4; i++) {
            double l = dist(m[i], m[(i + 3) % 4]);
            if (i == 0 || l > mx) mx = l;
            if (i == 0 || l < mn) mn = l;
        }
        double aspect = mn != 0 ? mx / mn : 0.001;
        out[7] = 1 / (aspect + err);
    }
}

/* MeshGeneration.get_quality(element, index), M:1728-1747, for the indices that depend on the quad alone:
 * 0 'default' (C:864-869), 1 compute_element_quality (M:1714-1726: sqrt(q1 q2) of get_quality_3, C:952-972),
 * 3 'stretch', 4 'robust', 5 'strong' (C:907-930).  NaN for any other index. */
double meshenv_ref_quad_quality(const double *xy, int index)
{
    double rec[8];
    if (index == 0 || index == 3 || index == 4) {
        meshenv_ref_element_quality(xy, rec);
        return index == 0 ? rec[7] : (index == 3 ? rec[3] : rec[5]);
    }
    if (index != 1 && index != 5) return NAN;
    P2 m[4];
    for (int i = 0; i < 4; i++) { m[i].x = xy[2 * i]; m[i].y = xy[2 * i + 1]; }
    double e[4], ang[4];
    for (int i = 0; i < 4; i++) {
        e[i] = dist(m[i], m[(i + 3) % 4]);
        ang[i] = cw(m[i], m[(i + 1) % 4], m[(i + 3) % 4]);
    }
    double area = 0.5 * e[0] * e[1] * sin(ang[0]) + 0.5 * e[2] * e[3] * sin(ang[2]); /* compute_area, C:935-950 */
    double q1 = 0;
    if (!(area <= 0)) { /* get_quality_3, C:952-961: `if area <= 0: q1 = 0`, so a NaN area takes the pow branch */
        double product = 1;
        for (int i = 0; i < 4; i++) product *= pow(e[i] / sqrt(area), sqrt(area) - e[i] > 0 ? 1 : -1);
        q1 = pow(product, 1.0 / 4);
    }
    double ap = 1;
    for (int i = 0; i < 4; i++) ap *= 1 - (fabs(ang[i] * (180.0 / PI) - 90) / 90); /* math.degrees(x) = x * (180 / pi) */
    double q2 = ap < 0 ? 0 : pow(ap, 1.0 / 4);
    if (index == 1) return pow(q1 * q2, 1.0 / 2);
    double amin = 0, amax = 0;
    for (int i = 0; i < 4; i++) {
        double a = fabs(ang[i]);
        if (i == 0 || a < amin) amin = a;
        if (i == 0 || a > amax) amax = a;
    }
    return sqrt(q1 * (amin / amax));
}

/* DumpQualityStats (Measurement/quality_verdict.py:77-90) prints, per measure, what vtkMeshQuality accumulates over
 * the cells of one mesh: minimum, average, maximum, variance (E[q^2] - E[q]^2) and cardinality.  vals = [n][8]
 * element records, stats = [8][4] = min, mean, max, variance.  (VTK itself is absent: parity unpinned for the
 * aggregate; the restatement follows the published vtkMeshQuality accumulation.) */
void meshenv_ref_quality_stats(const double *vals, int n, double *stats)
{
    for (int k = 0; k < 8; k++) {
        double mn = INFINITY, mx = -INFINITY, s = 0, s2 = 0;
        for (int i = 0; i < n; i++) {
            double q = vals[8 * i + k];
            if (q < mn) mn = q;
            if (q > mx) mx = q;
            s += q;
            s2 += q * q;
        }
        double avg = n ? s / n : 0;
        stats[4 * k] = n ? mn : 0;
        stats[4 * k + 1] = avg;
        stats[4 * k + 2] = n ? mx : 0;
        stats[4 * k + 3] = n ? s2 / n - avg * avg : 0;
    }
}

void meshenv_ref_step_batch(RefEnv **envs, int n, const float *actions, float *obs, double *reward,
                            uint8_t *done, uint8_t *is_complete, float *terminal_obs, int auto_reset,
                            int threads)
{
    (void)threads;
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 16) num_threads(threads > 0 ? threads : 1)
#endif
    for (int i = 0; i < n; i++) {
        meshenv_ref_step(envs[i], actions + 3 * i, obs + 18 * i, reward + i, done + i, is_complete + i);
        if (done[i] && auto_reset) {
            if (terminal_obs) memcpy(terminal_obs + 18 * i, obs + 18 * i, 18 * sizeof(float));
            meshenv_ref_reset(envs[i], obs + 18 * i);
        }
    }
}

/* T vector steps in ONE parallel region (the CPU baseline's best form: no fork / join per vector step, every env's state
 * stays in its thread's cache): thread-private env ranges, actions [T][n][3]; outputs of the LAST step only (obs / reward /
 * flags as meshenv_ref_step_batch writes them). */
void meshenv_ref_rollout_batch(RefEnv **envs, int n, int T, const float *actions, float *obs, double *reward,
                               uint8_t *done, uint8_t *is_complete, int auto_reset, int threads)
{
    (void)threads;
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 8) num_threads(threads > 0 ? threads : 1)
#endif
    for (int i = 0; i < n; i++) {
        for (int t = 0; t < T; t++) {
            meshenv_ref_step(envs[i], actions + ((size_t)t * n + i) * 3, obs + 18 * i, reward + i, done + i, is_complete + i);
            if (done[i] && auto_reset) meshenv_ref_reset(envs[i], obs + 18 * i);
        }
    }
}
