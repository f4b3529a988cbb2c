"""The synthetic-sample generator of the supervised mesher, restated in float64 Python `math` (the reference's own arithmetic):
`MeshAugmentation.sampling` of general/data_augmentation.py as csrc/meshenv_augment.h states it.  Written from the statement in
DESIGN.md section 30, array in / array out; nothing here reads the reference.

    uniforms -> proposal (angle, obs, actions)      propose_one / propose
    obs -> check_obs_quality                        obs_rejected
    (obs, act) -> ele, boundary, max_ele, max_bnd   score_one / score
    Philox4x32-10 uniforms of (seed, w, t, b, p)    philox_uniforms
    the ordered selection that stops at a quota     select_bin / sampling
"""
from __future__ import annotations

import math

import numpy as np

from policy_ref import philox4x32

MASK = 0xFFFFFFFF
PHILOX_TAG = 5                      # csrc/meshenv_augment.h kAugPhiloxTag: 0..4 are taken (tests/test_augment_cpu.py)
TYPES = (0.5, 0.0, 1.0)             # type index t = 0, 1, 2: the order sampling() concatenates
FRACS = (0.5, 0.25, 0.25)
BINS = (0.4, 0.6, 0.8, 1.0, 1.2, 1.4, 1.6, 1.8, 2.0, 2.2, 2.4)
N_ACTIONS = (20, 1, 1)              # candidates per surviving proposal
N_UNIFORMS = (57, 17, 17)           # 1 + 16 + 2 * 20, 1 + 16
LAM = 0.618


# ---------------------------------------------------------------------------------------------------------------- counts
def quota(n, pool, t):
    """ceil(frac_t * (n / pool) / 11): the count at which a bin's loop stops."""
    return math.ceil(FRACS[t] * (n / pool) / 11)


def rows_per_bin(n, pool, t):
    """The count is incremented before the append, and the loop leaves at the quota: Q - 1 rows."""
    return max(quota(n, pool, t) - 1, 0)


def row_count(n, pool=1):
    return pool * 11 * sum(rows_per_bin(n, pool, t) for t in range(3))


# --------------------------------------------------------------------------------------------------------------- uniforms
def philox_uniforms(seed, w, t, b, p, count):
    """Uniforms 0 .. count-1 of proposal p of (worker w, type index t, bin b), float64 [count].
    Counter words (p, (j >> 1) | b << 8 | t << 16, w, PHILOX_TAG), key (seed lo, seed hi); uniform j is numpy's 53-bit map of
    words (0, 1) of its block when j is even, (2, 3) when odd."""
    blocks = (count + 1) // 2
    j = np.arange(blocks, dtype=np.uint64)
    c1 = j | np.uint64(b << 8) | np.uint64(t << 16)
    words = philox4x32(np.full(blocks, p & MASK, np.uint64), c1, np.full(blocks, w, np.uint64), PHILOX_TAG, seed & MASK,
                       (seed >> 32) & MASK)
    a = np.stack([words[0], words[2]], 1).reshape(-1).astype(np.uint64)
    c = np.stack([words[1], words[3]], 1).reshape(-1).astype(np.uint64)
    u = ((a >> np.uint64(5)) * np.uint64(67108864) + (c >> np.uint64(6))).astype(np.float64) / 9007199254740992.0
    return u[:count]


# -------------------------------------------------------------------------------------------------------------- proposals
def propose_one(u, t, b):
    """One proposal from its uniforms (N_UNIFORMS[t] of them, in draw order): (angle, obs [18], actions [N_ACTIONS[t]][3])."""
    it = iter(u)

    def rnd(lo, hi):
        return float(next(it)) * (hi - lo) + lo

    k = BINS[b]
    angle = rnd(k - 0.2, k)
    o = [0.0] * 18
    o[0] = rnd(0.01, 0.45)
    o[2] = rnd(0.1, 0.77)
    if t == 0:
        o[3] = rnd(-0.5, 0.9) * math.pi
    elif t == 1:
        o[3] = rnd(-0.5 * math.pi, angle)
    else:
        o[3] = rnd(0.01, angle)
    o[4] = rnd(0.33, 1)
    o[5] = rnd(-0.5, 0.9) * math.pi
    o[6] = rnd(0.15, 1)
    o[7] = rnd(0, 1 / 3 * angle)
    o[8] = rnd(0.15, 1)
    o[9] = rnd(1 / 3 * angle, 2 / 3 * angle)
    o[10] = rnd(0.15, 1)
    o[11] = rnd(2 / 3 * angle, angle)
    o[12] = rnd(0.33, 1)
    o[13] = rnd(0.1, 1.5) * math.pi
    o[14] = rnd(0.1, 0.77)
    o[15] = rnd(0.01, angle) if t == 1 else rnd(0.01, 1.5) * math.pi
    o[16] = rnd(0.01, 0.45)
    o[17] = angle
    if t == 0:
        acts = [[0.5, rnd(0.01, 0.56), rnd(0.01, angle)] for _ in range(20)]
    elif t == 1:
        acts = [[0.0, o[14], o[15]]]
    else:
        acts = [[1.0, o[2], o[3]]]
    return angle, o, acts


# --------------------------------------------------------------------------------------------------------------- geometry
def _dist(a, b):
    return math.sqrt((a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2)


def _cw(s, p1, p2):
    v1x, v1y = p1[0] - s[0], p1[1] - s[1]
    v2x, v2y = p2[0] - s[0], p2[1] - s[1]
    theta = -math.atan2(v1x * v2y - v1y * v2x, v1x * v2x + v1y * v2y)
    return round(theta, 4) if math.copysign(1, theta) >= 0 else round(2 * math.pi + theta, 4)


def _cross(ax, ay, bx, by):
    return ax * by - bx * ay


def _straddle(p1, p2, q1, q2):
    s1 = round(math.sin(_cw(p1, q1, p2)), 4)
    s2 = round(math.sin(_cw(p1, q2, p2)), 4)
    if s1 == s2 and s2 == 0:
        l1, l2 = _dist(p1, p2), _dist(q1, q2)
        if l1 > l2:
            m = ((p2[0] + p1[0]) / 2, (p2[1] + p1[1]) / 2)
            return min(_dist(m, q2), _dist(m, q1)) <= l1 / 2
        m = ((q2[0] + q1[0]) / 2, (q2[1] + q1[1]) / 2)
        return min(_dist(m, p2), _dist(m, p1)) <= l2 / 2
    vmx, vmy = p2[0] - p1[0], p2[1] - p1[1]
    return _cross(q1[0] - p1[0], q1[1] - p1[1], vmx, vmy) * _cross(q2[0] - p1[0], q2[1] - p1[1], vmx, vmy) <= 0


def _is_cross(a1, a2, b1, b2):
    return _straddle(a1, a2, b1, b2) and _straddle(b1, b2, a1, a2)


def _seg_dist(p1, p2, v):
    a, b = p1
    A, B = p2[0] - p1[0], p2[1] - p1[1]
    s = (A * v[0] + B * v[1] - B * b - A * a) / (A ** 2 + B ** 2)
    if 0 <= s <= 1:
        return _dist(v, (a + s * A, b + s * B))
    return _dist(v, p1) if s < 0 else _dist(v, p2)


def _points(obs):
    """(n_points [7], r_points [3]): the nine (r, a) pairs as points, the origin in the middle of the seven."""
    pts = [(obs[i] * math.cos(obs[i + 1]), obs[i] * math.sin(obs[i + 1])) for i in range(0, 18, 2)]
    return [pts[6], pts[7], pts[8], (0, 0), pts[0], pts[1], pts[2]], [pts[3], pts[4], pts[5]]


def obs_rejected(obs):
    """check_obs_quality: a crossing among the seven-point front (segment i against j >= i + 2) or with the two radius
    segments, in the order the reference tests them, then longest / shortest front edge >= 5."""
    n, r = _points(obs)
    for i in range(1, 7):
        for j in range(i + 2, 7):
            if _is_cross(n[i], n[i - 1], n[j], n[j - 1]):
                return True
        for k in range(1, 3):
            if _is_cross(n[i], n[i - 1], r[k], r[k - 1]):
                return True
    lengths = [_dist(n[i], n[i - 1]) for i in range(1, 7)]
    return max(lengths) / min(lengths) >= 5


def _strong(m):
    e = [_dist(m[i], m[i - 1]) for i in range(4)]
    ang = [_cw(m[i], m[(i + 1) % 4], m[i - 1]) for i in range(4)]
    area = 0.5 * e[0] * e[1] * math.sin(_cw(m[0], m[1], m[3])) + 0.5 * e[2] * e[3] * math.sin(_cw(m[2], m[3], m[1]))
    if area <= 0:
        q1 = 0
    else:
        product = 1
        for edge in e:
            product *= math.pow(edge / math.sqrt(area), 1 if math.sqrt(area) - edge > 0 else -1)
        q1 = math.pow(product, 1 / 4)
    a = [math.fabs(x) for x in ang]
    return math.sqrt(q1 * (min(a) / max(a)))


def _boundary_quality(m, new_at, lo, hi, n, r):
    """compute_boundary_quality.  new_at: the quad slot of the generated vertex, or None; lo, hi: the smallest and largest
    index in n of the quad's vertices (no generated vertex)."""
    if new_at is not None:
        v = m[new_at]
        # the quad is (new, n[4], n[3], n[2]): left = m[-1] = n[2], right = m[1] = n[4]
        left, right = m[new_at - 1], m[(new_at + 1) % 4]
        left_angle = _cw(left, n[1], v)
        right_angle = _cw(right, v, n[5])
        angles = [a for a in (left_angle, right_angle) if a < math.pi / 2]
        q1 = 2 * min(angles) / math.pi if angles else 1
        dist = _dist(v, left) + _dist(v, right)
        dists = [_seg_dist(n[0], n[1], v), _seg_dist(n[6], n[5], v), _seg_dist(r[0], r[1], v), _seg_dist(r[1], r[2], v)]
        m_d = min(dists)
        q2 = m_d / dist if m_d < dist else 1
        target = dist / 2
        chain = [n[1], n[2], v, n[4], n[5]]
        mean = sum([_dist(chain[i], chain[i - 1]) for i in range(1, 5)]) / 4
        return math.pow(q1 * q2 * (min(mean, target) / max(mean, target)), 1 / 3)
    # 0 < lo and hi < 6 for both quads of the seven-point front (lo, hi = 1, 4 or 2, 5)
    left_angle = _cw(n[lo], n[lo - 1], n[hi])
    right_angle = _cw(n[hi], n[lo], n[hi + 1])
    angles = [a for a in (left_angle, right_angle) if a < math.pi / 2]
    chain = [n[lo - 1], n[lo], n[hi], n[hi + 1]]
    angle_quality = 2 * min(angles) / math.pi if angles else 1
    target = _dist(n[lo], n[hi])
    mean = sum([_dist(chain[i], chain[i - 1]) for i in range(1, 4)]) / 3
    return math.sqrt(angle_quality * (min(mean, target) / max(mean, target)))


def score_one(obs, act):
    """(valid, ele, boundary, max_ele, max_boundary) of one candidate: compute_quality and estimate_max_quality(method=3)."""
    n, r = _points(obs)
    kind = act[0]
    new_at, lo, hi = None, 0, 0
    if kind == 0:
        m, lo, hi = [n[1], n[4], n[3], n[2]], 1, 4
    elif kind == 1:
        m, lo, hi = [n[2], n[5], n[4], n[3]], 2, 5
    else:
        m, new_at = [(act[1] * math.cos(act[2]), act[1] * math.sin(act[2])), n[4], n[3], n[2]], 0
    # Mesh.is_valid(0): the two pairs of opposite sides do not cross, every corner within (0.01 pi, 0.99 pi)
    valid = not _is_cross(m[0], m[1], m[2], m[3]) and not _is_cross(m[0], m[3], m[1], m[2])
    if valid:
        for i in range(4):
            d = _cw(m[i], m[(i + 1) % 4], m[i - 1])
            if d > 0.99 * math.pi or d < 0.01 * math.pi:
                valid = False
                break
    if valid:
        # check_intersection: every side of the quad against every front and radius segment that shares no vertex OBJECT
        # with it (the reference compares identities; the generated vertex is in no list)
        ids = [None, 4, 3, 2] if new_at is not None else ([1, 4, 3, 2] if kind == 0 else [2, 5, 4, 3])
        for i in range(4):
            a, b = ids[i], ids[i - 1]
            for j in range(1, 7):
                if a not in (j, j - 1) and b not in (j, j - 1) and _is_cross(m[i], m[i - 1], n[j], n[j - 1]):
                    valid = False
            for j in range(1, 3):
                if _is_cross(m[i], m[i - 1], r[j], r[j - 1]):
                    valid = False
    if valid:
        # check_internal_element: the segment from each of r[0..2], n[0], n[6] to the centroid has to cross a side
        cx = (((0 + m[0][0]) + m[1][0]) + m[2][0] + m[3][0]) / 4
        cy = (((0 + m[0][1]) + m[1][1]) + m[2][1] + m[3][1]) / 4
        for v in r + [n[0], n[6]]:
            if not any(_is_cross(v, (cx, cy), m[i], m[i - 1]) for i in range(4)):
                valid = False
                break
    ele = boundary = 0
    if valid:
        ele = _strong(m)
        boundary = _boundary_quality(m, new_at, lo, hi, n, r)
    # estimate_max_quality(method=3)
    left, right, o = n[2], n[4], n[3]
    angle = _cw(o, left, right)
    rem = (2 * math.pi - angle) / 3
    angle_quality = min(angle, rem) / max(angle, rem)
    l1, l2 = _dist(o, left), _dist(o, right)
    area = l2 * l1 * math.sin(angle)
    product = 1
    for edge in (l1, l2):
        product *= math.pow(edge / math.sqrt(area), 1 if math.sqrt(area) - edge > 0 else -1)
    edge_quality = math.pow(product, 1 / 4)
    dists = [_seg_dist(r[0], r[1], o), _seg_dist(r[1], r[2], o)]
    max_ele = math.sqrt(angle_quality * edge_quality)
    max_boundary = math.sqrt(min(1, max(dists) / ((math.sqrt(2) / 2 + 0.5) * (l1 + l2))))
    return valid, ele, boundary, max_ele, max_boundary


def ratios(ele, boundary, max_ele, max_boundary):
    """The two quantities compared with the threshold."""
    quality = (1 - LAM) * ele + LAM * boundary
    max_quality = (1 - LAM) * max_ele + LAM * max_boundary
    return quality / max_quality, ele / max_ele


def accepted(ele, boundary, max_ele, max_boundary, threshold):
    a, b = ratios(ele, boundary, max_ele, max_boundary)
    return a >= threshold and b >= threshold


def propose(uniforms, t_index, b_index):
    """Arrays: uniforms [B, 57] (columns past N_UNIFORMS[t] unread), t_index, b_index [B] -> angle [B], obs [B, 18],
    actions [B, 20, 3] (rows past N_ACTIONS[t] zero), rejected [B] bool."""
    B = len(uniforms)
    angle, obs, acts, rej = np.zeros(B), np.zeros((B, 18)), np.zeros((B, 20, 3)), np.zeros(B, bool)
    for i in range(B):
        t, b = int(t_index[i]), int(b_index[i])
        angle[i], o, a = propose_one(uniforms[i, :N_UNIFORMS[t]], t, b)
        obs[i] = o
        acts[i, :len(a)] = a
        rej[i] = obs_rejected(o)
    return angle, obs, acts, rej


def score(obs, act):
    """Arrays [B, 18], [B, 3] -> rejected, valid [B] bool, q [B, 4] = ele, boundary, max_ele, max_boundary."""
    B = len(obs)
    rej, valid, q = np.zeros(B, bool), np.zeros(B, bool), np.zeros((B, 4))
    for i in range(B):
        o, a = [float(v) for v in obs[i]], [float(v) for v in act[i]]
        rej[i] = obs_rejected(o)
        valid[i], *q[i] = score_one(o, a)
    return rej, valid, q


# -------------------------------------------------------------------------------------------------------------- selection
def select_bin(seed, w, t, b, rows, threshold, max_proposals=1 << 22):
    """The first `rows` accepted candidates of the bin's stream in (proposal, action) order: x [rows, 18], y [rows, 3]."""
    x, y = [], []
    p = 0
    while len(x) < rows:
        if p >= max_proposals:
            raise RuntimeError(f"bin ({w}, {t}, {b}): {len(x)} of {rows} rows after {p} proposals")
        _, o, acts = propose_one(philox_uniforms(seed, w, t, b, p, N_UNIFORMS[t]), t, b)
        p += 1
        if obs_rejected(o):
            continue
        for a in acts:
            _, *q = score_one(o, a)
            if accepted(*q, threshold):
                x.append(o)
                y.append(a)
                if len(x) == rows:
                    break
    return np.array(x, np.float64).reshape(rows, 18), np.array(y, np.float64).reshape(rows, 3)


def sampling(n, threshold, seed=0, pool=1, workers=None):
    """sampling_main(pool, n, threshold) on the Philox streams: (x [R, 18], y [R, 3]) float64, ordered worker, type
    0.5 / 0 / 1, bin, acceptance.  workers: the worker indices to compute (default all of the pool)."""
    xs, ys = [], []
    for w in (range(pool) if workers is None else workers):
        for t in range(3):
            rows = rows_per_bin(n, pool, t)
            for b in range(11):
                x, y = select_bin(seed, w, t, b, rows, threshold)
                xs.append(x)
                ys.append(y)
    return np.concatenate(xs), np.concatenate(ys)
