"""TEST INFRASTRUCTURE: the quads on which the quality kernels (csrc/meshenv_quality.h) are pinned, and the host side of
the comparison (tests/test_quality_edges_cpu.py, tests/test_gpu_quality_edges.py, oracle/gen_golden.py --quality-edges-only).

* classes(): a deterministic list of named quad classes -- well-formed, concave, self-intersecting, reversed, zero
  edges, coincident and collinear vertices, near-degenerate, axis-aligned, kites / trapezoids whose sqrt(area) is an edge
  length, non-finite -- and their images under the transforms of the xf_* fixtures (scale 1e-3, 1e3, 1e4; shift
  (1e6, 0), (1e8, -1e8)).
* the reference of every comparison is the oracle (oracle.ref_lib.element_quality / quad_quality), which
  tests/golden/quality_edge_quads.npz pins to the reference repository on a sample of every class.
* ieee_records(): the oracle's arithmetic restated in numpy float64, with the square either libm's pow(v, 2.0) (the
  oracle's; equal to it bit for bit, asserted on the CPU) or v * v (the device's: entries 0-4 are then IEEE operations
  only and the device must give the same bits).
* extended(): the same formulas in np.longdouble from the oracle's own quantised corner angles (the 1e-4 rounding is a
  discontinuity and is not re-decided).  Used ONLY to measure the oracle's own rounding error, from which bounds() derives
  what the device may differ by.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

PI = 3.141592653589793
RECORD_NAMES = ("min_angle_deg", "max_angle_deg", "scaled_jacobian", "stretch", "taper", "robust", "area", "default")
INDICES = (0, 1, 3, 4, 5)                 # MeshGeneration.get_quality(element, index) of the quad alone
OUTPUTS = tuple(f"rec{k}" for k in range(8)) + tuple(f"idx{k}" for k in INDICES)
EXACT_OUTPUTS = ("rec0", "rec1", "rec2", "rec3", "rec4")   # IEEE operations only: the device gives the same bits
BRANCH_OUTPUTS = ("idx1", "idx5")         # the outputs that depend on the area <= 0 branch alone
BASE_RTOL, BASE_ATOL = 1e-12, 1e-13       # the project's bar for quality records (tests/test_gpu_quality.py)
FACTOR = 4.0                              # device allowance in units of the oracle's own deviation (see bounds())
AMBIGUOUS_CAP = 1e-3                      # at most 0.1 % of a class may sit on a branch the device may take otherwise
TRANSFORMS = (("", 1.0, (0.0, 0.0)), ("x1e-3", 1e-3, (0.0, 0.0)), ("x1e3", 1e3, (0.0, 0.0)), ("x1e4", 1e4, (0.0, 0.0)),
              ("dx1e6", 1.0, (1e6, 0.0)), ("d1e8", 1.0, (1e8, -1e8)))
WELL_BASES = ("well_formed", "concave", "reversed")
WELL_TRANSFORMS = ("", "x1e-3", "x1e3", "x1e4")
M = 1024                                  # quads per random class


# ------------------------------------------------------------------------------------------------ generator
def _convex(rng, m):
    """m clockwise convex quads (the orientation of every element the environment accepts)."""
    out = []
    sq = np.array([[0.0, 0.0], [0.0, 1.0], [1.0, 1.0], [1.0, 0.0]])
    while len(out) < m:
        q = sq + rng.uniform(-0.3, 0.3, (4, 2))
        th = rng.uniform(0, 2 * math.pi)
        rot = np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
        q = (q - 0.5) @ rot.T * rng.uniform(0.5, 2.0) + rng.uniform(-3, 3, 2)
        e = np.roll(q, -1, 0) - q
        cr = e[:, 0] * np.roll(e, -1, 0)[:, 1] - e[:, 1] * np.roll(e, -1, 0)[:, 0]
        if (cr < -0.05).all():
            out.append(q)
    return np.array(out)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _ra_equals_edge_rectangles():
    """Axis-aligned 1 x h rectangles on which the oracle's sqrt(area) EQUALS an edge length in float64: the corner angle
    quantises to 1.5708, sin(1.5708) = 1 - 6.7e-12, so h is searched among the doubles around 1 / sin(1.5708)."""
    s = math.sin(round(math.pi / 2, 4))
    found = []
    for base, other in ((1.0 / s, 1.0), (s, None)):
        h = base
        for _ in range(64):
            h = math.nextafter(h, 0.0)
        for _ in range(128):
            h = math.nextafter(h, math.inf)
            w = 1.0 if other is not None else h       # 1 x h rectangle / h x h square
            area = 0.5 * w * h * s + 0.5 * w * h * s
            if math.sqrt(area) in (w, h):
                found.append(np.array([[0.0, 0.0], [0.0, h], [w, h], [w, 0.0]]))
    return found


def base_classes():
    """[(name, quads [m, 4, 2] float64)], deterministic."""
    rng = np.random.default_rng(20240229)
    cls = []
    cv = _convex(rng, 6 * M)
    take = iter(range(6))

    def fresh():
        k = next(take)
        return cv[k * M:(k + 1) * M].copy()

    wf = fresh()
    wf[:M // 2] = np.round(wf[:M // 2], 4)                       # half on the 1e-4 lattice of the environment
    cls.append(("well_formed", wf))
    q = fresh()                                                  # one reflex corner
    k = rng.integers(0, 4, M)
    i = np.arange(M)
    mid = 0.5 * (q[i, (k + 1) % 4] + q[i, (k + 3) % 4])
    q[i, k] = mid + rng.uniform(0.15, 0.7, (M, 1)) * (q[i, (k + 2) % 4] - mid)
    cls.append(("concave", q))
    q = fresh()
    q[:, [1, 2]] = q[:, [2, 1]]
    cls.append(("self_intersecting", q))
    cls.append(("reversed", fresh()[:, ::-1].copy()))
    src = fresh()
    q = src.copy(); q[i, (k + 1) % 4] = q[i, k]
    cls.append(("one_zero_edge", q))
    q = src.copy()
    q[:M // 2, 1] = q[:M // 2, 0]; q[:M // 2, 3] = q[:M // 2, 2]          # two opposite edges: a segment
    q[M // 2:, 1] = q[M // 2:, 0]; q[M // 2:, 2] = q[M // 2:, 0]          # two adjacent edges: three vertices in one
    cls.append(("two_zero_edges", q))
    q = src.copy(); q[i, (k + 2) % 4] = q[i, k]
    cls.append(("coincident_opposite", q))
    q = src.copy(); q[:] = q[:, :1]
    cls.append(("all_coincident", q))
    q = src.copy()                                               # three collinear: generic (to rounding) and exact
    q[i, k] = 0.5 * (q[i, (k + 1) % 4] + q[i, (k + 3) % 4])
    a, b = np.round(rng.uniform(-3, 3, (M // 2, 2)), 4).T
    h1, h2, w = np.round(rng.uniform(0.2, 1.5, (3, M // 2)), 4)
    q[:M // 2] = np.stack([np.stack([a, b], 1), np.stack([a, b + h1], 1), np.stack([a, b + h1 + h2], 1),
                           np.stack([a + w, b + rng.uniform(0, 1, M // 2) * (h1 + h2)], 1)], 1)
    cls.append(("three_collinear", q))
    t = np.where(rng.random((M, 1)) < 0.5, np.array([[0.0, 1.0, 0.5, 2.0]]), np.array([[0.0, 1.0, 2.0, 3.0]]))
    t = t * rng.uniform(0.3, 1.5, (M, 1)) * np.where(rng.random((M, 1)) < 0.5, -1.0, 1.0)
    d = _unit(rng.normal(size=(M, 2)))
    d[:M // 4] = [1.0, 0.0]; d[M // 4:M // 2] = [0.0, 1.0]       # exact on the axes
    q = rng.uniform(-3, 3, (M, 1, 2)) + t[:, :, None] * d[:, None, :]
    q[:M // 2] = np.round(q[:M // 2], 4)
    cls.append(("all_collinear", q))
    q = src.copy()                                               # near-degenerate
    h = M // 2
    chord = q[i, (k + 1) % 4] - q[i, (k + 3) % 4]
    nrm = np.stack([-chord[:, 1], chord[:, 0]], 1)
    delta = 10 ** rng.uniform(-9, -3, (M, 1)) * np.where(rng.random((M, 1)) < 0.5, -1.0, 1.0)
    q[i[:h], k[:h]] = (0.5 * (q[i, (k + 1) % 4] + q[i, (k + 3) % 4]) + 0.25 * delta * nrm)[:h]   # corner delta off collinear
    eps = 10 ** rng.uniform(-12, -6, (M, 1))
    q[i[h:], (k[h:] + 1) % 4] = (q[i, k] + eps * (q[i, (k + 1) % 4] - q[i, k]))[h:]               # an edge eps of the others
    cls.append(("near_degenerate", q))
    a, b = np.round(rng.uniform(-3, 3, (M, 2)), 4).T             # axis-aligned, clockwise
    w, hh = np.round(rng.uniform(0.1, 2.0, (2, M)), 4)
    hh[:M // 4] = w[:M // 4]
    a[:M // 8] = np.round(a[:M // 8]); b[:M // 8] = np.round(b[:M // 8]); w[:M // 8] = hh[:M // 8] = 1.0
    q = np.stack([np.stack([a, b], 1), np.stack([a, b + hh], 1), np.stack([a + w, b + hh], 1), np.stack([a + w, b], 1)], 1)
    q[0] = [[0.0, 0.0], [0.0, 1.0], [1.0, 1.0], [1.0, 0.0]]
    exact = _ra_equals_edge_rectangles()
    assert 0 < len(exact) < 64
    q[1:1 + len(exact)] = np.array(exact)
    q[512:] = np.roll(q[512:], 1, axis=1)                        # every vertex takes the first slot
    cls.append(("axis_aligned", q))
    w = rng.uniform(0.5, 2.0, M)                                 # kites and trapezoids with sqrt(area) = an edge length
    h1 = w * rng.uniform(0.2, 1.5, M)
    h2 = (w * w + h1 * h1) / w - h1
    z = np.zeros(M)
    kite = np.stack([np.stack([z, h1], 1), np.stack([w, z], 1), np.stack([z, -h2], 1), np.stack([-w, z], 1)], 1)
    a = rng.uniform(0.3, 2.0, M); b = rng.uniform(0.3, 2.0, M); hh = 0.5 * (a + b)
    trap = np.stack([np.stack([z, z], 1), np.stack([z, a], 1), np.stack([hh, b], 1), np.stack([hh, z], 1)], 1)
    q = np.where((np.arange(M) % 2 == 0)[:, None, None], kite, trap) + rng.uniform(-3, 3, (M, 1, 2))
    cls.append(("kite_trapezoid", q))
    return cls


def non_finite():
    sq = np.array([[0.3, 0.2], [0.1, 1.3], [1.2, 1.1], [1.4, -0.1]])
    out = []
    for bad in (np.nan, np.inf, -np.inf):
        for v in range(4):
            for c in range(2):
                q = sq.copy(); q[v, c] = bad
                out.append(q)
    q = sq.copy(); q[1] = np.nan; out.append(q)
    q = sq.copy(); q[0] = np.inf; q[2] = np.inf; out.append(q)
    q = sq.copy(); q[0, 0] = np.inf; q[1, 0] = -np.inf; out.append(q)
    out.append(np.full((4, 2), np.nan))
    for den in (5e-324, -5e-324, 1e-310):                         # a denormal coordinate in an ordinary quad
        q = sq.copy(); q[0, 0] = den; out.append(q)
    q = np.zeros((4, 2)); q[0, 0] = 5e-324; q[2, 1] = 1e-310; q[3] = [1e-310, 1e-310]; out.append(q)
    # a quad whose every product underflows: the atan2 terms are signed zeros and every edge length is 0; clockwise, all
    # four corner angles come out as 0 (amax == 0), counter-clockwise as 6.2832
    tiny = np.array([[0.0, 0.0], [-1.0, 2.0], [1.0, 3.0], [2.0, 1.0]]) * 1e-170   # edges in quadrants II, I, IV, III
    out += [tiny, tiny[::-1].copy(), (sq - 0.7) * 1e-170, tiny + 1.0e-165]
    return np.array(out)


def _transform(q, scale, shift):
    return q * scale + np.asarray(shift, np.float64)


def classes():
    """[(name, kind, quads)]: kind "well" = compared at the base bar with nothing left out, "derived" = bounds()."""
    out = []
    for base, q in base_classes():
        for tag, scale, shift in TRANSFORMS:
            kind = "well" if base in WELL_BASES and tag in WELL_TRANSFORMS else "derived"
            out.append((base + ("@" + tag if tag else ""), kind, _transform(q, scale, shift)))
    # (extended precision does not model underflow, so it says nothing about the denormal quads: base bar)
    out.append(("non_finite", "well", non_finite()))
    return out


def golden_sample(per_class=14):
    """The quads recorded from the reference: the first per_class of every class and transform, all of non_finite, and
    the sqrt(area) == edge rectangles."""
    names, quads, cid = [], [], []
    for name, _, q in classes():
        n = len(q) if name == "non_finite" else (40 if name == "axis_aligned" else per_class)
        names.append(name)
        quads.append(q[:n]); cid += [len(names) - 1] * len(q[:n])
    return names, np.concatenate(quads), np.array(cid, np.int32)


# ------------------------------------------------------------------------------------------------ oracle side
def oracle_angles(q):
    """The oracle's quantised corner angles [m, 4] (Vertex.to_find_clockwise_angle at vertex i of (i + 1, i - 1))."""
    from oracle.ref_lib import lib
    L = lib()
    q = np.ascontiguousarray(q, np.float64).reshape(-1, 4, 2)
    out = np.empty((len(q), 4))
    for n in range(len(q)):
        for i in range(4):
            s, a, b = q[n, i], q[n, (i + 1) % 4], q[n, i - 1]
            out[n, i] = L.meshenv_ref_cw(s[0], s[1], a[0], a[1], b[0], b[1])
    return out


def oracle_outputs(q):
    """{output name: [m]} of the oracle: the eight record entries and the five indices."""
    from oracle.ref_lib import element_quality, quad_quality
    rec = element_quality(q)
    out = {f"rec{k}": rec[:, k] for k in range(8)}
    for k in INDICES:
        out[f"idx{k}"] = quad_quality(q, k)
    return out


_libm = C.CDLL("libm.so.6")
_libm.pow.restype = C.c_double
_libm.pow.argtypes = [C.c_double, C.c_double]
_pow2_libm = np.frompyfunc(lambda v: _libm.pow(v, 2.0), 1, 1)


def _first_min(cols):
    """min() of a Python list: starts from the first entry, replaced on a true `<` only."""
    r = cols[0]
    for c in cols[1:]:
        r = np.where(c < r, c, r)
    return r


def _first_max(cols):
    r = cols[0]
    for c in cols[1:]:
        r = np.where(c > r, c, r)
    return r


def _records(q, ang, T, sq, sin):
    """The arithmetic of meshenv_ref_element_quality / meshenv_ref_quad_quality in the number type T, from the corner
    angles ang.  Returns {output: [m]} plus the conditioning terms "area_scale" and "ra_minus_e" [m, 4]."""
    q = np.asarray(q, np.float64).astype(T)
    ang = np.asarray(ang, np.float64).astype(T)
    pi, half, one = T(PI), T(0.5), T(1.0)
    x, y = q[:, :, 0], q[:, :, 1]

    def length(dx, dy):
        return np.sqrt(sq(dx) + sq(dy))

    with np.errstate(all="ignore"):
        a = [ang[:, i] for i in range(4)]
        amin, amax = _first_min(a), _first_max(a)
        err = _first_max([np.abs(v - pi / T(2)) for v in a])
        out = {"rec0": amin * (T(180.0) / pi), "rec1": amax * (T(180.0) / pi)}
        e = [length(x[:, i] - x[:, i - 1], y[:, i] - y[:, i - 1]) for i in range(4)]      # e[i] = d(v[i], v[i-1])
        emin, emax = _first_min(e), _first_max(e)
        d0 = length(x[:, 0] - x[:, 2], y[:, 0] - y[:, 2])
        d1 = length(x[:, 1] - x[:, 3], y[:, 1] - y[:, 3])
        p = [(x[:, 0], y[:, 0]), (x[:, 3], y[:, 3]), (x[:, 2], y[:, 2]), (x[:, 1], y[:, 1])]   # p0..p3 = v[0], v[-1], v[-2], v[-3]
        lv = [(p[(i + 1) % 4][0] - p[i][0], p[(i + 1) % 4][1] - p[i][1]) for i in range(4)]      # l0..l3

        def cross(u, v):
            return u[0] * v[1] - v[0] * u[1]

        n = [length(*v) for v in lv]
        den = [n[0] * n[3], n[0] * n[1], n[1] * n[2], n[2] * n[3]]
        term = [cross(lv[3], lv[0]) / den[0], cross(lv[0], lv[1]) / den[1], cross(lv[1], lv[2]) / den[2],
                cross(lv[2], lv[3]) / den[3]]
        sj = _first_min(term)
        for k in (3, 2, 1, 0):      # the reference raises at the first zero denominator: that term's IEEE value
            sj = np.where(den[k] == 0, term[k], sj)
        out["rec2"] = sj
        stretch = np.sqrt(T(2.0)) * emin / np.where(d1 > d0, d1, d0)
        out["rec3"] = stretch
        x1 = ((p[1][0] - p[0][0]) + (p[2][0] - p[3][0]), (p[1][1] - p[0][1]) + (p[2][1] - p[3][1]))
        x2 = ((p[2][0] - p[1][0]) + (p[3][0] - p[0][0]), (p[2][1] - p[1][1]) + (p[3][1] - p[0][1]))
        x12 = ((p[0][0] - p[1][0]) + (p[2][0] - p[3][0]), (p[0][1] - p[1][1]) + (p[2][1] - p[3][1]))
        len1, len2 = length(*x1), length(*x2)
        out["rec4"] = length(*x12) / np.where(len2 < len1, len2, len1)
        out["rec5"] = np.sqrt(stretch * (amin / amax))
        t0, t2 = half * e[0] * e[1] * sin(a[0]), half * e[2] * e[3] * sin(a[2])
        area = t0 + t2
        out["rec6"] = area
        aspect = np.where(emin != 0, emax / emin, T(0.001))
        out["rec7"] = one / (aspect + err)
        out["idx0"], out["idx3"], out["idx4"] = out["rec7"], out["rec3"], out["rec5"]
        pos = ~(area <= 0)          # `if area <= 0: q1 = 0`: a NaN area takes the pow branch
        ra = np.sqrt(np.where(area <= 0, one, area))
        prod = one
        for i in range(4):
            prod = prod * np.where(ra - e[i] > 0, e[i] / ra, one / (e[i] / ra))
        q1 = np.where(pos, np.power(prod, T(0.25)), T(0.0))
        ap = one
        for i in range(4):
            ap = ap * (one - np.abs(a[i] * (T(180.0) / pi) - T(90.0)) / T(90.0))
        q2 = np.where(ap < 0, T(0.0), np.power(np.where(ap < 0, one, ap), T(0.25)))
        out["idx1"] = np.sqrt(q1 * q2)
        fa = [np.abs(v) for v in a]
        out["idx5"] = np.sqrt(q1 * (_first_min(fa) / _first_max(fa)))
        out["area_scale"] = half * (e[0] * e[1] + e[2] * e[3])
        out["ra_minus_e"] = np.stack([np.sqrt(area) - e[i] for i in range(4)], 1)
        out["angle_product"] = ap
        out["emin"] = emin
        out["amax"] = amax
    return out


def ieee_records(q, ang, square="libm"):
    """numpy float64 restatement of the oracle: square = "libm" (pow(v, 2.0): the oracle bit for bit) or "mul" (v * v:
    what the device computes; entries 0-4 are then IEEE operations only)."""
    if square == "libm":
        def sq(v):
            return _pow2_libm(np.asarray(v, np.float64)).astype(np.float64)
    else:
        def sq(v):
            return v * v
    sin = np.frompyfunc(lambda v: _libm_sin(v), 1, 1)
    return _records(q, ang, np.float64, sq, lambda v: sin(v).astype(np.float64))


_libm.sin.restype = C.c_double
_libm.sin.argtypes = [C.c_double]


def _libm_sin(v):
    return _libm.sin(float(v))


def extended(q, ang):
    """The same formulas in np.longdouble (64-bit significand) from the oracle's float64 angles."""
    T = np.longdouble
    return _records(q, ang, T, lambda v: v * v, np.sin)


# ------------------------------------------------------------------------------------------------ bounds
def _scale(name, orc, ext):
    """What a deviation of output `name` is measured against: the value itself; the area against 0.5 (e0 e1 + e2 e3)
    (its two terms may cancel); the two outputs that take a root of the area against the value times the cancellation
    factor area_scale / |area| (their relative error is that of the area, amplified by it)."""
    v = np.abs(orc[name])
    area_scale = np.asarray(ext["area_scale"], np.float64)
    if name == "rec6":
        return np.where(np.isfinite(area_scale), area_scale, v)
    if name in BRANCH_OUTPUTS:
        with np.errstate(all="ignore"):
            amp = area_scale / np.abs(orc["rec6"])
        return v * np.where(np.isfinite(amp) & (amp > 1), amp, 1.0)
    return v


def bounds(q, kind, orc=None, ang=None):
    """Per output the allowed |device - oracle| [m], the measured oracle deviation D (relative to _scale, class maximum)
    and the mask of items left out of BRANCH_OUTPUTS.

    well:    rtol 1e-12 |oracle| + 1e-13 (area: of its scale), nothing left out.
    derived: D = max over the class of |oracle - extended| / scale; allowed = (4 D + 1e-12) scale + 1e-13.  The factor 4:
             ocml and libm may each differ from the exact value in the last two bits of sin and of pow, compounded
             through one product and one root.
    An item is AMBIGUOUS when the oracle's |area| lies inside the area's own bound while its two terms are not both
    exactly zero: the device may then take the other side of `area <= 0`.  (angle_product is a product of IEEE
    operations on the quantised angles and ra - e only picks between x and 1 / (1 / x) at x = 1 +- rounding: neither is
    a discontinuity between device and oracle.)"""
    # The scaled Jacobian (rec2) and the taper (rec4) are a cross product / a difference of parallel vectors on the
    # collinear classes: D reaches O(1) there and the allowance constrains nothing.  They are IEEE operations only and
    # are compared bit for bit (tests/test_gpu_quality_edges.py); EXACT_OUTPUTS names them so that no ratio is reported.
    orc = orc or oracle_outputs(q)
    ang = oracle_angles(q) if ang is None else ang
    ext = extended(q, ang)
    allowed, dev = {}, {}
    for name in OUTPUTS:
        o = orc[name]
        sc = _scale(name, orc, ext)
        fin = np.isfinite(o) & np.isfinite(np.asarray(ext[name], np.float64)) & np.isfinite(sc)
        with np.errstate(all="ignore"):
            d = np.abs((o.astype(np.longdouble) - ext[name])).astype(np.float64) / np.where(sc > 0, sc, 1.0)
        d = np.where(fin & (sc > 0), d, 0.0)
        dev[name] = float(d.max()) if len(d) else 0.0
        sc0 = np.where(np.isfinite(sc), sc, 0.0)
        allowed[name] = ((FACTOR * dev[name] if kind == "derived" else 0.0) + BASE_RTOL) * sc0 + BASE_ATOL
    area, area_scale = orc["rec6"], np.asarray(ext["area_scale"], np.float64)
    # (the relative part of the bound: the absolute 1e-13 is a convenience of the comparison, not an error the area has)
    ambiguous = (np.isfinite(area) & np.isfinite(area_scale) & (area_scale > 0)
                 & (np.abs(area) <= allowed["rec6"] - BASE_ATOL))
    # both terms exactly zero (a zero edge, or sin(0)): the area is 0 on every conforming implementation
    ambiguous &= ~((area == 0) & _terms_zero(q, ang))
    return allowed, dev, ambiguous


def _terms_zero(q, ang):
    q = np.asarray(q, np.float64)
    e = [np.hypot(q[:, i, 0] - q[:, i - 1, 0], q[:, i, 1] - q[:, i - 1, 1]) for i in range(4)]
    return ((e[0] == 0) | (e[1] == 0) | (ang[:, 0] == 0)) & ((e[2] == 0) | (e[3] == 0) | (ang[:, 2] == 0))


def branches(q, orc=None, ang=None):
    """Which branch of the kernels every item takes, from the oracle's values alone: {name: bool [m]}."""
    orc = orc or oracle_outputs(q)
    ang = oracle_angles(q) if ang is None else ang
    r = ieee_records(q, ang, "libm")
    area = orc["rec6"]
    rme = np.asarray(r["ra_minus_e"], np.float64)
    pos = (area > 0)[:, None]
    return {"emin == 0": np.asarray(r["emin"]) == 0, "area <= 0": area <= 0, "angle_product < 0": np.asarray(r["angle_product"]) < 0,
            "amax == 0": np.asarray(r["amax"]) == 0, "ra - e == 0": (pos & (rme == 0)).any(1), "ra - e < 0": (pos & (rme < 0)).any(1),
            "ra - e > 0": (pos & (rme > 0)).any(1)}


def same_class(dev, orc):
    """Non-finite values agree in class: NaN where the oracle has NaN, the same signed infinity otherwise."""
    dev, orc = np.asarray(dev), np.asarray(orc)
    return (np.isnan(dev) == np.isnan(orc)) & (np.isposinf(dev) == np.isposinf(orc)) & (np.isneginf(dev) == np.isneginf(orc))
