"""CPU: the x-slab pre-filter of the observation scan (long rings, csrc/meshenv_kernels.h find_next_state stage C),
restated in Python floats and searched against the oracle's bisector / fan-slot tests on adversarial positions.

The filter keeps a ring position when its edge's x-extent meets ref.x +- W, W = slab_half_width(target_length);
it may drop a position only when the unfiltered scan gives it nothing: neither a fan slot (d(ref, v) < target_length)
nor a hit of the bisector segment ref -> p_s (Segment.intersection_vertex, oracle/meshenv_ref.c).  The search places
edges a few ulp inside and outside the slab and the bisector's end with the reference vertex at |x| from 1 to 1e9,
where the rounding of ref.x + qx in u = p_s - ref and of the slab bounds follow |ref.x| rather than the edge.  The half width
is restated here (Python floats are IEEE doubles, never fused); the GPU self-test (tests/test_gpu_geometry_range.py,
meshenv_selftest 17) evaluates the same cases with the kernel's slab_half_width / slab_keeps and must agree with this
restatement case by case."""
import math

import numpy as np


def slab_half_width(ref_x, target_length):
    """slab_half_width() of csrc/meshenv_kernels.h: target_length (1 + 1e-9) + 1e-9, whatever |ref.x|."""
    return target_length * (1 + 1e-9) + 1e-9


def narrow_half_width(ref_x, target_length):
    """A slack narrower than the bisector: not exact, the search must say so."""
    return target_length * (1 - 1e-7)


def bisector_hits(ref, u, v, b):
    """Segment(ref, ref + u).intersection_vertex(Segment(v, b)) is not None (oracle/meshenv_ref.c, C:657-676)."""
    ux, uy = u
    wx, wy = b[0] - v[0], b[1] - v[1]
    if wy == 0:
        if uy == 0:
            return False
        s = (v[1] - ref[1]) / uy
        h = (ref[0] - v[0] + s * ux) / wx
    elif wx == 0:
        if ux == 0:
            return False
        s = (v[0] - ref[0]) / ux
        h = (ref[1] - v[1] + s * uy) / wy
    else:
        den = uy / wy - ux / wx
        if den == 0:
            return False
        s = ((ref[0] - v[0]) / wx - (ref[1] - v[1]) / wy) / den
        h = (ref[0] - v[0] + s * ux) / wx
    return 0 < s < 1 and 0 < h < 1


def cases():
    """(ref, (qx, qy), target_length, v, b): reference vertices at |x| = 1 .. 1e9 (both signs, off-grid mantissas and
    powers of two), bisectors along +-x and slightly tilted, edges across the bisector's line whose nearer end sits
    k = 1 .. 8 ulp beyond the slab bound and k = -4 .. 4 ulp around the bisector's end fl(ref.x + qx), vertical and
    slanted away."""
    rng = np.random.default_rng(5)
    hw_new = slab_half_width
    for e in range(0, 10):
        for sign in (1.0, -1.0):
            for frac in (0.0, 0.37, float(rng.uniform(0.1, 0.9)), None):
                rx = sign * (10.0 ** e * (1 + frac) if frac is not None else 2.0 ** (3 * e + 1))
                ry = float(rng.uniform(-3, 3))
                for tl in (0.0004, 0.4, 1.0, 4.0, 4.0004, 40.0):
                    for alpha in (0.0, 1e-3, 0.3):
                        for d in (1.0, -1.0):
                            q = (d * tl * math.cos(alpha), tl * math.sin(alpha))
                            xs = []
                            for hw in (hw_new, narrow_half_width):
                                x = rx + d * hw(rx, tl)          # the slab bound, as rounded
                                for _ in range(8):
                                    x = math.nextafter(x, d * math.inf)
                                    xs.append(x)
                            x = rx + q[0]                        # the bisector's end, as rounded
                            for _ in range(4):
                                x = math.nextafter(x, -d * math.inf)
                            for _ in range(9):
                                xs.append(x)
                                x = math.nextafter(x, d * math.inf)
                            for x in xs:
                                yield (rx, ry), q, tl, (x, ry - 1.0), (x, ry + 1.0)              # vertical edge
                                yield (rx, ry), q, tl, (x, ry - 1.0), (x + d * 1e-3, ry + 1.0)   # slanted, away


def search(half_width):
    """Positions the filter with this half width drops although the unfiltered scan would count them."""
    dropped, checked, counted = [], 0, 0
    for ref, q, tl, v, b in cases():
        ux = (ref[0] + q[0]) - ref[0]
        uy = (ref[1] + q[1]) - ref[1]
        W = half_width(ref[0], tl)
        lo, hi = ref[0] - W, ref[0] + W
        keep = min(v[0], b[0]) <= hi and max(v[0], b[0]) >= lo
        hit = bisector_hits(ref, (ux, uy), v, b)
        fan = math.sqrt((ref[0] - v[0]) ** 2 + (ref[1] - v[1]) ** 2) < tl
        checked += 1
        counted += int(hit or fan)
        if (hit or fan) and not keep:
            dropped.append((ref, q, tl, v, b))
    return dropped, checked, counted


def test_kernel_slab_filter_drops_no_counted_position():
    dropped, checked, counted = search(slab_half_width)
    assert checked > 50000 and counted > 1000, (checked, counted)   # the cases reach positions the scan counts
    assert not dropped, (len(dropped), dropped[:3])


def test_search_finds_a_too_narrow_slab():
    """The search has teeth: a slab narrower than the bisector drops hits at every magnitude."""
    dropped, _, _ = search(narrow_half_width)
    mags = {int(math.floor(math.log10(abs(r[0])))) for r, *_ in dropped}
    assert set(range(0, 10)) <= mags, sorted(mags)
