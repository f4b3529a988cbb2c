"""CPU: the oracle's quality measures on degenerate, concave, inverted, non-finite and transformed quads against the
reference's own methods (tests/golden/quality_edge_quads.npz, recorded by oracle/gen_golden.py --quality-edges-only), and
the conditions the GPU comparison (tests/test_gpu_quality_edges.py) rests on, all from the oracle alone:

* where the reference returns a value the oracle returns the same bits; where it raises (ZeroDivisionError, ValueError)
  the oracle's IEEE value is non-finite -- that value is the device's specification;
* the numpy restatement of tests/quality_ref.py is the oracle bit for bit (with libm's pow(v, 2.0) as the square), so its
  v * v form is a sound expectation for the device's IEEE-only entries;
* every class takes the branch it is named for, the classes together reach every branch of the kernels, and at most
  0.1 % of a class (none of a well-conditioned one) sits where the device may take the other side of `area <= 0`.
"""
import functools
import os

import numpy as np

import quality_ref as Q
from conftest import GOLDEN_DIR


def _ulps(a, b):
    a = np.asarray(a, np.float64).view(np.int64); b = np.asarray(b, np.float64).view(np.int64)
    a = np.where(a < 0, np.int64(-2 ** 63) - a, a); b = np.where(b < 0, np.int64(-2 ** 63) - b, b)
    return np.abs(a - b)


def test_oracle_equals_the_reference_on_edge_quads():
    z = np.load(os.path.join(GOLDEN_DIR, "quality_edge_quads.npz"))
    names, quads, cid = Q.golden_sample()
    assert list(z["class_names"]) == names and np.array_equal(z["class_id"], cid)
    assert np.array_equal(z["quad_xy"], quads, equal_nan=True), "the generator no longer gives the recorded inputs"
    assert 300 <= len(quads) <= 2000
    orc = Q.oracle_outputs(quads)
    got = np.stack([orc[f"rec{k}"] for k in range(8)] + [orc[f"idx{k}"] for k in z["index"]], 1)
    exp = np.concatenate([z["record"], z["index_value"]], 1)
    raised = np.concatenate([z["record_raised"], z["index_raised"]], 1).astype(bool)
    finite_in = np.isfinite(quads).all(axis=(1, 2))
    assert raised.sum() > 500 and (~raised).sum() > 10000
    # where the reference raises, the oracle's IEEE value is non-finite; on finite input exactly there
    assert not np.isfinite(got[raised]).any(), np.argwhere(raised & np.isfinite(got))[:10]
    assert np.isfinite(exp[finite_in][~raised[finite_in]]).all()
    assert np.isfinite(got[finite_in][~raised[finite_in]]).all()
    same = (got == exp) | (np.isnan(got) & np.isnan(exp))
    off = ~same & ~raised
    # another libm's pow may round differently: at most one ulp, never on the two angle entries (no pow in them)
    print(f"oracle vs reference: {int(off.sum())} of {int((~raised).sum())} values differ (a different libm pow)")
    assert not off[:, :2].any()
    assert (_ulps(got[off], exp[off]) <= 1).all(), np.argwhere(off)[:10]
    # the recording itself was made with the libm the oracle was written against: no difference is expected there
    assert off.sum() <= 0.01 * off.size


@functools.lru_cache(maxsize=None)
def _per_class():
    out = []
    for name, kind, q in Q.classes():
        orc, ang = Q.oracle_outputs(q), Q.oracle_angles(q)
        _, dev, amb = Q.bounds(q, kind, orc, ang)
        out.append((name, kind, q, orc, ang, dev, amb, Q.branches(q, orc, ang)))
    return out


def test_numpy_restatement_is_the_oracle_bit_for_bit():
    for name, kind, q, orc, ang, *_ in _per_class():
        r = Q.ieee_records(q, ang, "libm")
        for k in [f"rec{i}" for i in range(8)] + ["idx0", "idx3", "idx4"]:
            v = np.asarray(r[k], np.float64)
            assert (((v == orc[k]) & (np.signbit(v) == np.signbit(orc[k]))) | (np.isnan(v) & np.isnan(orc[k]))).all(), (name, k)


def test_classes_take_their_branches_and_stay_inside_the_ambiguity_cap():
    covered = {}
    for name, kind, q, orc, ang, dev, amb, br in _per_class():
        base, _, tag = name.partition("@")
        frac = amb.mean()
        print(f"{name:34s} {kind:8s} m={len(q):5d} ambiguous={int(amb.sum())}  oracle deviation "
              + " ".join(f"{k}={dev[k]:.1e}" for k in Q.OUTPUTS))
        assert frac <= Q.AMBIGUOUS_CAP, name
        if kind == "well":
            assert not amb.any(), name
        for k, v in br.items():
            covered[k] = covered.get(k, 0) + int(v.sum())
        if tag in ("dx1e6", "d1e8"):      # a shift rounds the coordinates: the class keeps its name, not its exact shape
            continue
        reflex = ang > Q.PI
        sin0, sin2 = np.sin(ang[:, 0]), np.sin(ang[:, 2])
        named = {
            "well_formed": lambda: (~reflex).all() and (orc["rec6"] > 0).all() and not br["angle_product < 0"].any(),
            "concave": lambda: (reflex.sum(1) == 1).all() and br["angle_product < 0"].all(),
            "self_intersecting": lambda: (sin0 * sin2 < 0).all() and (reflex.sum(1) == 2).all(),
            "reversed": lambda: reflex.all() and br["area <= 0"].all(),
            "one_zero_edge": lambda: br["emin == 0"].all() and np.isnan(orc["rec2"]).all() and (orc["rec7"] > 0).all(),
            "two_zero_edges": lambda: br["emin == 0"].all() and br["area <= 0"].all(),
            "coincident_opposite": lambda: (orc["rec3"] > 0).all() and (np.hypot(*(q[:, 0] - q[:, 2]).T) * np.hypot(*(q[:, 1] - q[:, 3]).T) == 0).all(),
            "all_coincident": lambda: br["emin == 0"].all() and (orc["rec6"] == 0).all() and np.isnan(orc["rec3"]).all(),
            "three_collinear": lambda: (np.abs(ang - Q.PI).min(1) < 1.01e-4).all(),
            "all_collinear": lambda: (np.minimum(np.minimum(ang, np.abs(ang - Q.PI)), np.abs(ang - 2 * Q.PI)) < 1.01e-4).all(),
            "near_degenerate": lambda: ((np.abs(ang - Q.PI).min(1) < 1.1e-3) | (orc["rec3"] < 1e-5)).all(),
            "axis_aligned": lambda: (ang == round(Q.PI / 2, 4)).all() and (orc["rec4"] == 0).all(),
            "kite_trapezoid": lambda: (np.abs(np.asarray(Q.ieee_records(q, ang)["ra_minus_e"])).min(1)
                                       <= 1e-3 * np.sqrt(orc["rec6"])).all(),
            "non_finite": lambda: (~np.isfinite(q).all((1, 2)) | (np.abs(q) < 1e-160).any((1, 2))).all(),
        }
        assert named[base](), name
    print("branch coverage:", covered)
    for k in ("emin == 0", "area <= 0", "angle_product < 0", "amax == 0", "ra - e == 0", "ra - e < 0"):
        assert covered[k] > 0, k
