"""CPU: the case table of tests/density_cases.py covers what tests/test_gpu_density_rings.py is meant to reach.  Every
case goes through the host restatement (domains.density_domain, pinned to the reference by tests/test_domains_cpu.py)
and the table's own coverage is asserted here, so that the GPU test cannot pass by a class having gone missing: vertex
counts on both sides of every 64-lane trip, repeated pixels before and after their originals, negative point counts,
float pixels, both branches of the clockwise rule, the last edge popping and not popping, every raising kind, statuses
2 and 3."""
import collections

import density_cases as DC


def _count(pred):
    return sum(1 for c, e in DC.table() if pred(c, e))


def test_table_is_deterministic_and_within_the_entry_points_limits():
    a, b = DC.build_cases(), DC.build_cases()
    assert a == b and len(a) == len(DC.table())
    for c, e in DC.table():
        assert 3 <= len(c.pixels) <= DC.MAX_VERTS
        assert all(d >= 0.0 for d in c.densities) and c.base_length > 0
        if e.status == 0:
            assert 4 <= len(e.ring) <= DC.MAX_RING and len(e.ring) % 2 == 0, c.name      # every defined ring is even
    by_status = collections.Counter(e.status for _, e in DC.table())
    print("cases by status:", dict(by_status), "of", len(DC.table()))


def test_vertex_counts_on_both_sides_of_every_64_lane_trip():
    for m in DC.SEAM_COUNTS:
        n = _count(lambda c, e: "seam" in c.tags and e.status == 0 and e.distinct == m == len(c.pixels))
        assert n >= 8, (m, n)
    assert max(len(e.ring) for _, e in DC.table() if e.status == 0) == DC.MAX_RING


def test_every_class_has_defined_cases():
    want = {
        "repeat": lambda c, e: "repeat" in c.tags and e.distinct < len(c.pixels),
        "repeat, second dedupe trip": lambda c, e: "repeat" in c.tags and e.distinct < len(c.pixels) and len(c.pixels) > 64,
        "float": lambda c, e: "float" in c.tags,
        "float with a repeat": lambda c, e: "float" in c.tags and e.distinct < len(c.pixels),
        "negative": lambda c, e: e.negative,
        "input clockwise": lambda c, e: e.reversed is False,
        "input counter-clockwise": lambda c, e: e.reversed is True,
        "pop": lambda c, e: e.pop is True,
        "no pop": lambda c, e: e.pop is False,
    }
    for name, pred in want.items():
        n = _count(lambda c, e: e.status == 0 and pred(c, e))
        print(f"{name}: {n} defined cases")
        assert n >= 8, (name, n)
    # both branches of the clockwise rule and of the pop on rings of more than 64 vertices, too
    for pred in (lambda e: e.reversed, lambda e: not e.reversed, lambda e: e.pop, lambda e: not e.pop):
        assert _count(lambda c, e: e.status == 0 and e.distinct > 64 and pred(e)) >= 8
    rep = [c for c, e in DC.table() if "repeat" in c.tags and e.status == 0]
    assert sum("copy_before" in c.tags for c in rep) >= 4 and sum("copy_after" in c.tags for c in rep) >= 4
    for c in rep:      # every copy carries a density its pixel's other occurrences do not have
        seen = collections.defaultdict(list)
        for p, d in zip(c.pixels, c.densities):
            seen[p].append(d)
        assert all(len(set(v)) == len(v) for v in seen.values()), c.name
    # a negative count on the last edge: its only point is the one the pop removes
    assert _count(lambda c, e: e.status == 0 and e.negative and DC.edge_counts(c)[-1] < 0 and e.pop) >= 1


def test_raising_and_refused_cases():
    for kind in DC.RAISE_KINDS:
        n = _count(lambda c, e: kind in c.tags and e.status == 1)
        assert n >= 3, (kind, n)
        assert _count(lambda c, e: kind in c.tags and e.status != 1) == 0, kind
    assert _count(lambda c, e: "zero_defined" in c.tags and e.status == 0) >= 3
    sq = [e for c, e in DC.table() if c.name == "zero_single_0"][0]
    assert sq.status == 0 and len(sq.ring) == 120
    neg = [e for c, e in DC.table() if c.name == "neg_issue_example"][0]
    assert neg.status == 0 and len(neg.ring) == 68 and neg.negative
    assert _count(lambda c, e: "status2" in c.tags and e.status == 2) >= 2
    assert _count(lambda c, e: "status2" in c.tags and e.status != 2) == 0
    assert _count(lambda c, e: "status3" in c.tags and e.status == 3) >= 2
    assert _count(lambda c, e: ("status3" in c.tags) != (e.status == 3)) == 0
    assert _count(lambda c, e: "full_ring" in c.tags and e.status == 0 and len(e.ring) == DC.MAX_RING) == 2
