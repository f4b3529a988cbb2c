"""CPU: the host restatement of the topology report (tests/topology_ref.py) on a reference-recorded mesh and on hand meshes,
the aggregation of topology_report, and the packaging of include/meshenv_topology.h.  Nothing here needs a GPU."""
import os
import re

import numpy as np
import pytest

import topology_cases as TC
import topology_ref as TR
from conftest import GOLDEN_DIR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _second_way(quads, n0):
    """The same 16 numbers from array operations (np.unique / np.bincount) instead of the restatement's loops: no dedup
    (the callers pass meshes without repeated elements)."""
    q = np.asarray(quads, np.int64).reshape(-1, 4)
    val = np.bincount(q.ravel(), minlength=n0)
    used = val[val > 0]
    e = np.stack([q, np.roll(q, 1, axis=1)], axis=2).reshape(-1, 2)
    e.sort(axis=1)
    _, uses = np.unique(e, axis=0, return_counts=True)
    ring = np.stack([np.arange(n0), (np.arange(n0) + 1) % n0], axis=1)
    ring.sort(axis=1)
    _, both = np.unique(np.concatenate([e, ring]), axis=0, return_counts=True)
    hist = [int((used == k).sum()) for k in range(1, 8)] + [int((used >= 8).sum())]
    return np.array([0, len(q), len(used), int((~np.isin(used, (1, 2, 4))).sum()), *hist, len(uses), int((uses == 1).sum()),
                     int((uses > 2).sum()), int((both % 2 == 1).sum())], np.int32), val


def test_reference_recorded_mesh():
    fx = np.load(os.path.join(GOLDEN_DIR, "plot_boundary0_biased_s1.npz"))
    quads, n0 = fx["quads"], 30
    rep, val = TR.topology(quads, n0)
    assert rep.dtype == np.int32 and rep.shape == (16,) and val.dtype == np.uint8
    assert rep[:4].tolist() == [0, 42, 58, 20]
    assert rep[4:12].tolist() == [5, 20, 15, 13, 4, 1, 0, 0]
    assert rep[12:].tolist() == [99, 30, 0, 0]
    assert TR.euler(rep) == 1
    rep2, val2 = _second_way(quads, n0)
    assert rep.tolist() == rep2.tolist()
    assert val.tolist() == val2.tolist() and len(val) == int(quads.max()) + 1
    # a closed mesh of a disc: every ring edge is used once, every interior edge twice
    assert rep[13] == n0 and 4 * rep[1] == 2 * (rep[12] - rep[13]) + rep[13]
    padded, pv = TR.topology(quads, n0, width=200)
    assert padded.tolist() == rep.tolist() and len(pv) == 200 and not pv[len(val):].any()


def test_restatement_equals_the_reference_on_its_own_meshes():
    """tests/golden/quality_topology_reference.npz (oracle/gen_topology_golden.py): the reference's calculate_metrics over the live
    objects of its own env at every episode end, complete or not -- Singularity / num_vertices / num_elements are words 3 /
    2 / 1.  Where the reference's writer did not raise, its text reader (generate_meshes) finds n0 - 1 vertices more, all
    with no element: the B21 boundary-element lines of the file, read as vertices."""
    fx = np.load(os.path.join(GOLDEN_DIR, "quality_topology_reference.npz"))
    off, M = fx["elem_offsets"], len(fx["n0"])
    assert off[0] == 0 and off[-1] == len(fx["quads"]) and fx["quads"].dtype == np.int32
    assert int(fx["complete"].sum()) >= 5 and int((fx["complete"] == 0).sum()) >= 5 and len(set(fx["domain"].tolist())) >= 2
    assert 0 < int(fx["raised"].sum()) < M
    for m in range(M):
        quads, n0 = fx["quads"][off[m]:off[m + 1]], int(fx["n0"][m])
        assert len(quads) > 0
        rep, val = TR.topology(quads, n0)
        assert rep[0] == 0 and [int(rep[3]), int(rep[2]), int(rep[1])] == fx["live"][m].tolist(), m
        assert len(TR.dedup(quads.tolist())) == len(quads), m                      # dedup removes nothing
        for kw in (dict(dedup=False), dict(dedup=False, max_degree=16)):
            rep2, val2 = TR.topology(quads, n0, **kw)
            assert rep2.tolist() == rep.tolist() and val2.tolist() == val.tolist(), (m, kw)
        assert rep.tolist() == _second_way(quads, n0)[0].tolist(), m
        unused = n0 - int((val[:n0] > 0).sum())
        if fx["raised"][m]:
            assert unused > 0 and fx["from_file"][m].tolist() == [-1, -1, -1], m   # the writer looks every domain vertex up
        else:
            assert unused == 0, m
            assert (fx["from_file"][m] - fx["live"][m]).tolist() == [n0 - 1, n0 - 1, 0], m
        if fx["complete"][m]:
            assert rep[15] == 0 and rep[14] == 0 and rep[13] == n0 and TR.euler(rep) == 1, m
    # the mesh of the plotting fixture is the last one recorded: the reference's numbers for it
    plot = np.load(os.path.join(GOLDEN_DIR, "plot_boundary0_biased_s1.npz"))["quads"]
    assert np.array_equal(fx["quads"][off[M - 1]:], plot) and fx["live"][M - 1].tolist() == [20, 58, 42]


def test_golden_regenerates_from_the_reference():
    """oracle/gen_topology_golden.py --check in a process of its own (it stubs modules): what it records today is the
    committed file.  Needs the reference's sources, which only the machine that records fixtures has."""
    import subprocess
    import sys
    sys.path.insert(0, ROOT)
    try:
        from oracle.ref_harness import REFERENCE_ROOT, reference_available
    finally:
        sys.path.pop(0)
    if not (reference_available() and os.path.exists(os.path.join(REFERENCE_ROOT, "general", "post_processing.py"))):
        pytest.skip("the reference's sources are not on this machine")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "oracle", "gen_topology_golden.py"), "--check"], capture_output=True,
                         text=True)
    assert run.returncode == 0 and "regenerated == committed" in run.stdout, run.stdout + run.stderr


def _rep(quads, n0):
    rep, val = TR.topology(quads, n0)
    if len(TR.dedup(quads)) == len(quads):
        assert rep.tolist() == _second_way(quads, n0)[0].tolist()
    return dict(zip(("status", "elements", "vertices", "singularity"), rep[:4].tolist()), hist=rep[4:12].tolist(),
                edges=int(rep[12]), boundary=int(rep[13]), nonmanifold=int(rep[14]), front=int(rep[15]), euler=TR.euler(rep),
                valence=val.tolist())


def test_one_quad():
    r = _rep([[0, 1, 2, 3]], 4)
    assert (r["elements"], r["vertices"], r["singularity"]) == (1, 4, 0)
    assert r["hist"] == [4, 0, 0, 0, 0, 0, 0, 0] and r["valence"] == [1, 1, 1, 1]
    assert (r["edges"], r["boundary"], r["nonmanifold"], r["front"], r["euler"]) == (4, 4, 0, 0, 1)


def test_two_by_two_grid():
    # ring 0..7 clockwise around the square, vertex 8 = the centre (generated)
    r = _rep([[0, 1, 8, 7], [1, 2, 3, 8], [8, 3, 4, 5], [7, 8, 5, 6]], 8)
    assert (r["elements"], r["vertices"], r["singularity"]) == (4, 9, 0)
    assert r["valence"] == [1, 2, 1, 2, 1, 2, 1, 2, 4] and r["hist"] == [4, 4, 0, 1, 0, 0, 0, 0]
    assert (r["edges"], r["boundary"], r["nonmanifold"], r["front"], r["euler"]) == (12, 8, 0, 0, 1)


def test_three_quads_around_an_interior_vertex():
    # hexagon ring 0..5, vertex 6 inside: the only vertex with three elements
    r = _rep([[0, 1, 2, 6], [2, 3, 4, 6], [4, 5, 0, 6]], 6)
    assert (r["elements"], r["vertices"], r["singularity"]) == (3, 7, 1)
    assert r["valence"] == [2, 1, 2, 1, 2, 1, 3] and r["hist"] == [3, 3, 1, 0, 0, 0, 0, 0]
    assert (r["edges"], r["boundary"], r["nonmanifold"], r["front"], r["euler"]) == (9, 6, 0, 0, 1)


def test_repeated_element_is_removed():
    once = _rep([[0, 1, 2, 3]], 4)
    twice = _rep([[0, 1, 2, 3], [2, 3, 0, 1]], 4)     # equal SORTED vertex ids: post_processing.py:27-32
    assert twice == once


def test_edge_shared_by_three_elements():
    # three quads that all contain the edge (0, 1): a fan, not a surface
    r = _rep([[0, 1, 2, 3], [0, 1, 4, 5], [0, 1, 6, 7]], 4)
    assert r["nonmanifold"] == 1 and r["elements"] == 3 and r["vertices"] == 8
    assert r["valence"][:2] == [3, 3] and r["singularity"] == 2
    assert r["edges"] == 10 and r["boundary"] == 9


def test_unfinished_mesh_on_a_ring():
    # ring of 10, one element cut off at the corner 0 with a generated vertex 10: the front is 1 - 10 - 9 and the rest of the ring
    r = _rep([[9, 0, 1, 10]], 10)
    assert (r["elements"], r["vertices"]) == (1, 4)          # the six unused domain vertices are not counted
    assert r["valence"] == [1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 1]
    assert r["front"] == 10 and r["boundary"] == 4           # ring edges 1-2 .. 8-9 (8) + the two new edges
    assert r["singularity"] == 0


def test_counted_as_logged():
    """dedup=False: a repeated record counts twice -- what the kernel documents."""
    for _, name, q, n0, _ in TC.repeated_cases():
        kept, _ = TR.topology(q, n0)
        raw, val = TR.topology(q, n0, dedup=False)
        assert raw[1] == len(q) > kept[1] and raw.tolist() != kept.tolist(), name
        assert raw.tolist() == _second_way(q, n0)[0].tolist(), name                # bincount / unique do not dedup either
    twice, val = TR.topology([[0, 1, 2, 3], [2, 3, 0, 1]], 4, dedup=False)
    assert twice.tolist() == [0, 2, 4, 0, 0, 4, 0, 0, 0, 0, 0, 0, 4, 0, 0, 4] and val.tolist() == [2, 2, 2, 2]
    for _, name, q, n0, _ in TC.hand_cases() + TC.seam_cases() + TC.edge_use_cases():
        a, b = TR.topology(q, n0), TR.topology(q, n0, dedup=False)
        assert a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist(), name


def test_max_degree():
    """max_degree=16: more than 16 distinct neighbours -- ring neighbours of a domain vertex included, used or not -- give
    [3, 0, ...] and a zero row; at most 16 change nothing."""
    refused = np.array([3] + [0] * 15)
    expect = {"closed_wheel_15": 0, "closed_wheel_16": 0, "closed_wheel_17": 3, "closed_wheel_18": 3, "closed_wheel_20": 3,
              "open_fan_14": 0, "open_fan_15": 0, "open_fan_16": 3, "open_fan_17": 3, "domain_vertex_14_spokes": 0,
              "domain_vertex_15_spokes": 3, "ring_neighbours_are_element_neighbours": 0, "ring_neighbours_and_15_more": 3,
              "grid_between_refusals": 0, "book_14_on_4": 0, "book_15_on_4": 3, "book_256_on_4": 3, "bounded_book_255": 0,
              "bounded_book_256": 0, "bounded_book_300": 0}
    seen = {}
    for _, name, q, n0, n_new in TC.degree_cases() + TC.valence_cases() + TC.hand_cases():
        free, fval = TR.topology(q, n0, dedup=False)
        rep, val = TR.topology(q, n0, dedup=False, max_degree=16, width=n0 + n_new + 3)
        assert free[0] == 0 and free.tolist() == _second_way(q, n0)[0].tolist(), name
        seen[name] = int(rep[0])
        if rep[0] == 3:
            assert rep.tolist() == refused.tolist() and not val.any() and len(val) == n0 + n_new + 3, name
        else:
            assert rep.tolist() == free.tolist() and val[:len(fval)].tolist() == fval.tolist() and not val[len(fval):].any(), name
        assert TR.topology(q, n0, dedup=False, max_degree=10 ** 6)[0].tolist() == free.tolist(), name
    assert {k: seen[k] for k in expect} == expect
    assert all(seen[k] == 0 for k in TC.HAND)
    # the wheel's centre: exactly m neighbours
    for m in (15, 16, 17):
        q = TC.wheel(m, 6, 7, True)
        assert TR.topology(q, 6, max_degree=m)[0][0] == 0 and TR.topology(q, 6, max_degree=m - 1)[0][0] == 3


def test_books():
    """Edge uses 1..5 and element counts 1..9 and past 255 on the host."""
    for k in range(1, 6):
        rep, val = TR.topology(TC.book(k), 4, dedup=False, max_degree=16)
        # edges (v, a) and (b, v) with k uses, 2 k page edges with one; the ring 0-1-2-3-0 adds one use to (0, 1) and (3, 0)
        assert rep[12] == 2 + 2 * k and rep[13] == 2 * k + (2 if k == 1 else 0) and rep[14] == (2 if k > 2 else 0), k
        assert rep[15] == 2 * k + 2 + (2 if k % 2 == 0 else 0), k
        assert val.tolist() == [k, k, 0, k] + [1] * k
    for k in range(1, 10):
        rep, val = TR.topology(TC.book(k, 5), 5, dedup=False, max_degree=16)
        hist = [0] * 8
        hist[0] += k
        hist[min(k, 8) - 1] += 3
        assert rep[0] == 0 and rep[4:12].tolist() == hist and rep[3] == (0 if k in (1, 2, 4) else 3), k
    rep, val = TR.topology(TC.book(256), 4, dedup=False)
    assert rep.tolist() == TC.BOOK_256_ON_4 and val.tolist() == [255, 255, 0, 255] + [1] * 256
    for k in (255, 256, 300):
        rep, val = TR.topology(TC.bounded_book(k), 4, dedup=False, max_degree=16)
        assert rep[0] == 0 and rep[1] == k and val[4] == 255 and val.max() == 255 and rep[11] >= 1, k
        assert rep.tolist() == _second_way(TC.bounded_book(k), 4)[0].tolist()


def test_soups_reach_both_statuses():
    cases = TC.soup_cases()
    status = [int(TR.topology(q, n0, dedup=False, max_degree=16)[0][0]) for _, _, q, n0, _ in cases]
    assert len(cases) == 200 and set(status) == {0, 3}
    assert status.count(0) >= 50 and status.count(3) >= 20, (status.count(0), status.count(3))


def test_aggregation():
    from reinforcementlearning4meshgeneration_amd.evaluation import TOPOLOGY_FIELDS, topology_report
    assert len(TOPOLOGY_FIELDS) == 16 and TOPOLOGY_FIELDS[0] == "status" and TOPOLOGY_FIELDS[3] == "singularity"
    a, _ = TR.topology(np.load(os.path.join(GOLDEN_DIR, "plot_boundary0_biased_s1.npz"))["quads"], 30)
    b, _ = TR.topology([[0, 1, 8, 7], [1, 2, 3, 8], [8, 3, 4, 5], [7, 8, 5, 6]], 8)
    c, _ = TR.topology([[9, 0, 1, 10]], 10)
    d, _ = TR.topology([[0, 1, 2, 3], [0, 1, 4, 5], [0, 1, 6, 7]], 4)
    empty = np.zeros(16, np.int32)
    skipped = [np.eye(16, dtype=np.int32)[0] * s for s in (1, 2, 2, 4)]
    rep = topology_report(np.stack([a, empty, b, c, d] + skipped))
    assert rep["meshes"] == 4 and rep["elements"] == 42 + 4 + 1 + 3 and rep["vertices"] == 58 + 9 + 4 + 8
    s = np.array([20, 0, 0, 2])
    assert rep["singularity"] == dict(average=float(s.mean()), std=float(s.std()), min=0, max=20, total=22)
    assert rep["singular_fraction"] == 22 / 79
    assert rep["valence_histogram"] == (a[4:12] + b[4:12] + c[4:12] + d[4:12]).tolist()
    assert rep["closed"] == 2 and rep["nonmanifold"] == 1        # c and d have edges with an odd use count
    assert rep["euler"] == [1, 1, 1, TR.euler(d)]
    assert rep["skipped"] == {1: 1, 2: 2, 4: 1}
    nothing = topology_report(np.zeros((0, 16), np.int32))
    assert nothing["meshes"] == 0 and nothing["euler"] == [] and nothing["skipped"] == {} and nothing["singularity"]["total"] == 0
    assert np.isnan(nothing["singular_fraction"]) and nothing["valence_histogram"] == [0] * 8


def test_eval_result_without_topology():
    from reinforcementlearning4meshgeneration_amd.evaluation import EvalResult
    rec = dict(env=[1, 0], domain=[0, 0], step=[5, 5], length=[6, 6], flags=[1, 0], n_elements=[3, 0],
               **{"return": [1.0, 2.0], "return_raw": [1.0, 2.0]})
    res = EvalResult.from_records(rec, [1, 1], 6, True)
    assert res.topology is None and res.env.tolist() == [0, 1]
    with pytest.raises(ValueError):
        res.topology_report()
    z = np.zeros(2)
    direct = EvalResult(z, z, z, z, z, z, z, z, z, z, None, z, 6, True)          # the fourteen fields of before, positionally
    assert direct.topology is None and direct.finished is True
    a, _ = TR.topology([[0, 1, 2, 3]], 4)
    rec["topology"] = np.stack([a, np.zeros(16, np.int32)])                       # rows in slot order: env 1 first
    res = EvalResult.from_records(rec, [1, 1], 6, True)
    assert res.topology.dtype == np.int32 and res.topology.shape == (2, 16)
    assert res.topology[1].tolist() == a.tolist() and not res.topology[0].any()   # sorted with the other fields
    assert res.topology_report()["meshes"] == 1


def test_exports_and_header():
    from reinforcementlearning4meshgeneration_amd import _capi, build
    from reinforcementlearning4meshgeneration_amd.vec_env import MeshVecEnv
    names = _capi.EXPORTS_TOPOLOGY
    assert sorted(names) == ["meshenv_eval_set_topology", "meshenv_mesh_topology", "meshenv_topology_selftest"]
    header = open(os.path.join(ROOT, "include", "meshenv_topology.h")).read()
    defines = dict(re.findall(r"#define\s+(MESHENV_[A-Z_]+)\s+(\d+)", header))
    assert int(defines["MESHENV_TOPOLOGY_DIM"]) == _capi.TOPOLOGY_DIM == len(MeshVecEnv.TOPOLOGY_FIELDS) == TR.DIM == 16
    assert [int(defines["MESHENV_TOPO_" + k]) for k in ("OK", "MASKED", "LOG_OVERFLOW", "DEGREE", "NOT_ARCHIVED")] == \
        [_capi.TOPO_OK, _capi.TOPO_MASKED, _capi.TOPO_LOG_OVERFLOW, _capi.TOPO_DEGREE, _capi.TOPO_NOT_ARCHIVED]
    kernels = open(os.path.join(ROOT, "reinforcementlearning4meshgeneration_amd", "csrc", "meshenv_topology.h")).read()
    assert "k_mesh_topology" in kernels and "k_eval_topology" in kernels and "k_topology_selftest" in kernels
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import source_state
    finally:
        sys.path.pop(0)
    assert source_state.PUBLIC_HEADERS == build.PUBLIC_HEADERS
