"""GPU: the counting part of k_mesh_topology / k_eval_topology (csrc/meshenv_topology.h: mesh_topology) on element logs written
by hand, through meshenv_topology_selftest -- the paths no mesh of the environment takes: a full slot array (status 3), the
2-bit edge-use counter past its saturation, non-manifold edges, valence bins 6, 7 and >= 8, the uint8 clamp, vertex ids past
32767, the 64-lane loop at multiples of 64, repeated records.  The cases are those of tests/topology_cases.py; every one is
compared integer for integer -- 16 report words and the whole valence row -- with the host restatement
topology_ref.topology(..., dedup=False, max_degree=16).  All cases but the wide ids share one launch.

Every record is inside the kernel's contract (four distinct ids, each < n0 + n_new)."""
import collections

import numpy as np
import pytest

import topology_cases as TC
import topology_ref as TR

pytestmark = pytest.mark.gpu

WIDTH = 321                       # >= the largest n0 + n_new of the shared launch (260), no multiple of 64
CANARY32, CANARY8 = -1234567, 0xA5


def _expected(cases, width):
    rep = np.zeros((len(cases), 16), np.int32)
    val = np.zeros((len(cases), width), np.uint8)
    for i, (_, _, q, n0, _) in enumerate(cases):
        rep[i], val[i] = TR.topology(q, n0, width=width, dedup=False, max_degree=16)
    return rep, val


def _launch(cases, width):
    from reinforcementlearning4meshgeneration_amd import _capi
    rc, rep, val = _capi.topology_selftest([c[2] for c in cases], [c[3] for c in cases], [c[4] for c in cases], width,
                                           valence_fill=CANARY8, report_fill=CANARY32)
    assert rc == 0
    return rep, val


def _compare(cases, got, exp, pick):
    """Report and valence row of the picked cases; returns their statuses."""
    (rep, val), (erep, eval_) = got, exp
    statuses = []
    for i in pick:
        group, name, q, n0, n_new = cases[i]
        assert rep[i].tolist() == erep[i].tolist(), (name, rep[i].tolist(), erep[i].tolist())
        assert np.array_equal(val[i], eval_[i]), (name, np.nonzero(val[i] != eval_[i])[0][:8])
        assert rep[i, 0] in (0, 3) and not val[i, n0 + n_new:].any(), name       # every byte past the last vertex was written
        if rep[i, 0] == 3:
            assert not rep[i, 1:].any() and not val[i].any(), name
        else:
            assert rep[i, 1] == len(q), name
        statuses.append(int(rep[i, 0]))
    return statuses


@pytest.fixture(scope="module")
def shared():
    cases = TC.shared_cases()
    assert max(c[3] + c[4] for c in cases) <= WIDTH
    exp = _expected(cases, WIDTH)
    got = _launch(cases, WIDTH)
    groups = collections.defaultdict(list)
    for i, c in enumerate(cases):
        groups[c[0]].append(i)
    by_name = {c[1]: i for i, c in enumerate(cases)}
    assert len(by_name) == len(cases)
    return cases, got, exp, groups, by_name


def test_every_case_of_the_shared_launch(shared):
    cases, got, exp, groups, _ = shared
    statuses = _compare(cases, got, exp, range(len(cases)))
    count = collections.Counter(statuses)
    per_group = {g: dict(collections.Counter(statuses[i] for i in idx)) for g, idx in groups.items()}
    print(f"crafted logs compared: {len(cases)} meshes, status 0: {count[0]}, status 3: {count[3]}; by group {per_group}")
    assert set(count) == {0, 3} and count[0] >= 100 and count[3] >= 30


def test_reference_meshes(shared):
    cases, got, exp, groups, _ = shared
    _, recorded = TC.reference_cases()
    idx = groups["reference"]
    assert len(idx) == len(recorded) >= 11
    assert _compare(cases, got, exp, idx) == [0] * len(idx)
    # words 1..3 against what the reference itself counted, not only through the restatement
    assert np.array_equal(got[0][idx, 1:4], recorded)
    assert got[0][idx[-1], :4].tolist() == [0, 42, 58, 20]                      # plot_boundary0_biased_s1.npz


def test_hand_meshes(shared):
    cases, got, exp, groups, by_name = shared
    assert _compare(cases, got, exp, groups["hand"]) == [0] * 5
    rep, val = got
    assert rep[by_name["one_quad"]].tolist() == [0, 1, 4, 0, 4, 0, 0, 0, 0, 0, 0, 0, 4, 4, 0, 0]
    assert rep[by_name["two_by_two_grid"]].tolist() == [0, 4, 9, 0, 4, 4, 0, 1, 0, 0, 0, 0, 12, 8, 0, 0]
    assert rep[by_name["three_around_a_vertex"]].tolist() == [0, 3, 7, 1, 3, 3, 1, 0, 0, 0, 0, 0, 9, 6, 0, 0]
    fan = rep[by_name["fan_on_one_edge"]]
    assert fan[14] == 1 and fan[12] == 10 and fan[13] == 9 and fan[3] == 2
    ring = by_name["unfinished_ring"]
    assert rep[ring, 15] == 10 and rep[ring, 13] == 4 and rep[ring, 2] == 4
    assert val[ring, :11].tolist() == [1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 1]


def test_edge_uses_one_to_five(shared):
    """The 2-bit counter saturates at 3, the parity bit goes on toggling."""
    cases, got, exp, groups, by_name = shared
    assert _compare(cases, got, exp, groups["edge_uses"]) == [0] * 5
    for k in range(1, 6):
        r = got[0][by_name[f"edge_book_{k}"]]
        assert r[12] == 2 + 2 * k                                               # (v, a), (b, v) and 2 k page edges
        assert r[13] == 2 * k + (2 if k == 1 else 0)
        assert r[14] == (2 if k > 2 else 0)
        assert r[15] == 2 * k + 2 + (2 if k % 2 == 0 else 0), k                 # ring + k uses: odd for even k


def test_valence_bins_and_clamp(shared):
    cases, got, exp, groups, by_name = shared
    idx = groups["valence"]
    statuses = _compare(cases, got, exp, idx)
    rep, val = got
    name_of = {cases[i][1]: i for i in idx}
    for k in range(1, 10):
        r = rep[name_of[f"valence_book_{k}"]]
        hist = [0] * 8
        hist[0] += k
        hist[min(k, 8) - 1] += 3
        assert r[0] == 0 and r[4:12].tolist() == hist, k
        assert val[name_of[f"valence_book_{k}"], :5].tolist() == [k, k, 0, 0, k]
    for k in (254, 255, 256, 300):
        i = name_of[f"bounded_book_{k}"]
        assert rep[i, 0] == 0 and rep[i, 1] == k and val[i, 4] == min(k, 255) and rep[i, 11] >= 1, k
    # the plain book of 14 pages fills the 16 slots of a and b exactly; 15 and 256 pages are refused: the restatement's
    # numbers for the 256-page book (TC.BOOK_256_ON_4) are out of the kernel's reach, the clamp is reached by the bounded books
    assert [int(rep[name_of[f"book_{k}_on_4"], 0]) for k in (14, 15, 256)] == [0, 3, 3]
    assert statuses.count(3) == 2


def test_degree(shared):
    cases, got, exp, groups, _ = shared
    idx = groups["degree"]
    _compare(cases, got, exp, idx)
    status = {cases[i][1]: int(got[0][i, 0]) for i in idx}
    assert status == {"closed_wheel_15": 0, "closed_wheel_16": 0, "closed_wheel_17": 3, "closed_wheel_18": 3,
                      "open_fan_14": 0, "open_fan_15": 0, "open_fan_16": 3, "open_fan_17": 3,
                      "domain_vertex_14_spokes": 0, "domain_vertex_15_spokes": 3,
                      "ring_neighbours_are_element_neighbours": 0, "ring_neighbours_and_15_more": 3,
                      "grid_between_refusals": 0, "closed_wheel_20": 3}
    # the mesh between two refused ones is the 2x2 grid, untouched by its neighbours in the launch
    order = [cases[i][1] for i in idx]
    g = idx[order.index("grid_between_refusals")]
    assert got[0][g - 1, 0] == 3 and got[0][g + 1, 0] == 3
    assert got[0][g].tolist() == [0, 4, 9, 0, 4, 4, 0, 1, 0, 0, 0, 0, 12, 8, 0, 0]


def test_lane_seams(shared):
    cases, got, exp, groups, _ = shared
    idx = groups["seams"]
    assert _compare(cases, got, exp, idx) == [0] * len(idx)
    assert {cases[i][3] + cases[i][4] for i in idx} >= {63, 64, 65, 127, 128, 129, 193}
    for i in idx:
        name = cases[i][1]
        if name.startswith("singular_at_"):
            s = int(name.split("_")[2])
            assert got[0][i, 3] == 1 and got[0][i, 2] == 7 and got[1][i, s] == 3, name
            assert np.nonzero(got[1][i] == 3)[0].tolist() == [s], name
        if name in ("closing_edge_n0_64", "closing_edge_n0_128"):
            # one quad on the ring edge n0-1 -> 0: that edge is closed, the quad's three other edges are front
            assert got[0][i, 15] == cases[i][3] - 1 + 3 and got[0][i, 13] == 4, name


def test_empty(shared):
    cases, got, exp, groups, _ = shared
    assert _compare(cases, got, exp, groups["empty"]) == [0] * len(groups["empty"])
    for i in groups["empty"]:
        assert got[0][i].tolist() == [0] * 15 + [cases[i][3]], cases[i][1]       # the whole ring is front


def test_repeated_records_count_twice(shared):
    cases, got, exp, groups, _ = shared
    idx = groups["repeated"]
    assert _compare(cases, got, exp, idx) == [0] * len(idx)
    for i in idx:
        _, name, q, n0, _ = cases[i]
        removed = TR.topology(q, n0, width=WIDTH, dedup=True, max_degree=16)
        assert got[0][i].tolist() != removed[0].tolist() and not np.array_equal(got[1][i], removed[1]), name
        assert got[0][i, 1] == len(q) > removed[0][1], name


def test_random_soups(shared):
    cases, got, exp, groups, _ = shared
    idx = groups["soup"]
    assert len(idx) == 200
    # computed from the restatement alone
    want = [int(exp[0][i, 0]) for i in idx]
    assert want.count(0) >= 50 and want.count(3) >= 20 and set(want) == {0, 3}
    assert _compare(cases, got, exp, idx) == want
    live = [i for i in idx if exp[0][i, 0] == 0]
    assert exp[0][live, 14].max() > 0 and exp[0][live, 11].max() > 0 and exp[1][live].max() >= 8    # not trivial ones


@pytest.mark.parametrize("width", [65535, 40020], ids=["width_65535", "width_exact"])
def test_wide_ids(width):
    cases = TC.wide_cases()
    exp = _expected(cases, width)
    got = _launch(cases, width)
    assert _compare(cases, got, exp, range(len(cases))) == [0, 0]
    assert got[0][0, 1] == len(cases[0][2]) and got[1][0, 39990:40020].min() >= 1 and got[1][0, 1] == 1
    assert got[0][1].tolist() == [0] * 15 + [40000]


def test_refusals():
    from reinforcementlearning4meshgeneration_amd import _capi
    L = _capi.load()
    q = np.array([[0, 1, 2, 4]], np.int32)
    off, n0, n_new = np.array([0, 1], np.int32), np.array([4], np.int32), np.array([1], np.int32)
    rep = np.full((1, 16), CANARY32, np.int32)
    val = np.full((1, 70000), CANARY8, np.uint8)

    def call(width, off=off, q=q, n0=n0, n_new=n_new, rep=rep, val=val, n=1):
        ptr = [None if a is None else a.ctypes.data for a in (off, q, n0, n_new)]
        return L.meshenv_topology_selftest(0, n, *ptr, width, None if rep is None else rep.ctypes.data,
                                           None if val is None else val.ctypes.data)

    assert call(4) == _capi.E_ARG                      # width < n0 + n_new
    assert call(65536) == _capi.E_ARG and call(70000) == _capi.E_ARG and call(0) == _capi.E_ARG
    for name in ("off", "q", "n0", "n_new", "rep"):
        assert call(5, **{name: None}) == _capi.E_ARG, name
    assert call(5, n=0) == _capi.E_ARG
    assert call(5, q=np.array([[0, 1, 2, 5]], np.int32)) == _capi.E_ARG          # an id outside the mesh
    assert (rep == CANARY32).all() and (val == CANARY8).all()                    # nothing was written by a refused call
    assert call(5, val=None) == 0 and rep[0].tolist() == TR.topology(q, 4, dedup=False, max_degree=16)[0].tolist()
    assert call(5) == 0 and val[0, :5].tolist() == [1, 1, 1, 0, 1] and (val[0, 5:] == CANARY8).all()
    rc, _, _ = _capi.topology_selftest([q], [4], [1], 4)
    assert rc == _capi.E_ARG
