"""Crafted element logs for the topology report: the meshes tests/test_topology_cpu.py checks the host restatement on and
tests/test_gpu_topology_crafted.py hands to the kernel through meshenv_topology_selftest.  Pure Python / numpy.

Every record keeps the kernel's contract (include/meshenv_topology.h): four distinct ids, each < n0 + n_new.  A case is
(group, name, quads [n, 4], n0, n_new); ids are unified (domain vertex i -> i, k-th generated vertex -> n0 + k)."""
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def case(group, name, quads, n0, n_new=None):
    q = np.asarray(quads, np.int32).reshape(-1, 4)
    top = int(q.max()) + 1 if len(q) else 0
    if n_new is None:
        n_new = max(top - n0, 0)
    assert n0 >= 3 and n0 + n_new >= top and (len(q) == 0 or q.min() >= 0)
    assert all(len(set(r)) == 4 for r in q.tolist()), name           # the contract
    return (group, name, q, int(n0), int(n_new))


# ---------------------------------------------------------------------------------------------- the hand meshes
HAND = {
    "one_quad": ([[0, 1, 2, 3]], 4),
    "two_by_two_grid": ([[0, 1, 8, 7], [1, 2, 3, 8], [8, 3, 4, 5], [7, 8, 5, 6]], 8),
    "three_around_a_vertex": ([[0, 1, 2, 6], [2, 3, 4, 6], [4, 5, 0, 6]], 6),
    "fan_on_one_edge": ([[0, 1, 2, 3], [0, 1, 4, 5], [0, 1, 6, 7]], 4),
    "unfinished_ring": ([[9, 0, 1, 10]], 10),
}


def hand_cases():
    return [case("hand", k, q, n0) for k, (q, n0) in HAND.items()]


# ---------------------------------------------------------------------------------------------- the reference's meshes
def reference_cases():
    """(cases, recorded [M, 3] = num_elements, num_vertices, Singularity of the reference's calculate_metrics): every mesh
    of tests/golden/quality_topology_reference.npz (oracle/gen_topology_golden.py) and the one of plot_boundary0_biased_s1.npz,
    which the former file records once more as its last mesh: the reference's numbers for it."""
    fx = np.load(os.path.join(GOLDEN_DIR, "quality_topology_reference.npz"))
    off = fx["elem_offsets"]
    cases = [case("reference", f"{fx['domains'][fx['domain'][m]]}_step{fx['step'][m]}", fx["quads"][off[m]:off[m + 1]], fx["n0"][m])
             for m in range(len(fx["n0"]))]
    recorded = [fx["live"][m][::-1].tolist() for m in range(len(fx["n0"]))]
    plot = np.load(os.path.join(GOLDEN_DIR, "plot_boundary0_biased_s1.npz"))
    cases.append(case("reference", "plot_boundary0_biased_s1", plot["quads"], int(plot["n0"])))
    assert np.array_equal(cases[-1][2], cases[-2][2])
    recorded.append(recorded[-1])
    return cases, np.array(recorded, np.int32)


# ---------------------------------------------------------------------------------------------- edge uses and valence
def book(k, n0=4):
    """k quads [v, a, x_j, b] on the domain vertices v = 0, a = 1, b = n0 - 1 with generated x_j: distinct as sets; the
    edges (v, a) and (b, v) are used k times, v, a and b are in k elements.  a and b are neighbours of every x_j."""
    return [[0, 1, n0 + j, n0 - 1] for j in range(k)]


def bounded_book(k, n0=4):
    """k distinct quads [v, p, x, q] around the generated vertex v = n0 in which NO vertex has more than 16 neighbours, so
    that an element count past 255 is reported and not refused: p, q out of 16 generated vertices (v's neighbours), x out
    of 15 more (p then has v and at most 15 x).  120 pairs x 15 = 1800 distinct records at the most."""
    v, N, X = n0, [n0 + 1 + i for i in range(16)], [n0 + 17 + i for i in range(15)]
    out = []
    for x in X:
        for i in range(16):
            for j in range(i + 1, 16):
                out.append([v, N[i], x, N[j]])
    assert k <= len(out)
    return out[:k]


BOOK_256_ON_4 = [0, 256, 259, 3, 256, 0, 0, 0, 0, 0, 0, 3, 514, 512, 2, 516]    # the restatement without max_degree


def edge_use_cases():
    return [case("edge_uses", f"edge_book_{k}", book(k), 4) for k in range(1, 6)]


def valence_cases():
    out = [case("valence", f"valence_book_{k}", book(k, 5), 5) for k in range(1, 10)]
    out += [case("valence", f"bounded_book_{k}", bounded_book(k), 4) for k in (9, 254, 255, 256, 300)]
    # 14 pages: a and b have 16 neighbours (v, their other ring neighbour, 14 x); 15 pages and the 256 of the literal: refused
    out += [case("valence", f"book_{k}_on_4", book(k), 4) for k in (14, 15, 256)]
    return out


# ---------------------------------------------------------------------------------------------- degree
def wheel(m, centre, first, closed):
    """m quads [c, r_i, o_i, r_(i+1)] around c: closed -> m spokes (r_m = r_0), open -> m + 1.  Ids from `first` on."""
    n_r = m if closed else m + 1
    r = [first + i for i in range(n_r)]
    o = [first + n_r + i for i in range(m)]
    return [[centre, r[i], o[i], r[(i + 1) % n_r]] for i in range(m)]


def degree_cases():
    out = []
    for m in (15, 16, 17, 18):                       # generated centre: m neighbours
        out.append(case("degree", f"closed_wheel_{m}", wheel(m, 6, 7, True), 6))
    for m in (14, 15, 16, 17):                       # m + 1 neighbours
        out.append(case("degree", f"open_fan_{m}", wheel(m, 6, 7, False), 6))
    for spokes in (14, 15):                          # domain vertex 0: ring neighbours 1 and 5 + `spokes` generated ones
        out.append(case("degree", f"domain_vertex_{spokes}_spokes", wheel(spokes - 1, 0, 6, False), 6))
    # domain vertex 0 with 16 spokes of which the first and the last are its ring neighbours 5 and 1: 16 neighbours, not 18
    q = wheel(15, 0, 6, False)
    sub = {6: 5, 21: 1}
    out.append(case("degree", "ring_neighbours_are_element_neighbours", [[sub.get(v, v) for v in r] for r in q], 6))
    # ... and one spoke more: refused
    q = wheel(16, 0, 6, False)
    sub = {6: 5, 22: 1}
    out.append(case("degree", "ring_neighbours_and_15_more", [[sub.get(v, v) for v in r] for r in q], 6))
    # a mesh between two refused ones (the order of the list is the order of the launch)
    out.append(case("degree", "grid_between_refusals", HAND["two_by_two_grid"][0], 8))
    out.append(case("degree", "closed_wheel_20", wheel(20, 6, 7, True), 6))
    return out


# ---------------------------------------------------------------------------------------------- lane seams
def chain(lo, hi):
    """Quads [j, j+1, j+2, j+3] for j = lo .. hi - 4: every id of [lo, hi) is used, valences 1..4, edges with 1, 2 and 3 uses."""
    return [[j, j + 1, j + 2, j + 3] for j in range(lo, hi - 3)]


def tripod(s, others):
    """Three quads around s: s is in 3 elements (the only singular vertex), others[0:3] in 2, others[3:6] in 1."""
    a, b = others[:3], others[3:6]
    return [[s, a[0], b[0], a[1]], [s, a[1], b[1], a[2]], [s, a[2], b[2], a[0]]]


def seam_cases():
    out = []
    for nv in (63, 64, 65, 127, 128, 129, 193):
        out.append(case("seams", f"chain_nv{nv}_n0_30", chain(0, nv), 30, nv - 30))
        out.append(case("seams", f"chain_nv{nv}_all_domain", chain(0, nv), nv, 0))                      # n_new = 0
        out.append(case("seams", f"chain_nv{nv}_tail_unused", chain(0, nv - 5), 30, nv - 30))
        for s in sorted({63, 64, nv - 1}):
            if s < nv:
                near = dict.fromkeys((0, 1, 31, 62, 63, 64, 65, nv - 2, nv - 3, 2, 3, 4))       # distinct, in this order
                others = [v for v in near if v != s and v < nv][:6]
                out.append(case("seams", f"singular_at_{s}_of_{nv}", tripod(s, others), 30, nv - 30))
    for n0 in (64, 128):                              # the ring edge n0-1 -> 0 joins the last pass and the first
        out.append(case("seams", f"closing_edge_n0_{n0}", [[n0 - 1, 0, n0, n0 + 1]], n0))
        out.append(case("seams", f"closing_edge_n0_{n0}_all_domain", [[n0 - 1, 0, 1, 2], [n0 - 2, n0 - 1, 0, 5]], n0, 0))
        out.append(case("seams", f"closing_edge_n0_{n0}_chain", chain(0, n0 + 9) + [[n0 - 1, 0, n0 + 9, n0 + 10]], n0))
    return out


def empty_cases():
    return [case("empty", f"empty_n0_{n0}_new_{n_new}", [], n0, n_new) for n0, n_new in ((3, 0), (30, 0), (64, 0), (65, 7), (128, 64))]


def repeated_cases():
    base = [0, 1, 2, 3]
    out = [case("repeated", "same_order", [base, base], 4), case("repeated", "rotated", [base, [2, 3, 0, 1]], 4),
           case("repeated", "reversed", [base, [3, 2, 1, 0]], 4), case("repeated", "three_times", [base, base, [1, 2, 3, 0]], 4),
           case("repeated", "inside_a_grid", HAND["two_by_two_grid"][0] + [[8, 3, 4, 5], [5, 4, 3, 8]], 8)]
    return out


def wide_cases():
    """n0 = 40000, n_new = 20: ids past 32767 in the unsigned short slots."""
    n0 = 40000
    q = chain(39990, 40020) + [[n0 - 1, 0, n0, n0 + 1], [39995, 40019, 1, 40010]]
    return [case("wide", "ids_around_40000", q, n0, 20), case("wide", "empty_wide", [], n0, 20)]


# ---------------------------------------------------------------------------------------------- seeded random soups
SOUPS, SOUP_SEED = 200, 20240


def soup_cases():
    """200 meshes of E <= 60 records of four distinct ids out of a pool of P <= 40 vertices over a ring of n0: shared edges,
    high valences and full slot arrays are common.  A pool of at most 17 vertices cannot overflow the 16 slots; a large E
    on a large pool nearly always does."""
    rng = np.random.default_rng(SOUP_SEED)
    out = []
    for i in range(SOUPS):
        n0 = int(rng.integers(3, 21))
        P = int(rng.integers(max(n0, 4), 41))
        E = int(rng.integers(0, 61))
        q = [rng.choice(P, 4, replace=False).tolist() for _ in range(E)]
        out.append(case("soup", f"soup_{i}_n0_{n0}_P_{P}_E_{E}", q, n0, P - n0))
    return out


def shared_cases():
    """Everything that fits one launch of a common width (the wide ids have launches of their own)."""
    return (reference_cases()[0] + hand_cases() + edge_use_cases() + valence_cases() + degree_cases() + seam_cases() + empty_cases() +
            repeated_cases() + soup_cases())
