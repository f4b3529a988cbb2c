"""CPU: tests/samples_host.extract_samples_2 (the host restatement the GPU tests compare the device kernel with) against the reference's MeshGeneration.extract_samples_2 (general/mesh.py:1438-1489)
on meshes the reference generated (tests/golden/samples_*.npz, oracle/gen_samples_golden.py): same samples in the same
order, value for value (pure Python float arithmetic on both sides)."""
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR
from samples_host import extract_samples_2, reach, scan_corners, segment_lists

NAMES = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN_DIR, "samples_*.npz")))


@pytest.mark.parametrize("name", NAMES)
def test_extract_samples_2_matches_the_reference(name):
    tr = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    nn, nr, rad, idx, thr = tr["params"]
    samples, types, outputs = extract_samples_2(tr["quads"], tr["vertex_xy"], int(tr["n0"]), int(nn), int(nr), rad, index=int(idx),
                                                quality_threshold=float(thr))
    assert len(samples) == len(tr["samples"]) > 50
    assert np.array_equal(np.array(samples, np.float64), tr["samples"])
    assert np.array_equal(np.array(types, np.float64).reshape(-1), tr["types"])
    assert np.array_equal(np.array(outputs, np.float64), tr["outputs"])
    # a path of n_neighbor = 1 is the neighbour alone and never holds the target: the reference can only answer 0.5 there
    assert set(np.unique(tr["types"])) == ({0.0, 0.5, 1.0} if nn > 1 else {0.5})


def test_segment_lists_order_follows_connect_vertices():
    # one quad on a square ring [0, 1, 2, 3] plus a generated vertex 4: element [4, 0, 1, 2] (new vertex first, as B:177-182)
    adj = segment_lists(np.array([[4, 0, 1, 2]]), 5, 4)
    assert adj[0] == [3, 1, 4] and adj[4] == [2, 0] and adj[2] == [1, 3, 4] and adj[1] == [0, 2]


def test_recordings_reach_the_parameter_range_and_the_edge_classes():
    """What the recordings reach, counted with samples_host.reach on each recorded mesh with its recorded parameters: all
    twelve (n_neighbor, n_radius) pairs, both indices, thresholds 0.0 / 0.5 / 0.7, radii from 0.5 to 6, meshes of 20 or
    more elements on rings of 60 or more vertices, no sector beyond the kernel's 32 (one exactly at 32), and each edge
    class at least once: (a) the shared-list case of get_nodes under n_neighbor = 3, (b) equidistant vertices in one sector
    (stable sort order), (c) vertices exactly on a sector's start or end angle (strict inequalities), (d) elements of
    quality exactly 0 taken under threshold 0.0.  reach's sample count is held against the recorded list's length."""
    pairs, indices, thresholds, radii, rings, sectors = set(), set(), set(), set(), set(), []
    total = dict(dead_first=0, ties=0, edge_angles=0, zero_quality=0)
    for name in NAMES:
        tr = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
        nn, nr, rad, idx, thr = tr["params"]
        r = reach(scan_corners(tr["quads"], tr["vertex_xy"], int(tr["n0"])), int(nn), int(nr), float(rad), int(idx), float(thr))
        assert r["rows"] == len(tr["samples"]) <= 20000, (name, r["rows"])
        assert r["max_sector"] <= 32, (name, r["max_sector"])
        sectors.append(r["max_sector"])
        if len(tr["quads"]) >= 20:
            pairs.add((int(nn), int(nr))); indices.add(int(idx)); thresholds.add(float(thr)); radii.add(float(rad))
            rings.add(int(tr["n0"]))
        total["dead_first"] += r["dead_first"] if nn == 3 else 0
        total["zero_quality"] += r["zero_quality"] if thr == 0.0 else 0
        total["ties"] += r["ties"]
        total["edge_angles"] += r["edge_angles"]
    assert pairs == {(a, b) for a in (1, 2, 3) for b in (1, 2, 3, 4)}, sorted(pairs)
    assert indices == {1, 5} and thresholds == {0.0, 0.5, 0.7} and min(radii) == 0.5 and max(radii) == 6.0
    assert len([n for n in rings if n >= 60]) >= 1 and max(sectors) == 32
    assert all(v > 0 for v in total.values()), total
    print(f"recordings reach: {total}, largest sectors {sorted(sectors)}")
