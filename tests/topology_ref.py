"""Host restatement of the topology report (include/meshenv_topology.h, csrc/meshenv_topology.h) in numpy / pure Python.
Nothing here touches a device.

Written from the reference's general/post_processing.py:
  * :27-32 (generate_meshes) and :81-89 (generate_mesh_from_inp): an element whose SORTED vertex ids were seen before is
    dropped -- `if vs not in existing_eles`;
  * :145-151 (calculate_metrics, 'Singularity'): per vertex the number of elements with `v in ele.vertices` (identity: Vertex
    defines no __eq__), then the vertices whose count is not 4, 2 or 1;
  * :155-159: num_vertices = len(vertices), num_elements = len(elements).
The vertex list of the reference is the *NODE list of write_generated_elements_2_file, which holds the vertices contained in
at least one element: unused domain vertices of an unfinished mesh are not counted.

The edge rules are those of the report: an element contributes the four edges (v[i], v[i-1]); "uses" of an edge are the
elements that contain it; the domain ring 0 - 1 - ... - (n0-1) - 0 contributes one further use to each of its edges for
front_edges only."""
from collections import Counter

import numpy as np

DIM = 16


def dedup(quads):
    """post_processing.py:27-32: the elements in order, without those whose sorted vertex ids were seen before."""
    existing_eles, out = [], []
    for q in quads:
        vs = sorted(int(v) for v in q)
        if vs not in existing_eles:
            out.append([int(v) for v in q])
            existing_eles.append(vs)
    return out


def topology(quads, n0, width=None):
    """(report int32 [16], valence uint8 [width]) of the mesh quads [n, 4] (unified vertex ids: domain vertex i -> i, k-th
    generated vertex -> n0 + k) on a domain ring of n0 vertices.  width (default: largest id + 1, at least n0) pads the
    valence vector with zeros."""
    elements = dedup(np.asarray(quads, np.int64).reshape(-1, 4).tolist())
    top = max([n0] + [max(e) + 1 for e in elements])
    width = top if width is None else int(width)
    assert width >= top
    # post_processing.py:145-151
    singularity_count = [0] * width
    for e in elements:
        for v in set(e):
            singularity_count[v] += 1
    vertices = [v for v in range(width) if singularity_count[v] > 0]
    report = np.zeros(DIM, np.int32)
    report[1] = len(elements)                                                              # :158
    report[2] = len(vertices)                                                              # :156
    report[3] = sum(1 for v in vertices if singularity_count[v] not in (4, 2, 1))          # :151
    for v in vertices:
        report[4 + min(singularity_count[v], 8) - 1] += 1
    uses = Counter()
    for e in elements:
        for i in range(4):
            a, b = e[i], e[i - 1]
            uses[(min(a, b), max(a, b))] += 1
    report[12] = len(uses)
    report[13] = sum(1 for c in uses.values() if c == 1)
    report[14] = sum(1 for c in uses.values() if c > 2)
    total = Counter(uses)
    for i in range(n0):
        a, b = i, (i + 1) % n0
        total[(min(a, b), max(a, b))] += 1
    report[15] = sum(1 for c in total.values() if c % 2 == 1)
    return report, np.minimum(np.asarray(singularity_count), 255).astype(np.uint8)


def euler(report):
    return int(report[2]) - int(report[12]) + int(report[1])
