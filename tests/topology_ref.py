"""Host restatement of the topology report (include/meshenv_topology.h, csrc/meshenv_topology.h) in numpy / pure Python.
Nothing here touches a device.

Written from the reference's general/post_processing.py:
  * :81-89 (generate_mesh_from_inp) and :27-32 (generate_meshes): an element whose SORTED vertex ids were seen before is
    dropped -- `if vs not in existing_eles`;
  * :145-151 (calculate_metrics, 'Singularity'): per vertex the number of elements with `v in ele.vertices` (identity: Vertex
    defines no __eq__), then the vertices whose count is not 4, 2 or 1;
  * :155-159: num_vertices = len(vertices), num_elements = len(elements).
The vertex list is that of the route the reference's results table takes, final_metrics -> generate_mesh_from_inp: meshio's
points, i.e. the *NODE list of write_generated_elements_2_file, which holds the vertices contained in at least one element
(unused domain vertices of an unfinished mesh are not counted).  The reference's other reader, the text reader generate_meshes
(:15-36), takes every line without a leading `*` and with at most four fields for a vertex -- also the n0 - 1 B21
boundary-element lines the writer emits -- so on the reference's own files it reports n0 - 1 more vertices, all with element
count 0 and therefore n0 - 1 more singularities.  That is recorded (tests/golden/quality_topology_reference.npz, `from_file`)
and not imitated.  The writer itself raises ValueError on a mesh that leaves a domain vertex unused (it looks every domain vertex up in
the *NODE list); the counts here are defined for such a mesh as well (the fixture's `live` columns: calculate_metrics over the
live objects).

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


_dedup = dedup      # topology() has an option of the same name


def topology(quads, n0, width=None, dedup=True, max_degree=None):
    """(report int32 [16], valence uint8 [width]) of the mesh quads [n, 4] (unified vertex ids: domain vertex i -> i, k-th
    generated vertex -> n0 + k) on a domain ring of n0 vertices.  width (default: largest id + 1, at least n0) pads the
    valence vector with zeros.  dedup=False: the elements are counted as given, a repeated record twice -- what the kernel
    documents.  max_degree=16: ([3, 0, ..., 0], zeros) when a vertex has more than max_degree distinct neighbours -- the
    vertices it shares an element edge with and, for a domain vertex, its two ring neighbours whether or not an element uses
    them (the kernel's status 3: its slot array is full)."""
    elements = np.asarray(quads, np.int64).reshape(-1, 4).tolist()
    if dedup:
        elements = _dedup(elements)
    top = max([n0] + [max(e) + 1 for e in elements])
    width = top if width is None else int(width)
    assert width >= top
    if max_degree is not None:
        neighbours = {v: {(v - 1) % n0, (v + 1) % n0} for v in range(n0)}
        for e in elements:
            for i in range(4):
                neighbours.setdefault(e[i], set()).add(e[i - 1])
                neighbours.setdefault(e[i - 1], set()).add(e[i])
        if any(len(nb) > max_degree for nb in neighbours.values()):
            report = np.zeros(DIM, np.int32)
            report[0] = 3
            return report, np.zeros(width, np.uint8)
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
