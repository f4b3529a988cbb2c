"""TEST INFRASTRUCTURE (container-only): records what the reference's general/post_processing.py counts on meshes the
reference's env generated itself (tests/golden/quality_topology_reference.npz: ids and integers only; the quality_ prefix
keeps the file out of the step-trace fixtures tests/conftest.golden_names lists).

The env is driven as oracle/ref_harness.record_trace drives it.  At every episode end with at least one element:
  * the element list as ids into env.boundary.vertices (domain vertex i -> i, k-th generated vertex -> n0 + k);
  * `live`: Singularity / num_vertices / num_elements of calculate_metrics(nodes, env.generated_meshes, ...), where nodes is
    the node list write_generated_elements_2_file builds (the vertices of the elements in first-occurrence order), over the
    live objects -- unfinished meshes included;
  * `raised`: whether write_generated_elements_2_file raised (it looks every domain vertex up in that node list: ValueError
    on a mesh that leaves one unused);
  * `from_file`: where it did not raise, the same three numbers from generate_meshes(file) + calculate_metrics on the written
    file (-1 otherwise).  This is the reference's text reader, which also takes the n0 - 1 B21 boundary-element lines of the
    file for vertices: recorded as the reference's own output, not as something to imitate.

usage: python oracle/gen_topology_golden.py            writes the fixture
       python oracle/gen_topology_golden.py --check    regenerates in memory and compares with the committed fixture"""
from __future__ import annotations

import contextlib
import io
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_harness as H  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "quality_topology_reference.npz")
# (domain, seed of biased_actions, steps, stop at the first complete episode).  The last one is the stream of
# gen_golden.plot_fixture: its first complete mesh is the one of tests/golden/plot_boundary0_biased_s1.npz.
CASES = [("boundary0", 1, 1500, False), ("star", 5, 150, False), ("half_wheel1", 3, 600, False), ("boundary0", 1, 700, True)]
KEYS = ("Singularity", "num_vertices", "num_elements")


def _three(pp, vertices, elements):
    m = pp.calculate_metrics(vertices, elements, {k: [] for k in KEYS}, list(KEYS))
    assert all(len(m[k]) == 1 for k in KEYS)
    return [int(m[k][0]) for k in KEYS]


def record():
    pp, stubbed = H.load_post_processing()
    meshes = []
    for d, (dom, seed, T, until_complete) in enumerate(CASES):
        pts = H.domain_points(dom)
        env = H.make_env(pts)
        env.reset()
        acts = H.biased_actions(seed, T)
        for t in range(T):
            _, _, done, info = env.step(acts[t])
            if not done:
                continue
            if len(env.generated_meshes) > 0:
                table = {id(v): k for k, v in enumerate(env.boundary.vertices)}
                quads = [[table[id(v)] for v in m.vertices] for m in env.generated_meshes]
                nodes = []
                for ele in env.generated_meshes:           # write_generated_elements_2_file's node list
                    nodes.extend([n for n in ele.vertices if n not in nodes])
                live = _three(pp, nodes, env.generated_meshes)
                raised, from_file = 0, [-1, -1, -1]
                with tempfile.TemporaryDirectory() as tmp:
                    path = os.path.join(tmp, "mesh.inp")
                    try:
                        with contextlib.redirect_stdout(io.StringIO()):
                            env.write_generated_elements_2_file(path)
                    except ValueError:
                        raised = 1
                    if not raised:
                        from_file = _three(pp, *pp.generate_meshes(path))
                meshes.append(dict(domain=d, n0=len(pts), step=t, complete=int(bool(info["is_complete"])), quads=quads,
                                   live=live, raised=raised, file=from_file))
                if until_complete and info["is_complete"]:
                    break
            env.reset()
    offsets = np.concatenate([[0], np.cumsum([len(m["quads"]) for m in meshes])]).astype(np.int32)
    out = dict(domains=np.array([c[0] for c in CASES]), seeds=np.array([c[1] for c in CASES], np.int32),
               steps=np.array([c[2] for c in CASES], np.int32),
               domain=np.array([m["domain"] for m in meshes], np.int32), n0=np.array([m["n0"] for m in meshes], np.int32),
               step=np.array([m["step"] for m in meshes], np.int32),
               complete=np.array([m["complete"] for m in meshes], np.uint8),
               elem_offsets=offsets, quads=np.concatenate([np.array(m["quads"], np.int32).reshape(-1, 4) for m in meshes]),
               live=np.array([m["live"] for m in meshes], np.int32), raised=np.array([m["raised"] for m in meshes], np.uint8),
               from_file=np.array([m["file"] for m in meshes], np.int32))
    return out, stubbed


def main():
    out, stubbed = record()
    summary = (f"{len(out['n0'])} meshes, {int(out['complete'].sum())} complete, {int((1 - out['complete']).sum())} unfinished, "
               f"writer raised on {int(out['raised'].sum())}, {len(out['quads'])} elements; stubbed {list(stubbed)}")
    if "--check" in sys.argv[1:]:
        have = np.load(OUT)
        assert sorted(have.files) == sorted(out), (have.files, sorted(out))
        for k in out:
            assert have[k].dtype == out[k].dtype and np.array_equal(have[k], out[k]), k
        print("regenerated == committed:", summary)
        return
    np.savez_compressed(OUT, **out)
    print(summary, "->", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
