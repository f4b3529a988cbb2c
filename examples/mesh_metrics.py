#!/usr/bin/env python
"""The reference's results table (general/post_processing.py:93-161, metrics_4_domains / final_metrics) for meshes generated
on the device: per domain the quality measures (Element quality = 'robust', Stretch, Taper, Scaled Jacobian, MinAngle,
MaxAngle) beside Singularity, num_vertices and num_elements -- the first six from one k_element_quality launch, the last three
from one k_mesh_topology launch, nothing pulled to the host per env.

The meshes come from random-policy episodes (biased uniform actions, no trained checkpoint ships with the package): every env
keeps stepping with auto-reset and the table scores the last FINISHED episode of each env.

    python examples/mesh_metrics.py [--envs 256] [--steps 600] [--seed 0]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# reference column -> (MeshVecEnv.QUALITY_MEASURES name)
QUALITY_COLUMNS = (("Element quality", "robust"), ("Stretch", "stretch"), ("Taper", "taper"), ("Scaled Jacobian", "scaled_jacobian"),
                   ("MinAngle", "min_angle_deg"), ("MaxAngle", "max_angle_deg"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256, help="environments per domain")
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import torch

    from reinforcementlearning4meshgeneration_amd import MeshVecEnv, boundary, random_domain

    d1 = np.load(os.path.join(ROOT, "tests", "golden", "boundary16_biased_s2.npz"))["domain_xy"]   # ui/domains/boundary16.json
    domains = {"boundary(0)": boundary(0), "boundary16 (d1)": [tuple(p) for p in d1], "random_domain(8)": random_domain(8)}
    rng = np.random.default_rng(args.seed)
    n = args.envs
    header = ["domain", "meshes", "closed"] + [c for c, _ in QUALITY_COLUMNS] + ["Singularity", "num_vertices", "num_elements"]
    table = []
    for name, dom in domains.items():
        env = MeshVecEnv([dom], n_envs=n, log_capacity=256)
        env.reset()
        for _ in range(args.steps):
            a = rng.uniform([-1, -1.5, 0], [1, 1.5, 1.5], size=(n, 3))
            pick = rng.random(n) < 0.6
            a[pick] = np.stack([rng.uniform(-1, 1, n), rng.uniform(0.2, 1.0, n), rng.uniform(0.3, 1.2, n)], axis=1)[pick]
            env.step(torch.from_numpy(a.astype(np.float32)).cuda())
        quality = env.quality_report("last")
        topo = env.topology_report("last")
        row = [name, str(topo["meshes"]), str(topo["closed"])]
        for _, measure in QUALITY_COLUMNS:
            row.append(f"{quality[measure]['average']:.3f}" if measure in quality else "-")
        m = max(topo["meshes"], 1)
        row += [f"{topo['singularity']['average']:.2f}", f"{topo['vertices'] / m:.1f}", f"{topo['elements'] / m:.1f}"]
        table.append(row)
        print(f"{name}: valence histogram (1..7, >=8 elements per vertex) {topo['valence_histogram']}, singular fraction "
              f"{topo['singular_fraction']:.3f}, non-manifold meshes {topo['nonmanifold']}, skipped {topo['skipped']}")
        env.close()
    widths = [max(len(r[i]) for r in [header] + table) for i in range(len(header))]
    for r in [header] + table:
        print("  ".join(c.ljust(w) for c, w in zip(r, widths)))


if __name__ == "__main__":
    main()
