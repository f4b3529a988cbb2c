#!/usr/bin/env python
"""Meshing with the supervised element-extraction network (the reference's "FNN mesher", general/EBRD.py:525-579) on the device:

    state = env.reset(static=True)
    while not done:  action, type = get_action(state, model);  state, _, done, info = env.move(action, round(type, 2))
    env.smooth(env.boundary.vertices, ...)                                      # EBRD.py:566, on the complete meshes

for three built-in domains and for 4096 random domains, as ``MeshVecEnv.mesh_with(FusedFNN)``: one forward launch and one move
per step for ALL envs, finished envs frozen where they ended, the host looking at the device once every 32 moves.  Then what
the reference does with the result, on the running episodes of the same handle: smoothing of the complete meshes, the quality
and topology tables, and the training samples extract_samples_2 would take from them.

NO TRAINED NETWORK SHIPS with this package: the reference holds no weights file.  Without --weights the network is a randomly
initialised one whose action bias is set to a plausible point; it extracts some elements and closes almost no domain, so the
tables below mostly show that the machinery runs.  With --weights file.pt (a ``torch.save(model.state_dict())`` of EBRD.py:320)
the same script meshes with a trained network.

    python examples/fnn_meshing.py [--weights file.pt] [--seed 1] [--envs 4096] [--max-steps 400]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def random_policy(seed):
    """A module of the reference's shape (fc1 .. fc5, action_head, type_head) with torch's default initialisation."""
    import torch
    import torch.nn as nn
    torch.manual_seed(seed)
    net = nn.Module()
    for name, n_in, n_out in (("fc1", 18, 64), ("fc2", 64, 128), ("fc3", 128, 64), ("fc4", 64, 32), ("fc5", 32, 16),
                              ("action_head", 16, 2), ("type_head", 16, 3)):
        setattr(net, name, nn.Linear(n_in, n_out))
    with torch.no_grad():
        net.action_head.bias.copy_(torch.tensor([0.25, 0.85]))      # (radius fraction, angle) inside move()'s useful range
    return net


def report(name, env, res):
    import torch
    complete = res.complete != 0
    sweeps, _ = env.smooth(mask=complete, which="current")           # EBRD.py:566: only finished meshes can be smoothed
    smoothed = int((sweeps[complete] >= 0).sum()) if bool(complete.any()) else 0
    quality = env.quality_report("current")
    topo = env.topology_report("current")
    few = torch.arange(env.num_envs, device=env.device) < 16          # (extract_samples_2 takes ~1000 samples per element)
    _, _, _, offsets, _ = env.extract_samples(which="current", mask=few)
    steps = res.steps.cpu().numpy()
    print(f"== {name}: {env.num_envs} envs, {res.total_steps} vector steps")
    print(f"   finished {int(res.finished.sum())}, complete {int(complete.sum())} (complete rate {res.complete_rate:.4f}), "
          f"smoothed {smoothed}; moves per env: median {int(np.median(steps))}, max {int(steps.max())}")
    codes = torch.bincount(res.code.long(), minlength=5).cpu().numpy()
    print(f"   last move codes (OK, NONE, RAISES, NEEDS_SMOOTHING, SMOOTH_RAISES): {codes[:5].tolist()}; elements per env: "
          f"mean {float(res.n_elements.float().mean()):.1f}, max {int(res.n_elements.max())}")
    if quality["meshes"]:
        print("   quality_report: " + ", ".join(f"{k} {quality[k]['average']:.3f}" for k in ("robust", "stretch", "taper", "scaled_jacobian",
                                                                                             "min_angle_deg", "max_angle_deg")))
    print(f"   topology_report: meshes {topo['meshes']}, elements {topo['elements']}, vertices {topo['vertices']}, closed "
          f"{topo['closed']}, non-manifold {topo['nonmanifold']}, singular fraction {topo['singular_fraction']:.3f}")
    print(f"   extract_samples: {int(offsets[-1])} training samples in the meshes of the first {int(few.sum())} envs")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--weights", help="torch.save(model.state_dict()) of a trained network (EBRD.py:320)")
    ap.add_argument("--seed", type=int, default=1, help="seed of the randomly initialised network (without --weights) and of the domains")
    ap.add_argument("--envs", type=int, default=4096, help="random domains")
    ap.add_argument("--max-steps", type=int, default=400)
    args = ap.parse_args()
    import torch

    from reinforcementlearning4meshgeneration_amd import FusedFNN, MeshVecEnv, boundary, random_domain

    if args.weights:
        fnn = FusedFNN.from_state_dict(torch.load(args.weights, map_location="cpu"))
        print(f"network: {args.weights}")
    else:
        fnn = FusedFNN.from_module(random_policy(args.seed))
        print(f"network: random initialisation, seed {args.seed} -- NOT a trained mesher (none ships: the reference holds no weights)")

    d1 = np.load(os.path.join(ROOT, "tests", "golden", "boundary16_biased_s2.npz"))["domain_xy"]   # ui/domains/boundary16.json
    env = MeshVecEnv([boundary(0), [tuple(p) for p in d1], random_domain(8)], auto_reset=False, log_capacity=1024)
    report("boundary(0), boundary16, random_domain(8)", env, env.mesh_with(fnn, max_steps=args.max_steps))
    env.close()

    env = MeshVecEnv.from_random(args.envs, seed=1000 * args.seed, auto_reset=False, log_capacity=512)
    res = env.mesh_with(fnn, max_steps=args.max_steps, check_every=32)
    report(f"random_domain({1000 * args.seed} + k)", env, res)
    # one env, as the reference would look at it: the mesh of env 0 and where its loop ended
    quads, vertex_xy = env.get_elements(0)
    print(f"   env 0: {len(quads)} elements, {len(vertex_xy)} vertices, ended after {int(res.steps[0])} moves with code {int(res.code[0])}")
    env.close()


if __name__ == "__main__":
    main()
