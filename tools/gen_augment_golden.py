"""TEST INFRASTRUCTURE (needs the reference checkout, like oracle/gen_*.py): records MeshAugmentation of the reference's
general/data_augmentation.py for tests/test_augment_cpu.py and tests/test_gpu_augment.py.

    tests/golden/quality_augment_proposals.npz   random / sample_state / sample_action / check_obs_quality on recorded uniforms
    tests/golden/quality_augment_scores.npz      compute_quality, estimate_max_quality(method=3), the accept decisions, the obs check
    tests/golden/augment_counts.json             row counts of the reference's own sampling(n, 0.7), and how long it took here

(The two .npz carry the `quality_` prefix because tests/conftest.py takes every other .npz of tests/golden/ for a recorded
step() trace, and tests/policy_ref.py every other `obs [., 18]` for network input rows.)

usage: python tools/gen_augment_golden.py [--no-counts]     (the counts take the reference about half a minute)
"""
from __future__ import annotations

import contextlib
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_harness as H  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
TYPES = (0.5, 0, 1)                  # type index 0, 1, 2: the order sampling() concatenates
N_UNIFORMS = (57, 17, 17)
PROPOSAL_SEED, PER_CELL = 20240, 8   # proposals per (type, bin) of quality_augment_proposals.npz
SCORE_SEED, PER_TYPE, ACTIONS_05, ACCEPTED_PER_TYPE = 7, 600, 4, 30
THRESHOLDS = (0.6, 0.7, 0.8)
MARGIN = 1e-9
COUNT_SEED, COUNT_N = 3, (88, 440)


def load():
    H.load_post_processing()         # the stand-ins for the plotting libraries the module imports
    import importlib
    with contextlib.redirect_stdout(io.StringIO()):
        mod = importlib.import_module("general.data_augmentation")
    return mod


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def record_proposals(mod):
    mg = mod.MeshAugmentation([], [])
    keys = list(mg.get_angle_distribution(11).keys())
    assert [float(k) for k in keys] == [0.4, 0.6, 0.8, 1.0, 1.2, 1.4, 1.6, 1.8, 2.0, 2.2, 2.4]
    rng = np.random.default_rng(PROPOSAL_SEED)
    rows = [(t, b) for t in range(3) for b in range(11) for _ in range(PER_CELL)]
    B = len(rows)
    uniforms = np.zeros((B, 57))
    angle, obs, acts, rej = np.zeros(B), np.zeros((B, 18)), np.zeros((B, 20, 3)), np.zeros(B, bool)
    real = np.random.random
    try:
        for i, (t, b) in enumerate(rows):
            uniforms[i, :N_UNIFORMS[t]] = rng.random(N_UNIFORMS[t])
            it = iter(uniforms[i, :N_UNIFORMS[t]].tolist())
            np.random.random = lambda: next(it)   # noqa: B023
            k = keys[b]
            angle[i] = mg.random(float(k) - 0.2, float(k))
            o = mg.sample_state(angle[i], type=TYPES[t])
            a = mg.sample_action(o, angle[i], type=TYPES[t], m=20)
            assert next(it, None) is None, "the draw count of a proposal changed"
            obs[i], acts[i, :len(a)], rej[i] = o, a, mg.check_obs_quality(o)
    finally:
        np.random.random = real
    assert 0 < rej.sum() < B
    np.savez_compressed(os.path.join(OUT, "quality_augment_proposals.npz"), uniforms=uniforms, t_index=np.array([r[0] for r in rows], np.int32),
                        b_index=np.array([r[1] for r in rows], np.int32), angle=angle, proposal_obs=obs, actions=acts, rejected=rej)
    # (the key is not `obs`: tests/policy_ref.input_rows gathers every golden `obs [., 18]` as network input rows)
    print(f"quality_augment_proposals.npz: {B} proposals, {int(rej.sum())} rejected by check_obs_quality")


def record_scores(mod):
    mg = mod.MeshAugmentation([], [])
    keys = list(mg.get_angle_distribution(11).keys())
    np.random.seed(SCORE_SEED)
    called = []
    inner = mg.compute_boundary_quality
    mg.compute_boundary_quality = lambda *a, **k: (called.append(1), inner(*a, **k))[1]   # reached for a valid element only
    lam = 0.618
    prop_obs, prop_rej, prop_t, prop_b = [], [], [], []
    prop, act, valid, q, raises = [], [], [], [], []
    for t in range(3):
        for i in range(PER_TYPE):
            b = i % 11
            angle = mg.random(float(keys[b]) - 0.2, float(keys[b]))
            o = mg.sample_state(angle, type=TYPES[t])
            prop_obs.append(o)
            prop_rej.append(bool(mg.check_obs_quality(o)))
            prop_t.append(t)
            prop_b.append(b)
            for a in mg.sample_action(o, angle, type=TYPES[t], m=ACTIONS_05):
                prop.append(len(prop_obs) - 1)
                act.append(a)
                del called[:]
                try:
                    ele, bnd = mg.compute_quality([o, a])
                    mx_ele, mx_bnd = mg.estimate_max_quality([o, a], method=3)
                    raises.append(False)
                except Exception:
                    ele = bnd = mx_ele = mx_bnd = float("nan")
                    raises.append(True)
                valid.append(bool(called))
                q.append((ele, bnd, mx_ele, mx_bnd))
    q = np.array(q, np.float64)
    valid, raises = np.array(valid), np.array(raises)
    assert not raises.any(), "the reference raised: choose another SCORE_SEED"

    def ratios(q):
        return np.stack([((1 - lam) * q[:, 0] + lam * q[:, 1]) / ((1 - lam) * q[:, 2] + lam * q[:, 3]), q[:, 0] / q[:, 2]], 1)

    def decide(q):
        ratio = ratios(q)
        margin = min(float(np.abs(ratio - thr).min()) for thr in THRESHOLDS)
        assert margin > MARGIN, f"a ratio within {MARGIN} of a threshold ({margin}): choose another SCORE_SEED"
        return np.stack([(ratio >= thr).all(1) for thr in THRESHOLDS], 1), margin

    accept, margin = decide(q)
    prop_t = np.array(prop_t, np.int32)
    row_t = prop_t[np.array(prop)]
    assert (q[~valid, :2] == 0).all() and (q[valid, 0] > 0).all()
    assert valid.mean() >= 0.10, valid.mean()
    per_type = [int(accept[row_t == t, 1].sum()) for t in range(3)]
    # 600 unfiltered proposals of a type hold 17 / 9 / 15 rows accepted at 0.7 on average (36 seeds: at most 25 / 16 / 23), never
    # the 30 a type should have.  The 3600 rows stay as they are; the stream goes on, and the next accepted rows of each type are
    # kept as `extra_*` until the type has its 30.
    extra = dict(obs=[], rejected=[], act=[], q=[], t=[])
    for t in range(3):
        have, i = per_type[t], PER_TYPE
        while have < ACCEPTED_PER_TYPE:
            b, i = i % 11, i + 1
            angle = mg.random(float(keys[b]) - 0.2, float(keys[b]))
            o = mg.sample_state(angle, type=TYPES[t])
            for a in mg.sample_action(o, angle, type=TYPES[t], m=ACTIONS_05):
                row = (*mg.compute_quality([o, a]), *mg.estimate_max_quality([o, a], method=3))
                r = ratios(np.array([row], np.float64))[0]
                if (r >= 0.7).all() and have < ACCEPTED_PER_TYPE:
                    have += 1
                    for k, v in zip(("obs", "rejected", "act", "q", "t"), (o, bool(mg.check_obs_quality(o)), a, row, t)):
                        extra[k].append(v)
    extra_q = np.array(extra["q"], np.float64)
    extra_accept, extra_margin = decide(extra_q)
    assert extra_accept[:, 1].all()
    extra_t = np.array(extra["t"], np.int32)
    total = [per_type[t] + int((extra_t == t).sum()) for t in range(3)]
    assert min(total) >= ACCEPTED_PER_TYPE, total
    prop_rej = np.array(prop_rej)
    np.savez_compressed(os.path.join(OUT, "quality_augment_scores.npz"), prop_obs=np.array(prop_obs, np.float64), prop_rejected=prop_rej,
                        prop_t=prop_t, prop_b=np.array(prop_b, np.int32), prop=np.array(prop, np.int32),
                        act=np.array(act, np.float64), valid=valid, q=q, thresholds=np.array(THRESHOLDS), accept=accept,
                        raises=raises, reject_rate=np.array([prop_rej[prop_t == t].mean() for t in range(3)]),
                        reject_n=np.array([PER_TYPE] * 3, np.int64), extra_obs=np.array(extra["obs"], np.float64),
                        extra_rejected=np.array(extra["rejected"]), extra_act=np.array(extra["act"], np.float64), extra_q=extra_q,
                        extra_accept=extra_accept, extra_t=extra_t)
    print(f"quality_augment_scores.npz: {len(q)} rows, {valid.mean():.1%} valid, accepted at 0.7 per type {per_type} + {len(extra_q)} extra rows = "
          f"{total}, smallest margin {min(margin, extra_margin):.2g}, "
          f"obs rejection {[round(float(prop_rej[prop_t == t].mean()), 3) for t in range(3)]}")


def record_counts(mod):
    out = {"threshold": 0.7, "seed": COUNT_SEED, "types": list(TYPES), "n": {}}
    for n in COUNT_N:
        np.random.seed(COUNT_SEED)
        mg = mod.MeshAugmentation([], [])
        t0 = time.time()
        data = quiet(mg.sampling, n, 0.7)
        dt = time.time() - t0
        types = np.array(data["output_types"]).reshape(-1)
        out["n"][str(n)] = {"rows": int(len(types)), "per_type": [int((types == t).sum()) for t in TYPES],
                            "reference_seconds_one_core": round(dt, 1)}
        print(f"sampling({n}, 0.7): {len(types)} rows {out['n'][str(n)]['per_type']} in {dt:.1f} s")
    with open(os.path.join(OUT, "augment_counts.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def main():
    mod = load()
    record_proposals(mod)
    record_scores(mod)
    if "--no-counts" not in sys.argv:
        record_counts(mod)


if __name__ == "__main__":
    main()
