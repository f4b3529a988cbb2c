"""The sample generator without a GPU: the float64 restatement (tests/augment_ref.py) against the reference's recordings
(tools/gen_augment_golden.py), the row-count formula, the C header against the binding, every Python refusal, the Philox tag,
the JSON round trip."""
from __future__ import annotations

import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_ref as A  # noqa: E402
import policy_ref  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def proposals():
    return dict(np.load(os.path.join(GOLDEN, "quality_augment_proposals.npz")))


@pytest.fixture(scope="module")
def scores():
    return dict(np.load(os.path.join(GOLDEN, "quality_augment_scores.npz")))


# ------------------------------------------------------------------------------------------------------------ restatement
def test_proposals_bit_for_bit(proposals):
    z = proposals
    angle, obs, acts, rej = A.propose(z["uniforms"], z["t_index"], z["b_index"])
    assert np.array_equal(angle, z["angle"]) and np.array_equal(obs, z["proposal_obs"]) and np.array_equal(acts, z["actions"])
    assert np.array_equal(rej, z["rejected"])
    # the fixture covers every (type, bin) cell and both outcomes of the check
    assert len(set(zip(z["t_index"].tolist(), z["b_index"].tolist()))) == 33 and 0 < rej.sum() < len(rej)
    assert (obs[:, 1] == 0).all() and np.array_equal(obs[:, 17], angle)
    t = z["t_index"]
    assert np.array_equal(acts[t == 1, 0, 1:], obs[t == 1, 14:16]) and np.array_equal(acts[t == 2, 0, 1:], obs[t == 2, 2:4])
    assert (acts[t == 0, :, 0] == 0.5).all() and (acts[t != 0, 1:] == 0).all()


def test_scores_bit_for_bit(scores):
    z = scores
    assert len(z["q"]) == 3600 and not z["raises"].any()
    obs = z["prop_obs"][z["prop"]]
    rej, valid, q = A.score(obs, z["act"])
    assert np.array_equal(rej, z["prop_rejected"][z["prop"]])
    assert np.array_equal(valid, z["valid"])
    assert np.array_equal(q, z["q"])          # both sides are CPython's libm
    assert valid.mean() >= 0.10
    for k, thr in enumerate(z["thresholds"]):
        acc = np.array([A.accepted(*row, thr) for row in q])
        assert np.array_equal(acc, z["accept"][:, k])
        margin = min(abs(r - thr) for row in q for r in A.ratios(*row))
        assert margin > 1e-9
    # 600 unfiltered proposals of a type hold fewer than 30 rows accepted at 0.7 (tools/gen_augment_golden.py); the recording's
    # `extra_*` rows, the next accepted ones of the same reference stream, bring every type to 30
    row_t = z["prop_t"][z["prop"]]
    assert min(int(z["accept"][row_t == t, 1].sum()) + int((z["extra_t"] == t).sum()) for t in range(3)) >= 30
    rej, valid, q = A.score(z["extra_obs"], z["extra_act"])
    assert np.array_equal(rej, z["extra_rejected"]) and valid.all() and np.array_equal(q, z["extra_q"])
    for k, thr in enumerate(z["thresholds"]):
        assert np.array_equal(np.array([A.accepted(*row, thr) for row in q]), z["extra_accept"][:, k])
        assert min(abs(r - thr) for row in q for r in A.ratios(*row)) > 1e-9
    assert z["extra_accept"][:, 1].all()


def test_row_counts():
    counts = json.load(open(os.path.join(GOLDEN, "augment_counts.json")))
    from reinforcementlearning4meshgeneration_amd import augmentation as M
    for n, rec in counts["n"].items():
        n = int(n)
        per_type = [11 * A.rows_per_bin(n, 1, t) for t in range(3)]
        assert per_type == rec["per_type"] and A.row_count(n) == rec["rows"] == M.row_count(n)
        assert tuple(A.rows_per_bin(n, 1, t) for t in range(3)) == M.rows_per_bin(n)
    assert counts["n"]["440"]["per_type"] == [209, 99, 99] and counts["n"]["88"]["rows"] == 55
    assert A.row_count(40000, 10) == M.row_count(40000, 10) == 10 * 11 * ((182 - 1) + 2 * (91 - 1)) == 39710
    assert A.row_count(0) == M.row_count(0) == 0 and M.row_count(11) == 0      # quotas 1, 1, 1: counted, never appended
    assert [A.quota(440, 1, t) for t in range(3)] == [20, 10, 10]


# ---------------------------------------------------------------------------------------------------------------- binding
def test_exports_and_header():
    import reinforcementlearning4meshgeneration_amd as pkg
    from reinforcementlearning4meshgeneration_amd import _capi, augmentation
    assert len(_capi.EXPORTS_AUGMENT) == 7
    header = open(os.path.join(ROOT, "include", "meshenv_augment.h")).read()
    defines = dict(re.findall(r"#define\s+(MESHENV_[A-Z_]+)\s+(\d+)", header))
    assert int(defines["MESHENV_AUGMENT_PHILOX_TAG"]) == _capi.AUGMENT_PHILOX_TAG == A.PHILOX_TAG
    assert int(defines["MESHENV_AUGMENT_BINS"]) == _capi.AUGMENT_BINS == len(A.BINS) == len(augmentation.BIN_KEYS)
    assert int(defines["MESHENV_AUGMENT_TYPES"]) == _capi.AUGMENT_TYPES == 3
    assert int(defines["MESHENV_AUGMENT_MAX_ACTIONS"]) == _capi.AUGMENT_MAX_ACTIONS == max(A.N_ACTIONS)
    assert int(defines["MESHENV_AUGMENT_UNIFORMS"]) == _capi.AUGMENT_UNIFORMS == max(A.N_UNIFORMS)
    assert int(defines["MESHENV_AUGMENT_MAX_POOL"]) == _capi.AUGMENT_MAX_POOL
    assert int(defines["MESHENV_AUGMENT_MAX_ROUND"]) == _capi.AUGMENT_MAX_ROUND
    assert int(defines["MESHENV_AUGMENT_MAX_ROUNDS"]) == _capi.AUGMENT_MAX_ROUNDS and _capi.AUGMENT_MAX_ROUNDS * _capi.AUGMENT_MAX_ROUND < 2 ** 32
    assert int(defines["MESHENV_AUGMENT_STATS"]) == _capi.AUGMENT_STATS == len(augmentation.STATS)
    assert augmentation.TYPES == A.TYPES and augmentation.FRACTIONS == A.FRACS and augmentation.BIN_KEYS == A.BINS
    for k in ("DeviceMeshAugmentation", "AugmentScore"):
        assert k in pkg.__all__ and getattr(pkg, k) is getattr(augmentation, k)
    assert augmentation.AugmentScore._fields == ("obs_rejected", "valid", "ele", "boundary", "max_ele", "max_boundary", "accept")
    # the device header states the tag and the counter layout the restatement uses
    dev = open(os.path.join(ROOT, "reinforcementlearning4meshgeneration_amd", "csrc", "meshenv_augment.h")).read()
    assert re.search(r"kAugPhiloxTag\s*=\s*5u", dev)


def test_refusals():
    import torch
    from reinforcementlearning4meshgeneration_amd import augmentation as M
    ok = dict(n=88, threshold=0.7, pool=1, round_size=256, max_rounds=4, dtype=torch.float32)
    M.check_sampling_args(**ok)
    for bad in (dict(n=-1), dict(pool=0), dict(pool=-3), dict(pool=1025), dict(threshold=0.0), dict(threshold=-0.1), dict(threshold=1.5),
                dict(threshold=float("nan")), dict(round_size=63), dict(round_size=2 ** 20 + 64), dict(round_size=100),
                dict(max_rounds=0), dict(max_rounds=4096)):
        with pytest.raises(ValueError):
            M.check_sampling_args(**{**ok, **bad})
    for bad in (dict(n=88.0), dict(pool=1.5), dict(threshold="0.7"), dict(threshold=None), dict(dtype=torch.float16), dict(n=True)):
        with pytest.raises(TypeError):
            M.check_sampling_args(**{**ok, **bad})
    M.check_sampling_args(**{**ok, "threshold": 1.0})
    obs, act = torch.zeros(5, 18, dtype=torch.float64), torch.zeros(5, 3, dtype=torch.float64)
    M.check_score_args(obs, act)
    M.check_score_args(obs, act, 0.7)
    M.check_score_args(obs[:0], act[:0])
    for o, a in ((obs[:, :17], act), (obs, act[:, :2]), (obs[0], act[0]), (obs, act[:4]), (obs.reshape(5, 2, 9), act)):
        with pytest.raises(ValueError):
            M.check_score_args(o, a)
    for o, a in ((obs.float(), act), (obs, act.float()), (obs.numpy(), act), (obs, act.long())):
        with pytest.raises(TypeError):
            M.check_score_args(o, a)
    for thr in (0.0, 1.01, -1):
        with pytest.raises(ValueError):
            M.check_score_args(obs, act, thr)
    u = torch.zeros(4, 57, dtype=torch.float64)
    t, b = M.check_propose_args(u, [0, 1, 2, 0], [0, 10, 5, 3])
    assert t.dtype == np.int32 and b.dtype == np.int32
    for args in ((u[:, :17], [0] * 4, [0] * 4), (u, [0] * 3, [0] * 4), (u, [3, 0, 0, 0], [0] * 4), (u, [0] * 4, [11, 0, 0, 0]),
                 (u, [-1, 0, 0, 0], [0] * 4)):
        with pytest.raises(ValueError):
            M.check_propose_args(*args)
    for args in ((u.float(), [0] * 4, [0] * 4), (u, [0.0] * 4, [0] * 4)):
        with pytest.raises(TypeError):
            M.check_propose_args(*args)


# ----------------------------------------------------------------------------------------------------------------- Philox
def test_philox_tag_is_a_stream_of_its_own():
    seed, w, t, b, p = 0x1234_5678_9ABC_DEF0, 3, 2, 7, 41
    u = A.philox_uniforms(seed, w, t, b, p, 57)
    assert u.shape == (57,) and (u >= 0).all() and (u < 1).all() and len(set(u.tolist())) == 57
    # the block of uniforms 2 j, 2 j + 1 is one Philox call with the documented counter; the map is numpy's 53-bit one
    j = 5
    words = policy_ref.philox4x32(p, j | b << 8 | t << 16, w, A.PHILOX_TAG, seed & A.MASK, seed >> 32)
    a0, b0, a1, b1 = (int(v) for v in words)
    assert u[2 * j] == ((a0 >> 5) * 67108864 + (b0 >> 6)) / 9007199254740992
    assert u[2 * j + 1] == ((a1 >> 5) * 67108864 + (b1 >> 6)) / 9007199254740992
    # none of the tags in use elsewhere (0 rollout noise, 1 replay draw, 2 TD target, 3 SAC actor gradient, 4 warm-up actions)
    import offpolicy_learn_ref
    import replay_ref
    import td_target_ref
    import actor_grad_ref
    taken = {0, replay_ref.DRAW_TAG, td_target_ref.PHILOX_TAG, actor_grad_ref.PHILOX_TAG, offpolicy_learn_ref.UNIFORM_TAG}
    assert taken == {0, 1, 2, 3, 4} and A.PHILOX_TAG not in taken
    for tag in taken:
        other = policy_ref.philox4x32(p, j | b << 8 | t << 16, w, tag, seed & A.MASK, seed >> 32)
        assert all(int(x) != int(y) for x, y in zip(words, other))
    # every coordinate of (seed, w, t, b, p) moves the stream, and a prefix is a prefix
    for other in ((seed + 1, w, t, b, p), (seed, w + 1, t, b, p), (seed, w, t - 1, b, p), (seed, w, t, b + 1, p), (seed, w, t, b, p + 1),
                  (seed ^ (1 << 40), w, t, b, p)):
        assert not np.intersect1d(u, A.philox_uniforms(*other, 57)).size
    assert np.array_equal(A.philox_uniforms(seed, w, t, b, p, 17), u[:17])


def test_selection_stops_at_the_quota():
    # the ordered selection on a bin with a generous acceptance: rows are a prefix-stable function of the stream
    x3, y3 = A.select_bin(5, 0, 0, 6, 3, 0.6)
    x1, y1 = A.select_bin(5, 0, 0, 6, 1, 0.6)
    assert x3.shape == (3, 18) and y3.shape == (3, 3) and np.array_equal(x3[:1], x1) and np.array_equal(y3[:1], y1)
    assert (y3[:, 0] == 0.5).all() and ((x3[:, 17] >= 1.4) & (x3[:, 17] < 1.6)).all()
    rej, valid, q = A.score(x3, y3)
    assert not rej.any() and valid.all() and all(A.accepted(*row, 0.6) for row in q)
    x0, y0 = A.select_bin(5, 0, 0, 6, 0, 0.6)
    assert x0.shape == (0, 18) and y0.shape == (0, 3)
    with pytest.raises(RuntimeError):
        A.select_bin(5, 0, 1, 0, 1, 0.999, max_proposals=50)


# ------------------------------------------------------------------------------------------------------------------- JSON
def test_json_round_trip(tmp_path, scores):
    from reinforcementlearning4meshgeneration_amd import augmentation as M
    x = scores["prop_obs"][scores["prop"]][:40]
    y = scores["act"][:40]
    path = str(tmp_path / "samples.json")
    M.save_json(path, x, y)
    data = json.load(open(path))
    assert sorted(data) == ["output_types", "outputs", "samples"]
    assert np.asarray(data["samples"]).shape == (40, 18) and np.asarray(data["output_types"]).shape == (40, 1)
    assert np.asarray(data["outputs"]).shape == (40, 2)
    # what build_training_data makes of it
    y_ref = np.concatenate((np.asarray(data["output_types"]), np.asarray(data["outputs"])), axis=1)
    assert np.array_equal(np.asarray(data["samples"]), x) and np.array_equal(y_ref, y)
    x2, y2 = M.load_json(path)
    assert np.array_equal(x2, x) and np.array_equal(y2, y) and x2.dtype == np.float64
    import torch
    M.DeviceMeshAugmentation.save_json(path, torch.from_numpy(x).float(), torch.from_numpy(y).float())
    x3, y3 = M.DeviceMeshAugmentation.load_json(path)
    assert np.array_equal(x3, x.astype(np.float32)) and np.array_equal(y3, y.astype(np.float32))
    with pytest.raises(ValueError):
        M.save_json(path, x[:, :17], y)
