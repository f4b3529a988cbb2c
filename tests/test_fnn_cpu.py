"""CPU: the host half of the FNN mesher (reinforcementlearning4meshgeneration_amd/fnn.py, include/meshenv_fnn.h): the weight
packing, the refusals, the packaging of the C-ABI, and the seed hunt -- the closed loop of general/EBRD.py:525-548 run with
eager torch and the oracle's move(), which finds and pins the conditions tests/test_gpu_fnn.py needs of its seeded nets.
Nothing here needs a GPU."""
import os
import re
import types

import numpy as np
import pytest

import fnn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_packing_round_trip_is_bit_exact():
    from reinforcementlearning4meshgeneration_amd.fnn import PACKED_FLOATS, FNNSpec
    policy = R.make_policy(5, R.ACTION_BIAS)
    sd = policy.state_dict()
    assert list(sd) == [f"{name}.{part}" for name, _, _ in R.LAYERS for part in ("weight", "bias")]
    for spec in (FNNSpec.from_state_dict(sd), FNNSpec.from_module(policy), FNNSpec.from_state_dict({k: v.numpy() for k, v in sd.items()})):
        packed = spec.packed()
        assert packed.dtype == np.float32 and packed.shape == (PACKED_FLOATS,) == (R.PACKED_FLOATS,)
        back, padding = R.unpack(packed)
        assert sorted(back) == sorted(sd)
        for key, want in sd.items():
            got = back[key]
            assert got.shape == tuple(want.shape), key
            assert np.array_equal(got.view(np.uint32), want.numpy().view(np.uint32)), key     # bit for bit
        assert padding.size == R.PACKED_FLOATS - sum(v.numel() for v in sd.values()) and not padding.any()
    # the shared head tile: columns 0-1 the action_head, 2-4 the type_head, in that order, biases alike
    head_bias = packed[-16:]
    assert np.array_equal(head_bias[:2], np.float32(R.ACTION_BIAS)) and np.array_equal(head_bias[2:5], sd["type_head.bias"].numpy())
    assert not head_bias[5:].any()
    # a distinct value per element lands where the layout says (an order mix-up inside a layer cannot cancel)
    ramp, at = {}, 1.0
    for name, rows, cols in R.LAYERS:
        ramp[f"{name}.weight"] = (at + np.arange(rows * cols, dtype=np.float32)).reshape(rows, cols)
        ramp[f"{name}.bias"] = -(at + np.arange(rows, dtype=np.float32))
        at += rows * cols
    back, padding = R.unpack(FNNSpec.from_state_dict(ramp).packed())
    assert all(np.array_equal(back[k], v) for k, v in ramp.items()) and not padding.any()


def test_other_architectures_are_refused_with_the_expected_shapes():
    from reinforcementlearning4meshgeneration_amd.fnn import FNNSpec
    sd = dict(R.make_policy(0).state_dict())
    wide = dict(sd)
    wide["fc1.weight"], wide["fc1.bias"] = np.zeros((500, 6), np.float32), np.zeros(500, np.float32)    # original_ann.py
    with pytest.raises(ValueError, match=r"fc1 \[64, 18\]"):
        FNNSpec.from_state_dict(wide)
    headless = {k: v for k, v in sd.items() if not k.startswith("type_head")}
    with pytest.raises(ValueError, match="type_head"):
        FNNSpec.from_state_dict(headless)
    scalar_type = dict(sd)
    scalar_type["type_head.weight"], scalar_type["type_head.bias"] = np.zeros((1, 16), np.float32), np.zeros(1, np.float32)
    with pytest.raises(ValueError, match=r"type_head \[3, 16\]"):
        FNNSpec.from_state_dict(scalar_type)
    with pytest.raises(ValueError, match="type_head"):
        FNNSpec.from_module(types.SimpleNamespace(**{n: getattr(R.make_policy(0), n) for n, _, _ in R.LAYERS[:-1]}))
    # the C entry refuses the same shapes itself, naming what it expects
    from reinforcementlearning4meshgeneration_amd import _capi
    L = _capi.load()
    spec = FNNSpec.from_state_dict(sd)
    ptrs, shapes = spec.load_args()
    shapes = shapes.copy()
    shapes[0] = 500
    out = np.zeros(R.PACKED_FLOATS, np.float32)
    assert L.meshenv_fnn_pack(ptrs, shapes.ctypes.data, out.ctypes.data) == _capi.E_ARG
    assert b"fc1 [64][18]" in L.meshenv_fnn_last_error(None)


def test_mesh_with_refuses_auto_reset_and_a_missing_element_log():
    from reinforcementlearning4meshgeneration_amd.vec_env import MeshVecEnv
    with pytest.raises(ValueError, match="auto_reset=False"):
        MeshVecEnv.mesh_with(types.SimpleNamespace(auto_reset=True, log_capacity=512), None)
    with pytest.raises(ValueError, match="log_capacity"):
        MeshVecEnv.mesh_with(types.SimpleNamespace(auto_reset=False, log_capacity=0), None)
    with pytest.raises(ValueError, match="check_every"):
        MeshVecEnv.mesh_with(types.SimpleNamespace(auto_reset=False, log_capacity=512), None, check_every=0)


def test_exports_and_header():
    from reinforcementlearning4meshgeneration_amd import _capi, fnn
    header = open(os.path.join(ROOT, "include", "meshenv_fnn.h")).read()
    defines = dict(re.findall(r"#define\s+(MESHENV_[A-Z_]+)\s+(\d+)", header))
    assert int(defines["MESHENV_FNN_PACKED_FLOATS"]) == _capi.FNN_PACKED_FLOATS == fnn.PACKED_FLOATS == R.PACKED_FLOATS
    assert int(defines["MESHENV_FNN_TENSORS"]) == _capi.FNN_TENSORS == 2 * len(fnn.LAYERS) == 14
    assert int(defines["MESHENV_MOVE_SKIPPED"]) == _capi.MOVE_SKIPPED == 255
    assert tuple(fnn.LAYERS) == tuple(R.LAYERS)
    kernels = open(os.path.join(ROOT, "reinforcementlearning4meshgeneration_amd", "csrc", "meshenv_fnn.h")).read()
    assert "k_fnn_forward" in kernels and "k_fnn_advance" in kernels and "__builtin_amdgcn_mfma_f32_16x16x4f32" in kernels
    assert _capi.load().meshenv_abi_version() == 1      # a header of its own: meshenv.h is unchanged


def test_seed_hunt_closed_loop_net_meets_the_conditions_of_the_gpu_test():
    """The closed-loop reference (eager torch float32 Policy + oracle move()) on the 48 envs of the GPU test.  The net of
    CLOSED_LOOP_SEED must extract an element in at least a quarter of the envs, send at least one env through smooth_pave,
    and leave at least one env finished before MAX_STEPS and at least one not; the counts are pinned as observed here."""
    loop, seen = R.closed_loop_cpu(R.CLOSED_LOOP_SEED)
    counts = R.closed_loop_counts(loop)
    print("closed loop, seed", R.CLOSED_LOOP_SEED, counts, "accepted moves", int(loop.accepted.sum()), "smooth_pave passes",
          int(loop.smoothed.sum()), "steps", np.sort(loop.steps).tolist())
    assert counts["envs_with_accepted_move"] >= 0.25 * R.N_ENVS
    assert counts["envs_through_smooth_pave"] >= 1 and counts["finished_early"] >= 1 and counts["unfinished"] >= 1
    assert counts == R.CLOSED_LOOP_COUNTS and int(loop.accepted.sum()) == R.CLOSED_LOOP_ACCEPTED_MOVES
    assert seen.shape == (R.MAX_STEPS, R.N_ENVS, 18)
    # a finished env is never moved again: its step count is where it finished
    assert (loop.steps[~loop.finished] == R.MAX_STEPS).all() and (loop.steps[loop.finished] < R.MAX_STEPS).all()


def test_early_stop_net_finishes_every_env_where_the_oracle_says():
    """The crafted net of the GPU early-stop tests returns type 0 and EARLY_STOP_POINT whatever it reads; the oracle alone then
    gives the step count of each of the 21 envs (16 domains, the first five twice).  Pinned as observed here."""
    import torch
    sd = R.early_stop_state_dict()
    net = R.make_policy(0)
    net.load_state_dict(sd)
    pts, typ = R.get_action(net, R.forward_observations(33))
    assert np.array_equal(pts, np.tile(np.float64(np.float32(R.EARLY_STOP_POINT)), (33, 1))) and not typ.any()
    assert int(torch.argmax(torch.tensor(R.EARLY_STOP_TYPE_BIAS))) == 0
    loop, total = R.early_stop_cpu()
    print("early-stop net: vector steps", total, "steps", loop.steps.tolist(), "smooth_pave passes", loop.smoothed.tolist(),
          "accepted moves", loop.accepted.tolist())
    assert R.EARLY_STOP_ENVS == 21 > 16 and R.EARLY_STOP_ENVS % 16 != 0
    assert total == max(R.EARLY_STOP_STEPS) == 192 and loop.finished.all()
    assert loop.steps.tolist() == list(R.EARLY_STOP_STEPS)
    assert (loop.done == 1).all() and (loop.complete == 0).all() and (loop.code == 0).all()
    assert (loop.smoothed >= 1).all()
    # what the GPU tests cut out of these counts: chunks of 50 stop at 200; 195 = 50 + 50 + 50 + 45 covers the longest env; a
    # budget of 9 = 4 + 4 + 1 finishes exactly the envs that need 8
    assert -(-192 // 50) * 50 == 200 and 192 <= 195 and sorted(set(R.EARLY_STOP_STEPS))[:2] == [8, 10]
    assert R.EARLY_STOP_STEPS.count(8) == 2
    # the domains repeat with period 16
    assert R.EARLY_STOP_STEPS[16:] == R.EARLY_STOP_STEPS[:5]


@pytest.mark.parametrize("seed,type_scale", R.FORWARD_NETS)
def test_seed_hunt_forward_nets_keep_the_margin_cap(seed, type_scale):
    """Eager torch float32 against float64 alone, on the observations the GPU forward test uses: at most 1 % of the rows may
    have a top-two logit margin within 8 err_torch, and on the others float32 must already pick the float64 rule type."""
    obs = R.forward_observations(4096)
    assert obs.shape == (4096, 18) and (np.abs(obs).sum(axis=1) == 0).sum() == 240 and len(np.unique(obs, axis=0)) > 500
    st = R.forward_stats(R.forward_policy(seed, type_scale), obs)
    excluded = 1.0 - st["decided"].mean()
    hist = np.bincount(st["l64"].argmax(axis=1), minlength=3)
    print(f"forward net seed {seed} x{type_scale}: err_torch {st['err_torch']:.3g}, excluded {excluded:.4f}, fp64 argmax counts {hist.tolist()}")
    assert 0 < st["err_torch"] < 2e-6 and excluded <= 0.01
    assert (st["l32"].argmax(axis=1) == st["l64"].argmax(axis=1))[st["decided"]].all()
    if type_scale != 1.0:
        assert (hist > 1000).sum() >= 2      # the rule type really varies over the batch
