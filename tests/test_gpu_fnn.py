"""GPU: the FNN mesher (include/meshenv_fnn.h; csrc/meshenv_fnn.h: k_fnn_forward, k_fnn_advance; k_move_skip):
  (a) the forward against the same net in float64, with a tolerance measured from eager torch float32 against float64;
      points / types exactly what EBRD.get_action makes of the device's own float32 outputs; crafted heads for ties and NaN;
  (b) mesh_with in lockstep with the oracle's move() on 48 envs over 16 domains, the freeze of finished envs (the skip
      mask), record=False against record=True, and the log_capacity = 0 path;
  (c) the early stops of mesh_with on a crafted net and 21 envs: the finished.all() break, a last chunk shorter than
      check_every, a call on a batch that has finished, a budget shorter than most episodes.
tests/fnn_ref.py holds the nets, the observations and the counts tests/test_fnn_cpu.py pinned for them on the CPU."""
import functools

import numpy as np
import pytest

import fnn_ref as R

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _fused(seed, type_scale):
    from reinforcementlearning4meshgeneration_amd import FusedFNN
    return FusedFNN.from_module(R.forward_policy(seed, type_scale))


def _device_forward(fnn, obs, finished=None):
    import torch
    fin = None if finished is None else torch.from_numpy(finished)
    return [x.cpu().numpy() for x in fnn.forward(torch.from_numpy(obs).cuda(), finished=fin, raw=True)]


# ------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("seed,type_scale", R.FORWARD_NETS)
@pytest.mark.parametrize("n", [1, 15, 16, 17, 33, 4096])
def test_forward_matches_fp64_within_the_measured_tolerance(n, seed, type_scale):
    """n: one workgroup, both sides of the 16-env tile boundary, a ragged tail (row 16 is a None observation), one
    workgroup per CU.  The yardstick is eager torch float32 against float64 on the same rows (err_torch); the device may
    be 4 err_torch + 1e-6 off float64: a different summation order through seven layers.  Measured on the MI355X at
    n = 4096: DESIGN.md section 28."""
    import torch
    policy = R.forward_policy(seed, type_scale)
    obs = R.forward_observations(4096)[:n]
    st = R.forward_stats(policy, obs)
    points, types, actions, logits = _device_forward(_fused(seed, type_scale), obs)
    err_dev = max(float(np.abs(actions - st["a64"]).max()), float(np.abs(logits - st["l64"]).max()))
    print(f"n {n} seed {seed} x{type_scale}: err_torch {st['err_torch']:.3g}, device against fp64 {err_dev:.3g}, "
          f"rows within the margin {int((~st['decided']).sum())}")
    assert actions.dtype == np.float32 and logits.dtype == np.float32 and points.dtype == np.float64 and types.dtype == np.float64
    assert err_dev <= 4 * st["err_torch"] + 1e-6
    # what get_action hands to move(): the exact widening of the float32 action, torch's argmax of the float32 logits over 2
    assert np.array_equal(points, actions.astype(np.float64))
    assert np.array_equal(types, torch.argmax(torch.from_numpy(logits), dim=1).numpy() / 2.0)
    # and the float64 net's rule type wherever its top-two margin decides it
    assert (~st["decided"]).mean() <= 0.01
    assert np.array_equal(types[st["decided"]], st["l64"].argmax(axis=1)[st["decided"]] / 2.0)
    # get_action is the same call without the raw outputs
    p2, t2 = _fused(seed, type_scale).get_action(torch.from_numpy(obs).cuda())
    assert np.array_equal(p2.cpu().numpy(), points) and np.array_equal(t2.cpu().numpy(), types)


def test_forward_writes_zeros_for_finished_rows_and_leaves_the_others():
    seed, scale = R.FORWARD_NETS[1]
    obs = R.forward_observations(33)
    plain = _device_forward(_fused(seed, scale), obs)
    finished = (np.arange(33) % 3 == 1).astype(np.uint8)
    masked = _device_forward(_fused(seed, scale), obs, finished)
    for a, b in zip(plain, masked):
        assert np.array_equal(a[finished == 0], b[finished == 0]) and not b[finished != 0].any()


CRAFTED = [   # type_head bias (zero trunk, zero head weights: the logits ARE the bias) -> torch.argmax
    ((1.0, 1.0, 1.0), 0), ((0.0, 2.0, 2.0), 1), ((2.0, 1.0, 2.0), 0), ((-1.0, -3.0, -1.0), 0), ((0.0, 0.0, 1e-30), 2),
    ((float("nan"), 5.0, 1.0), 0), ((1.0, float("nan"), float("nan")), 1), ((3.0, 1.0, float("nan")), 2),
    ((float("inf"), float("nan"), 0.0), 1), ((float("-inf"), float("-inf"), float("-inf")), 0), ((-0.0, 0.0, 0.0), 0),
]


@pytest.mark.parametrize("bias,want", CRAFTED)
def test_argmax_ties_take_the_lowest_index_and_the_first_nan_wins(bias, want):
    import torch
    from reinforcementlearning4meshgeneration_amd import FusedFNN
    sd = {k: torch.zeros_like(v) for k, v in R.make_policy(0).state_dict().items()}
    sd["type_head.bias"] = torch.tensor(bias, dtype=torch.float32)
    sd["action_head.bias"] = torch.tensor([0.375, -1.25])
    fnn = FusedFNN.from_state_dict(sd)
    obs = R.forward_observations(17)
    points, types, actions, logits = _device_forward(fnn, obs)
    assert np.array_equal(logits, np.tile(np.float32(bias), (17, 1)), equal_nan=True)
    assert int(torch.argmax(torch.tensor(bias, dtype=torch.float32))) == want                       # the table is torch's
    assert np.array_equal(types, np.full(17, want / 2.0))
    assert np.array_equal(points, np.tile([0.375, -1.25], (17, 1)))
    fnn.close()


# --------------------------------------------------------------------------------------------------------- closed loop
def _make_env(log_capacity=512, n=R.N_ENVS):
    from reinforcementlearning4meshgeneration_amd import MeshVecEnv
    doms = R.closed_loop_domains()
    env_domain = (np.arange(n) % len(doms)).astype(np.int32)
    return MeshVecEnv(doms, env_domain=env_domain, auto_reset=False, log_capacity=log_capacity)


def _snapshot(env, k, elements=True):
    st = env.get_state(k)
    out = {key: np.asarray(v).copy() for key, v in st.items()}
    if elements:
        out["quads"], out["vertex_xy"] = env.get_elements(k)
    out["not_valid"] = env.get_not_valid(k)
    return out


def _same(a, b):
    return a.keys() == b.keys() and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


EXTRA_STEPS = 16


FINAL = ("steps", "done", "complete", "code", "finished", "n_elements")


def _leg(env, loop, res):
    """What a recorded mesh_with call left, with the oracle loop stepped through the same moves -- fed the device's own recorded
    points and types."""
    hist = {k: getattr(res, k).cpu().numpy() for k in ("points", "types", "obs", "step_code", "step_done", "step_complete")}
    final = {k: getattr(res, k).cpu().numpy() for k in FINAL}
    trace = []
    for t in range(res.total_steps):
        before = (loop.finished.copy(), loop.obs.copy())
        trace.append(before + loop.step(hist["points"][t], hist["types"][t]))
    return dict(total_steps=res.total_steps, hist=hist, final=final, trace=trace, oracle=loop.summary(),
                snaps=[_snapshot(env, k) for k in range(env.num_envs)], obs_end=env.obs.cpu().numpy().copy())


@pytest.fixture(scope="module")
def run():
    """Once for the tests below: mesh_with(record=True) of the seeded closed-loop net, then EXTRA_STEPS more moves through
    mesh_with(reset=False), each with the oracle in lockstep -- fed the device's own recorded points and types."""
    from reinforcementlearning4meshgeneration_amd import FusedFNN
    policy = R.make_policy(R.CLOSED_LOOP_SEED, R.ACTION_BIAS)
    fnn = FusedFNN.from_module(policy)
    env = _make_env()
    loop = R.OracleLoop(R.make_refs(R.closed_loop_domains(), R.N_ENVS))

    first = _leg(env, loop, env.mesh_with(fnn, max_steps=R.MAX_STEPS, check_every=8, record=True))
    more = _leg(env, loop, env.mesh_with(fnn, max_steps=EXTRA_STEPS, check_every=8, record=True, reset=False))
    return dict(policy=policy, fnn=fnn, env=env, first=first, more=more)


def _check_leg(leg):
    """Every step of a leg against the oracle: the observation each forward read, the codes, the flags, the zero rows of the
    finished envs; at the end the bookkeeping and every env's mesh."""
    hist, final, oracle = leg["hist"], leg["final"], leg["oracle"]
    worst = 0.0
    for t, (fin0, obs0, ran, o, d, c, code) in enumerate(leg["trace"]):
        live = ~fin0
        assert np.array_equal(ran, live)
        # the observation the forward read: the oracle's current one (1e-5, the bound of test_gpu_move.py); zeros once finished
        diff = np.abs(hist["obs"][t][live].astype(np.float64) - obs0[live])
        worst = max(worst, float(diff.max()) if diff.size else 0.0)
        assert diff.size == 0 or diff.max() <= 1e-5, t
        assert not hist["obs"][t][fin0].any() and not hist["points"][t][fin0].any() and not hist["types"][t][fin0].any()
        assert np.array_equal(hist["step_code"][t], code), (t, hist["step_code"][t].tolist(), code.tolist())
        raised = code == 2           # the reference raises: no flags to compare
        assert np.array_equal(hist["step_done"][t][~raised], d[~raised]), t
        assert np.array_equal(hist["step_complete"][t][~raised], c[~raised]), t
    # the bookkeeping: steps to done or code >= 2, the last move's flags, the mesh
    assert np.array_equal(final["steps"], oracle["steps"]) and np.array_equal(final["finished"] != 0, oracle["finished"])
    assert np.array_equal(final["code"], oracle["code"])
    assert np.array_equal(final["done"], oracle["done"]) and np.array_equal(final["complete"], oracle["complete"])
    ok = oracle["code"] == 0
    assert np.abs(leg["obs_end"][ok].astype(np.float64) - oracle["obs"][ok]).max() <= 1e-5
    for k in range(len(leg["snaps"])):
        ids, xy = oracle["rings"][k]
        snap = leg["snaps"][k]
        assert np.array_equal(snap["ring_ids"], ids) and np.array_equal(snap["ring_xy"], xy), k
        assert snap["n_elem"] == oracle["n_elem"][k] == final["n_elements"][k] == len(snap["quads"]), k
        assert len(snap["not_valid"]) == oracle["n_not_valid"][k], k
    return worst


def test_mesh_with_runs_in_lockstep_with_the_oracle(run):
    leg = run["first"]
    assert leg["total_steps"] == R.MAX_STEPS and leg["hist"]["obs"].shape == (R.MAX_STEPS, R.N_ENVS, 18)
    worst = _check_leg(leg)
    counts = R.closed_loop_counts(leg["oracle"])
    print("closed loop on the device:", counts, "accepted moves", int(leg["oracle"]["accepted"].sum()), "smooth_pave passes",
          int(leg["oracle"]["smoothed"].sum()), "max obs err", worst)
    # the conditions the seed was chosen for (tests/test_fnn_cpu.py found them with the oracle alone)
    assert counts["envs_with_accepted_move"] >= 0.25 * R.N_ENVS and counts["envs_through_smooth_pave"] >= 1
    assert counts["finished_early"] >= 1 and counts["unfinished"] >= 1


def test_recorded_points_are_the_eager_net_on_the_recorded_observations(run):
    hist = run["first"]["hist"]
    live = hist["step_code"].reshape(-1) != 255
    obs = hist["obs"].reshape(-1, 18)[live]
    st = R.forward_stats(run["policy"], obs)
    pts = hist["points"].reshape(-1, 2)[live]
    err = float(np.abs(pts - st["a64"]).max())
    print(f"closed loop: {len(obs)} forwards, err_torch {st['err_torch']:.3g}, device points against fp64 {err:.3g}")
    assert err <= 4 * st["err_torch"] + 1e-6
    assert np.array_equal(pts.astype(np.float32).astype(np.float64), pts)          # widened float32 values
    typ = hist["types"].reshape(-1)[live]
    assert np.array_equal(typ[st["decided"]], st["l64"].argmax(axis=1)[st["decided"]] / 2.0) and (~st["decided"]).mean() <= 0.01


def test_finished_envs_stay_frozen_through_further_calls(run):
    """EXTRA_STEPS more moves through mesh_with(reset=False): every env that had finished is byte for byte as it was -- ring,
    record, element log, not_valid_points, observation (the skip mask of k_move and, through the codes, of the smoothing
    launches) -- while the others go on in lockstep with the oracle."""
    first, more = run["first"], run["more"]
    finished = first["final"]["finished"] != 0
    assert finished.any() and not finished.all() and more["total_steps"] == EXTRA_STEPS
    for k in np.flatnonzero(finished):
        assert _same(first["snaps"][k], more["snaps"][k]), k
    assert np.array_equal(more["obs_end"][finished], first["obs_end"][finished])
    for k in ("steps", "code", "done", "complete", "n_elements", "finished"):
        assert np.array_equal(more["final"][k][finished], first["final"][k][finished]), k
    h = more["hist"]
    assert (h["step_code"][:, finished] == 255).all() and not h["step_done"][:, finished].any() and not h["step_complete"][:, finished].any()
    assert not h["obs"][:, finished].any() and not h["points"][:, finished].any() and not h["types"][:, finished].any()
    _check_leg(more)
    assert (more["final"]["steps"][~finished] > first["final"]["steps"][~finished]).all()
    assert any(not _same(first["snaps"][k], more["snaps"][k]) for k in np.flatnonzero(~finished))


def test_record_false_gives_the_same_meshes_and_a_reset_env_starts_over(run):
    import torch
    fnn, first = run["fnn"], run["first"]
    env = _make_env()
    res = env.mesh_with(fnn, max_steps=R.MAX_STEPS, check_every=8, record=False)
    assert res.points is None and res.step_code is None and res.total_steps == R.MAX_STEPS
    for k in ("steps", "code", "done", "complete", "finished", "n_elements"):
        assert np.array_equal(getattr(res, k).cpu().numpy(), first["final"][k]), k
    assert all(_same(_snapshot(env, k), first["snaps"][k]) for k in range(R.N_ENVS))
    assert np.array_equal(env.obs.cpu().numpy(), first["obs_end"])
    # a reset env is no longer a finished one: mesh_with(reset=False) after a masked reset moves it again, from its first move
    finished = first["final"]["finished"] != 0
    env.reset(mask=torch.from_numpy(finished.astype(np.uint8)), static=True)
    res3 = env.mesh_with(fnn, max_steps=8, check_every=8, reset=False)
    assert np.array_equal(res3.steps.cpu().numpy()[finished], np.minimum(first["final"]["steps"][finished], 8))
    assert np.array_equal(res3.steps.cpu().numpy()[~finished], first["final"]["steps"][~finished] + 8)
    env.close()


def test_a_handle_without_element_log_finishes_at_needs_smoothing(run):
    """log_capacity = 0: the smooth_pave inside move() cannot run, the move returns MESHENV_MOVE_NEEDS_SMOOTHING with done = 1
    and the loop must finish the env there -- at the move where the oracle (and the logged handle) first went through
    smooth_pave.  mesh_with refuses such a handle; move_fnn is the call underneath it."""
    first = run["first"]
    first_smooth = first["oracle"]["first_smooth"]
    smoothed = first_smooth >= 0
    assert smoothed.sum() >= 1
    env = _make_env(log_capacity=0)
    with pytest.raises(ValueError, match="log_capacity"):
        env.mesh_with(run["fnn"], max_steps=8)
    env.reset(static=True)
    st = env._new_fnn_state()
    for _ in range(R.MAX_STEPS // 8):
        env.move_fnn(run["fnn"], 8, st)
    got = {k: v.cpu().numpy() for k, v in st.items()}
    print("log_capacity 0: envs finished at NEEDS_SMOOTHING", int(smoothed.sum()), "at moves", sorted(set(first_smooth[smoothed].tolist())))
    assert (got["code"][smoothed] == 3).all() and (got["done"][smoothed] == 1).all() and (got["complete"][smoothed] == 0).all()
    assert (got["finished"][smoothed] == 1).all() and np.array_equal(got["steps"][smoothed], first_smooth[smoothed])
    # the envs that never needed a smoothing end exactly as on the logged handle
    for k in ("steps", "code", "done", "complete", "finished", "n_elements"):
        assert np.array_equal(got[k][~smoothed], first["final"][k][~smoothed]), k
    for k in np.flatnonzero(~smoothed)[:8]:
        a, b = _snapshot(env, int(k), elements=False), first["snaps"][k]
        assert np.array_equal(a["ring_ids"], b["ring_ids"]) and np.array_equal(a["ring_xy"], b["ring_xy"])
    env.close()


def test_move_fnn_refuses_what_it_cannot_run(run):
    import torch
    from reinforcementlearning4meshgeneration_amd import MeshEnvError
    env, fnn = run["env"], run["fnn"]
    with pytest.raises(TypeError):
        env.move_fnn(object(), 1, env._new_fnn_state())
    with pytest.raises(ValueError):
        env.move_fnn(fnn, 0, env._new_fnn_state())
    with pytest.raises(ValueError):
        fnn.forward(torch.zeros((4, 17), device="cuda"))
    with pytest.raises(MeshEnvError, match="no output"):
        fnn._check(fnn._L.meshenv_fnn_forward(fnn._h, 4, torch.zeros((4, 18), device="cuda").data_ptr(), None, None, None, None, None),
                   "meshenv_fnn_forward")


# ---------------------------------------------------------------------------------------------------------- early stops
def _early_env():
    return _make_env(n=R.EARLY_STOP_ENVS)


@pytest.fixture(scope="module")
def early():
    """Once for the tests below: the early-stop net of tests/fnn_ref.py (type 0 and one point whatever it reads) on 21 envs,
    mesh_with(max_steps=500, check_every=50, record=True) with the oracle in lockstep, then eight more moves on the batch that
    has finished.  tests/test_fnn_cpu.py pins the step counts with the oracle alone."""
    from reinforcementlearning4meshgeneration_amd import FusedFNN
    fnn = FusedFNN.from_state_dict(R.early_stop_state_dict())
    env = _early_env()
    loop = R.OracleLoop(R.make_refs(R.closed_loop_domains(), R.EARLY_STOP_ENVS))
    first = _leg(env, loop, env.mesh_with(fnn, max_steps=500, check_every=50, record=True))
    state = {k: v.clone() for k, v in env._fnn_state.items()}
    again = env.mesh_with(fnn, max_steps=8, check_every=8, record=True, reset=False)
    after = dict(total_steps=again.total_steps, final={k: getattr(again, k).cpu().numpy() for k in FINAL},
                 hist={k: getattr(again, k).cpu().numpy() for k in ("points", "types", "obs", "step_code", "step_done", "step_complete")},
                 snaps=[_snapshot(env, k) for k in range(R.EARLY_STOP_ENVS)], obs_end=env.obs.cpu().numpy().copy(),
                 state_before=state, state_after={k: v.clone() for k, v in env._fnn_state.items()})
    yield dict(fnn=fnn, first=first, after=after)
    env.close()
    fnn.close()


def test_mesh_with_stops_at_the_chunk_in_which_the_last_env_finishes(early):
    leg = early["first"]
    hist, final = leg["hist"], leg["final"]
    steps = np.array(R.EARLY_STOP_STEPS)
    assert leg["total_steps"] == 200 and final["finished"].all() and hist["obs"].shape == (200, R.EARLY_STOP_ENVS, 18)
    worst = _check_leg(leg)
    print("early stop on the device: total_steps", leg["total_steps"], "steps", final["steps"].tolist(), "smooth_pave passes",
          leg["oracle"]["smoothed"].tolist(), "max obs err", worst)
    assert final["steps"].tolist() == list(R.EARLY_STOP_STEPS)
    assert (final["done"] == 1).all() and (final["complete"] == 0).all() and (final["code"] == 0).all()
    assert (leg["oracle"]["smoothed"] >= 1).all()
    # every forward returned the crafted action: type 0 and the point, on live rows; rows after an env's last move 255 / zeros
    live = np.arange(200)[:, None] < steps[None, :]
    assert np.array_equal(hist["step_code"] != 255, live)
    assert (hist["points"][live] == np.float64(np.float32(R.EARLY_STOP_POINT))).all() and not hist["types"][live].any()
    for k in ("points", "types", "obs", "step_done", "step_complete"):
        assert not hist[k][~live].any(), k
    # done is raised at each env's last move and at no other
    last = np.zeros_like(live)
    last[steps - 1, np.arange(R.EARLY_STOP_ENVS)] = True
    assert np.array_equal(hist["step_done"] != 0, last)


def test_a_last_chunk_shorter_than_check_every(early):
    fnn, first = early["fnn"], early["first"]
    env = _early_env()
    res = env.mesh_with(fnn, max_steps=195, check_every=50, record=True)
    assert res.total_steps == 195 and tuple(res.step_code.shape) == (195, R.EARLY_STOP_ENVS) and bool(res.finished.all())
    for k in FINAL:
        assert np.array_equal(getattr(res, k).cpu().numpy(), first["final"][k]), k
    assert all(_same(_snapshot(env, k), first["snaps"][k]) for k in range(R.EARLY_STOP_ENVS))
    assert np.array_equal(env.obs.cpu().numpy(), first["obs_end"])
    for k in ("points", "types", "obs", "step_code", "step_done", "step_complete"):
        assert np.array_equal(getattr(res, k).cpu().numpy(), first["hist"][k][:195]), k
    env.close()


def test_a_finished_batch_is_left_byte_for_byte(early):
    import torch
    first, after = early["first"], early["after"]
    assert after["total_steps"] == 8
    assert all(_same(a, b) for a, b in zip(first["snaps"], after["snaps"]))
    assert after["obs_end"].tobytes() == first["obs_end"].tobytes()
    for k, v in after["state_before"].items():
        assert torch.equal(v, after["state_after"][k]) and v.dtype == after["state_after"][k].dtype, k
    for k in FINAL:
        assert np.array_equal(after["final"][k], first["final"][k]), k
    h = after["hist"]
    assert h["step_code"].shape == (8, R.EARLY_STOP_ENVS) and (h["step_code"] == 255).all()
    for k in ("points", "types", "obs", "step_done", "step_complete"):
        assert not h[k].any(), k


def test_a_budget_shorter_than_most_episodes(early):
    fnn = early["fnn"]
    steps = np.array(R.EARLY_STOP_STEPS)
    env = _early_env()
    res = env.mesh_with(fnn, max_steps=9, check_every=4)
    assert res.total_steps == 9 and res.points is None
    finished = res.finished.cpu().numpy() != 0
    assert np.array_equal(finished, steps == 8) and finished.sum() == 2
    assert np.array_equal(res.steps.cpu().numpy(), np.minimum(steps, 9)) and (res.steps.cpu().numpy()[~finished] == 9).all()
    assert np.array_equal(res.done.cpu().numpy() != 0, finished)
    env.close()
