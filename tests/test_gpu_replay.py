"""GPU: DeviceReplayBuffer (k_replay_add / k_replay_sample, csrc/meshenv_replay.h) is SB3's ReplayBuffer as
tests/replay_ref.py restates it, bit for bit (int32 views compared; there is no tolerance anywhere): the six views, pos
and full after every add, the drawn indices, the five sampled fields, with synthetic histories, real TD3 / SAC rollouts, a
store beyond 4 GiB, SB3's numpy add, the refusals, and back-to-back calls without synchronisation."""
import ctypes as C

import numpy as np
import pytest

import replay_ref as R

pytestmark = pytest.mark.gpu

PATTERN = 0x7FC12345           # a NaN with a payload: rows that were never written must keep it
LOW_HIGH = (np.array([-1.0, -1.5, 0.0], np.float32), np.array([1.0, 1.5, 1.5], np.float32))


@pytest.fixture(scope="module")
def envs():
    from reinforcementlearning4meshgeneration_amd.domains import boundary
    from reinforcementlearning4meshgeneration_amd.vec_env import MeshVecEnv
    made = {}

    def get(n):
        if n not in made:
            made[n] = MeshVecEnv([boundary(0)], n_envs=n)
        return made[n]
    yield get
    for e in made.values():
        e.close()


def _buffer(env, rows, pattern=True, **kw):
    import torch
    from reinforcementlearning4meshgeneration_amd import DeviceReplayBuffer
    buf = DeviceReplayBuffer(env, buffer_size=rows * env.num_envs, **kw)
    ref = R.ReplayRef(rows * env.num_envs, env.num_envs, **kw)
    assert buf.rows == buf.buffer_size == ref.rows == rows and buf.n_envs == env.num_envs
    if pattern:
        buf.store.view(torch.int32).fill_(PATTERN)
        ref.fill(PATTERN)
    return buf, ref


def _assert_state(buf, ref, what):
    assert (buf.pos, buf.full, buf.size()) == (ref.pos, ref.full, ref.size()), what
    for k in R.ReplayRef.FIELDS:
        got, want = getattr(buf, k).cpu().numpy(), getattr(ref, k)
        assert got.dtype == np.float32 and got.shape == want.shape, (what, k)
        if not R.same_bits(got, want):
            bad = np.argwhere(np.ascontiguousarray(got).view(np.int32) != want.view(np.int32))
            raise AssertionError(f"{what} {k}: {len(bad)} elements differ, first at {bad[0].tolist()}: "
                                 f"{got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}")


def _actor_dict(torch, h):
    """The history in the shape step_actor_T returns it (obs[t] = the observation after step t, actions [T + 1])."""
    T, n = h["done"].shape
    acts = np.concatenate([h["actions"], np.zeros((1, n, 3), np.float32)])
    d = dict(actions=acts, obs=h["obs_after"], reward=h["reward"], done=h["done"], complete=h["complete"],
             terminal_obs=h["terminal_obs"])
    return {k: torch.from_numpy(v).cuda() for k, v in d.items()}, torch.from_numpy(h["obs0"]).cuda()


def _policy_dict(torch, h):
    """The history in the shape collect_rollout returns it (obs = the first T slices of a [T + 1] block)."""
    T, n = h["done"].shape
    block = torch.from_numpy(np.concatenate([h["obs0"][None], h["obs_after"]])).cuda()
    d = dict(actions=-h["actions"][::-1], buffer_actions=h["actions"], reward=h["reward"], done=h["done"],   # actions: not what is stored
             complete=h["complete"], terminal_obs=h["terminal_obs"])
    out = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}
    out["obs"] = block[:T]
    return out


# ------------------------------------------------------------------------------------------------ 1. synthetic histories
SHAPES = [(3, 1, 7), (1, 17, 4), (5, 17, 4), (6, 1000, 6), (9, 1000, 4), (7, 4096, 5), (32, 4096, 40), (3, 65536, 4)]


@pytest.mark.parametrize("T,n,rows", SHAPES, ids=[f"T{T}_n{n}_rows{r}" for T, n, r in SHAPES])
def test_add_rollout_equals_the_restatement(envs, T, n, rows):
    import torch
    env = envs(n)
    buf, ref = _buffer(env, rows)
    modes = set()
    for call in range(5 if T == 1 else 3):
        h = R.synthetic(T, n, seed=1000 * T + n + call)
        assert R.kinds_present(h["done"], h["complete"])
        if call % 3 == 0:          # step_actor_T's shape, actions scaled by the venv's Box (SAC)
            out, obs0 = _actor_dict(torch, h)
            assert buf.add_rollout(out, obs0=obs0) == T
            ref.add_rollout(**h, low_high=LOW_HIGH)
            modes.add("scaled")
        elif call % 3 == 1:        # collect_rollout's shape, buffer_actions as they are (TD3)
            h["actions"][0, n - 1, 2] = np.array([0x7FA00001], np.uint32).view(np.float32)[0]   # a NaN payload, copied untouched
            buf.add_rollout(_policy_dict(torch, h))
            ref.add_rollout(**h)
            modes.add("plain")
        else:                      # step_actor_T's shape with other bounds given (odd T) or the scaling switched off
            out, obs0 = _actor_dict(torch, h)
            lh = (np.array([-2.0, 0.0, -1.0], np.float32), np.array([3.0, 0.7, 1.1], np.float32)) if T % 2 else None
            buf.add_rollout(out, obs0=obs0, scale_actions=lh if lh is not None else False)
            ref.add_rollout(**h, low_high=lh)
        _assert_state(buf, ref, f"T={T} n={n} rows={rows} call {call}")
        if not ref.full:           # rows not yet written stay exactly as allocated, padding included
            tail = buf.store[ref.pos:].cpu().numpy().view(np.uint32)
            assert tail.size and (tail == PATTERN).all()
    assert modes == {"scaled", "plain"} and ref.full
    if n >= 4:                     # the special payloads went through
        o, r = buf.next_observations.cpu().numpy(), buf.rewards.cpu().numpy()
        assert np.isnan(o[:, 2]).any() and np.isinf(o[:, 3]).any()
        assert ((np.abs(r[:, 1]) > 0) & (np.abs(r[:, 1]) < np.finfo(np.float32).tiny)).any()


def test_every_kind_of_transition_is_in_the_histories():
    for T, n, _ in SHAPES:
        if T * n >= 3:
            h = R.synthetic(T, n, seed=1000 * T + n)
            assert R.kinds_present(h["done"], h["complete"]), (T, n)


# ------------------------------------------------------------------------------------------------ 2. real rollouts
def _td3(torch):
    from reinforcementlearning4meshgeneration_amd.policy import FusedPolicy
    torch.manual_seed(4321)
    pi, mu = [torch.nn.Linear(18, 256), torch.nn.Linear(256, 256)], torch.nn.Linear(256, 3)
    with torch.no_grad():
        mu.weight.mul_(6.0)
    return FusedPolicy.deterministic(pi, mu, activation="relu", sigma=torch.full((3,), 0.2))


def _sac(torch):
    from reinforcementlearning4meshgeneration_amd.actor import FusedActor
    torch.manual_seed(7)
    lin = [torch.nn.Linear(18, 128), torch.nn.Linear(128, 128), torch.nn.Linear(128, 128)]
    mu, ls = torch.nn.Linear(128, 3), torch.nn.Linear(128, 3)
    with torch.no_grad():
        mu.weight.mul_(6.0)
        ls.bias.fill_(-0.5)
    return FusedActor.from_torch(lin, mu, ls)


def _terminal_rows_check(buf, out, pos_before, T):
    """Stored next_observations of done envs are the terminal observations, not the reset observations."""
    done = out["done"].cpu().numpy() != 0
    term = out["terminal_obs"].cpu().numpy()
    nxt = buf.next_observations.cpu().numpy()
    checked = 0
    for t in range(max(T - buf.rows, 0), T):
        row = (pos_before + t) % buf.rows
        assert R.same_bits(nxt[row][done[t]], term[t][done[t]]), t
        checked += int(done[t].sum())
    assert checked > 0


def test_td3_collect_rollout_into_the_buffer():
    import torch
    from reinforcementlearning4meshgeneration_amd import MeshVecEnv, boundary
    n, T, rows = 4096, 260, 300            # two rollouts: the second write wraps, rows does not divide T
    env = MeshVecEnv([boundary(0)], n_envs=n)
    policy = _td3(torch)
    buf, ref = _buffer(env, rows)
    env.reset_tensor()
    for call in range(2):
        out = env.collect_rollout(policy, T, seed=11, counter=call * T)
        h = {k: out[k].cpu().numpy() for k in ("reward", "done", "complete", "terminal_obs")}
        obs = out["obs"].cpu().numpy()
        obs_after = np.concatenate([obs[1:], env.obs.cpu().numpy()[None]])     # env.obs: the observation after step T - 1
        assert h["done"].any() and (h["done"] & (1 - h["complete"])).any()
        before = buf.pos
        buf.add_rollout(out)
        ref.add_rollout(obs[0], obs_after, h["terminal_obs"], out["buffer_actions"].cpu().numpy(), h["reward"], h["done"],
                        h["complete"])
        _assert_state(buf, ref, f"td3 call {call}")
        _terminal_rows_check(buf, out, before, T)
    assert buf.full and buf.pos == (2 * T) % rows
    policy.close()
    env.close()


def test_sac_step_actor_T_into_the_buffer_with_scaled_actions():
    import torch
    from reinforcementlearning4meshgeneration_amd import MeshVecEnv, boundary
    n, T, rows = 4096, 260, 150            # T > rows: only the last 150 steps of each call stay
    env = MeshVecEnv([boundary(0)], n_envs=n)
    actor = _sac(torch)
    buf, ref = _buffer(env, rows)
    obs0 = env.reset_tensor().clone()
    acts = actor.sample(obs0, 5, 0)
    for call in range(2):
        out = env.step_actor_T(actor, acts, T, seed=5, counter=1 + call * T, want_terminal_obs=True)
        h = {k: out[k].cpu().numpy() for k in ("obs", "reward", "done", "complete", "terminal_obs")}
        assert h["done"].any()
        before = buf.pos
        buf.add_rollout(out, obs0=obs0)
        a = out["actions"][:T].cpu().numpy()
        ref.add_rollout(obs0.cpu().numpy(), h["obs"], h["terminal_obs"], a, h["reward"], h["done"], h["complete"],
                        low_high=LOW_HIGH)
        _assert_state(buf, ref, f"sac call {call}")
        _terminal_rows_check(buf, out, before, T)
        stored = buf.actions.cpu().numpy()
        assert stored.min() >= -1.0 and stored.max() <= 1.0 and np.abs(stored).max() > 0.5      # scaled to [-1, 1]
        obs0, acts = out["obs"][T - 1].clone(), out["actions"][T]
    actor.close()
    env.close()


# ------------------------------------------------------------------------------------------------ 3. sampling
def _host_copy(buf):
    ref = R.ReplayRef(buf.rows * buf.n_envs, buf.n_envs)
    for k in R.ReplayRef.FIELDS:
        setattr(ref, k, np.ascontiguousarray(getattr(buf, k).cpu().numpy()))
    ref.pos, ref.full = buf.pos, buf.full
    return ref


def _assert_samples(got, want, B, what):
    assert type(got).__name__ == "ReplayBufferSamples"
    assert got._fields == ("observations", "actions", "next_observations", "dones", "rewards")
    shapes = dict(observations=(B, 18), actions=(B, 3), next_observations=(B, 18), dones=(B, 1), rewards=(B, 1))
    for k in got._fields:
        g = getattr(got, k)
        assert g.is_cuda and tuple(g.shape) == shapes[k] and g.is_contiguous(), (what, k)
        g = g.cpu().numpy()
        assert g.dtype == np.float32 and R.same_bits(g, getattr(want, k)), (what, k)


@pytest.mark.parametrize("fill", ["partly", "full"])
def test_sample_and_gather_equal_the_restatement(envs, fill):
    import torch
    n, rows = 1000, 50
    env = envs(n)
    buf, _ = _buffer(env, rows, pattern=False)
    for call, T in enumerate((20,) if fill == "partly" else (20, 45)):
        h = R.synthetic(T, n, seed=77 + call)
        out, obs0 = _actor_dict(torch, h)
        buf.add_rollout(out, obs0=obs0)
    assert buf.full == (fill == "full") and buf.size() == (20 if fill == "partly" else rows)
    host = _host_copy(buf)
    for B in (1, 100, 256, 1000, 65536):
        seed, counter = (9 << 32) | B, (1 << 33) + B
        got, rows_d, envs_d = buf.sample(B, seed=seed, counter=counter, return_indices=True)
        assert rows_d.dtype == torch.int32 and envs_d.dtype == torch.int32 and rows_d.shape == envs_d.shape == (B,)
        r, e = rows_d.cpu().numpy(), envs_d.cpu().numpy()
        r_ref, e_ref = R.draw_indices(seed, counter, B, buf.size(), n)
        assert np.array_equal(r, r_ref) and np.array_equal(e, e_ref), B
        assert r.min() >= 0 and r.max() < buf.size() and e.min() >= 0 and e.max() < n
        _assert_samples(got, host.get_samples(r, e), B, f"sample B={B}")
        again = buf.sample(B, seed=seed, counter=counter)
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(got, again))
        _, r2, e2 = buf.sample(B, seed=seed, counter=counter + 1, return_indices=True)
        assert not (torch.equal(r2, rows_d) and torch.equal(e2, envs_d))
        if B >= 1000:
            assert len(np.unique(r)) == buf.size()
    # explicit indices: repeated ones, the last row and the last env
    b = np.array([0, 0, rows - 1, rows - 1, 3, 3, 3, buf.size() - 1] + list(range(rows)) * 3, np.int32)
    e = np.array([0, 0, n - 1, 0, n - 1, 5, 5, n - 1] + [n - 1, 0, 17] * rows, np.int32)
    got = buf.gather(torch.from_numpy(b).cuda(), torch.from_numpy(e).cuda())
    _assert_samples(got, host.get_samples(b, e), len(b), "gather")
    trunc = (host.dones != 0) & (host.timeouts != 0)
    assert trunc.any() and not host.get_samples(*np.nonzero(trunc)).dones.any()


# ------------------------------------------------------------------------------------------------ 4. 64-bit offsets
def test_store_beyond_4_gib(envs):
    import torch
    n = 4096
    env = envs(n)
    from reinforcementlearning4meshgeneration_amd import DeviceReplayBuffer
    rec = env._L.meshenv_replay_record_floats()
    rows = (2 ** 32) // (n * rec * 4) + 104          # 5565 rows at 48 floats per record, 4200 at 64
    buf = DeviceReplayBuffer(env, buffer_size=rows * n)
    assert buf.store.numel() * 4 > 2 ** 32
    ref_rows = {}
    buf.pos = rows - 2                                # the write covers the last two rows and wraps to row 0
    h = R.synthetic(3, n, seed=64)
    out, obs0 = _actor_dict(torch, h)
    buf.add_rollout(out, obs0=obs0, scale_actions=False)
    assert (buf.pos, buf.full) == (1, True)
    small = R.ReplayRef(3 * n, n)
    small.add_rollout(**h)
    for i, row in enumerate((rows - 2, rows - 1, 0)):
        for k in R.ReplayRef.FIELDS:
            assert R.same_bits(getattr(buf, k)[row].cpu().numpy(), getattr(small, k)[i]), (row, k)
        ref_rows[row] = i
    for row in (1, rows // 2, rows - 3):              # untouched rows are still the zeros they were allocated as
        assert not buf.store[row].view(torch.int32).any()
    b = np.array([rows - 1, 0, rows - 2, rows - 1, 0], np.int32)
    e = np.array([n - 1, 0, 1234, 0, n - 1], np.int32)
    got = buf.gather(torch.from_numpy(b).cuda(), torch.from_numpy(e).cuda())
    want = small.get_samples(np.array([ref_rows[x] for x in b]), e)
    _assert_samples(got, want, len(b), "gather beyond 4 GiB")
    del buf
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ 5. SB3's add
def test_sb3_signature_add_with_numpy_inputs(envs):
    n, rows = 17, 5
    env = envs(n)
    buf, ref = _buffer(env, rows)
    h = R.synthetic(8, n, seed=5)
    last = h["obs0"]
    for t in range(8):
        done = h["done"][t] != 0
        infos = [{"is_complete": bool(c)} for c in h["complete"][t]]
        for k in np.nonzero(done)[0]:
            infos[k] = {"is_complete": bool(h["complete"][t][k]), "terminal_observation": h["terminal_obs"][t][k],
                        "TimeLimit.truncated": not bool(h["complete"][t][k])}
        next_obs = np.where(done[:, None], h["terminal_obs"][t], h["obs_after"][t])
        rew = h["reward"][t].astype(np.float32)
        buf.add(last, next_obs, h["actions"][t], rew, done, infos)
        ref.add_sb3(last, next_obs, h["actions"][t], rew, done, infos)
        last = h["obs_after"][t]
        _assert_state(buf, ref, f"sb3 add step {t}")
    assert ref.timeouts.any() and ref.full


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_c_abi_refusals(envs):
    import torch
    from reinforcementlearning4meshgeneration_amd import _capi
    n = 17
    env = envs(n)
    L, hdl = env._L, env._handle
    rec = L.meshenv_replay_record_floats()
    rows, T, B = 4, 2, 8
    f32 = dict(dtype=torch.float32, device="cuda")
    store = torch.zeros((rows, n, rec), **f32)
    a = dict(obs0=torch.zeros((n, 18), **f32), obs_after=torch.zeros((T, n, 18), **f32), tobs=torch.zeros((T, n, 18), **f32),
             act=torch.zeros((T, n, 3), **f32), rew=torch.zeros((T, n), dtype=torch.float64, device="cuda"),
             done=torch.zeros((T, n), dtype=torch.uint8, device="cuda"), comp=torch.zeros((T, n), dtype=torch.uint8, device="cuda"))

    def add(T=T, rows=rows, pos=0, store=store.data_ptr(), **over):
        p = {k: v.data_ptr() for k, v in a.items()}
        p.update(over)
        return L.meshenv_replay_add(hdl, T, p["obs0"], p["obs_after"], p["tobs"], p["act"], p["rew"], p["done"], p["comp"], None, 1,
                                    store, rows, pos)

    def refused(rc, name):
        msg = L.meshenv_last_error(hdl)
        assert rc == _capi.E_ARG and msg.decode().startswith(name + ":"), (rc, msg)

    assert add() == 0
    for kw in (dict(T=0), dict(T=-3), dict(rows=0), dict(pos=-1), dict(pos=rows), dict(store=None), dict(store=store.data_ptr() + 4),
               *[{k: None} for k in a], dict(obs_after=store.data_ptr()), dict(done=store.data_ptr() + 64)):
        refused(add(**kw), "meshenv_replay_add")

    o = dict(obs=torch.zeros((B, 18), **f32), act=torch.zeros((B, 3), **f32), nxt=torch.zeros((B, 18), **f32),
             dones=torch.zeros((B, 1), **f32), rew=torch.zeros((B, 1), **f32))
    idx = torch.zeros(B, dtype=torch.int32, device="cuda")
    idx2 = torch.zeros(B, dtype=torch.int32, device="cuda")

    def sample(rows=rows, size=2, batch=B, store=store.data_ptr(), rows_in=None, envs_in=None, rows_out=None, envs_out=None, **over):
        p = {k: v.data_ptr() for k, v in o.items()}
        p.update(over)
        return L.meshenv_replay_sample(hdl, store, rows, size, batch, C.c_uint64(1), C.c_uint64(2), rows_in, envs_in, p["obs"],
                                       p["act"], p["nxt"], p["dones"], p["rew"], rows_out, envs_out)

    assert sample() == 0
    assert sample(rows_in=idx.data_ptr(), envs_in=idx2.data_ptr(), rows_out=None) == 0
    for kw in (dict(batch=0), dict(batch=-1), dict(rows=0), dict(size=0), dict(size=rows + 1), dict(store=None),
               *[{k: None} for k in o], dict(rows_in=idx.data_ptr()), dict(envs_in=idx.data_ptr()),
               dict(obs=store.data_ptr()), dict(rew=store.data_ptr() + 16), dict(rows_out=store.data_ptr()),
               dict(nxt=o["obs"].data_ptr()), dict(dones=o["rew"].data_ptr()), dict(rows_out=idx.data_ptr(), envs_out=idx.data_ptr()),
               dict(rows_in=idx.data_ptr(), envs_in=idx2.data_ptr(), rows_out=idx.data_ptr())):
        refused(sample(**kw), "meshenv_replay_sample")
    torch.cuda.synchronize()


def test_python_refusals(envs):
    import torch
    from reinforcementlearning4meshgeneration_amd import DeviceReplayBuffer, MeshEnvError  # noqa: F401
    n = 17
    env = envs(n)
    with pytest.raises(ValueError, match="optimize_memory_usage"):
        DeviceReplayBuffer(env, buffer_size=100, optimize_memory_usage=True)
    with pytest.raises(ValueError, match="buffer_size"):
        DeviceReplayBuffer(env, buffer_size=0)
    buf = DeviceReplayBuffer(env, buffer_size=3)
    assert buf.rows == 1                                   # buffer_size < n_envs keeps one row, as SB3 does
    buf = DeviceReplayBuffer(env, buffer_size=4 * n)
    with pytest.raises(ValueError, match="empty"):
        buf.sample(10)
    with pytest.raises(ValueError, match="empty"):
        buf.gather(torch.zeros(2, dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda"))
    h = R.synthetic(3, n, seed=1)
    out, obs0 = _actor_dict(torch, h)
    with pytest.raises(ValueError, match="obs0"):
        buf.add_rollout(out)
    with pytest.raises(ValueError, match="terminal_obs"):
        buf.add_rollout({k: v for k, v in out.items() if k != "terminal_obs"}, obs0=obs0)
    with pytest.raises(ValueError, match="reward"):
        buf.add_rollout(dict(out, reward=out["reward"].float()), obs0=obs0)
    with pytest.raises(ValueError, match="shape"):
        buf.add_rollout(dict(out, complete=out["complete"][:2]), obs0=obs0)
    with pytest.raises(ValueError, match="obs0"):
        buf.add_rollout(out, obs0=obs0.cpu())
    with pytest.raises(ValueError, match="contiguous"):
        buf.add_rollout(dict(out, obs=out["obs"].transpose(0, 1).contiguous().transpose(0, 1)), obs0=obs0)
    with pytest.raises(ValueError, match="high > low"):
        buf.add_rollout(out, obs0=obs0, scale_actions=([0, 0, 0], [1, 0, 1]))
    pol = _policy_dict(torch, h)
    with pytest.raises(ValueError, match="obs0"):
        buf.add_rollout(pol, obs0=obs0)
    with pytest.raises(ValueError, match="block"):
        buf.add_rollout(dict(pol, obs=pol["obs"].clone()))
    with pytest.raises(ValueError, match="collect_rollout or step_actor_T"):
        buf.add_rollout([1, 2])
    assert buf.pos == 0 and not buf.full                   # nothing was stored by a refused call
    buf.add_rollout(out, obs0=obs0)
    with pytest.raises(ValueError, match="VecNormalize"):
        buf.sample(4, env=object())
    with pytest.raises(ValueError, match="batch_size"):
        buf.sample(0)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device="cuda")   # noqa: E731
    with pytest.raises(ValueError, match="int32"):
        buf.gather(torch.zeros(2, dtype=torch.int64, device="cuda"), i32(0, 0))
    with pytest.raises(ValueError, match="same"):
        buf.gather(i32(0, 1), i32(0))
    for b, e in ((i32(0, 4), i32(0, 0)), (i32(-1, 0), i32(0, 0)), (i32(0, 0), i32(0, n)), (i32(0, 0), i32(-1, 0))):
        with pytest.raises(ValueError, match="out of range"):
            buf.gather(b, e)
    with pytest.raises(ValueError, match="infos"):
        buf.add(h["obs0"], h["obs0"], h["actions"][0], h["reward"][0], h["done"][0], [{}])
    with pytest.raises(ValueError, match="add:"):
        buf.add(h["obs0"][:3], h["obs0"], h["actions"][0], h["reward"][0], h["done"][0], [{}] * n)


# ------------------------------------------------------------------------------------------------ 7. stream order
def test_back_to_back_calls_need_no_synchronisation():
    import torch
    from reinforcementlearning4meshgeneration_amd import DeviceReplayBuffer, MeshVecEnv, boundary
    n, T = 1000, 40
    policy = _td3(torch)
    results = []
    for sync in (False, True):
        env = MeshVecEnv([boundary(0)], n_envs=n)
        buf = DeviceReplayBuffer(env, buffer_size=64 * n)
        env.reset_tensor()
        wait = torch.cuda.synchronize if sync else (lambda: None)
        got = []
        for call in range(3):
            out = env.collect_rollout(policy, T, seed=3, counter=call * T)
            wait()
            buf.add_rollout(out)
            wait()
            got.append(buf.sample(4096, seed=21, counter=call, return_indices=True))
            wait()
        torch.cuda.synchronize()
        results.append(([x.cpu().numpy() for s, r, e in got for x in (*s, r, e)], buf.store.cpu().numpy()))
        env.close()
    policy.close()
    (a, sa), (b, sb) = results
    assert np.array_equal(sa.view(np.int32), sb.view(np.int32)) and sa.any()
    assert len(a) == len(b) == 21
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))
