"""GPU: the update and reward-helper wavefronts of the CU-group step kernel, bit for bit against the one-wave kernel.

Phase 2 of k_step_group keeps its wave-uniform fp64 values -- the reference vertex and its right neighbour, base length,
target length, the bisector, the boundary-quality sums, the state handed over in LDS -- in vector registers instead of
forcing each through the scalar file (csrc/meshenv_kernels.h: vu_f64, env_apply<true>, find_next_state<true>,
reward_on_helper), and does not read back the Decision fields whose value the checks fix.  None of this may change a
result.  Every case drives a CU-group handle of two workgroups (MESHENV_GROUP = 16 / 8, read once by meshenv_create) and,
per workgroup, one handle on the one-wave k_step (MESHENV_GROUP = 1) holding that workgroup's environments, with the same
action rows, and compares observation, reward, done, complete and terminal_obs after every step, and the full state of
every environment (meshenv_get_state) and the work counters at the end.  Environments are independent, so the reference
handle of a workgroup also COUNTS that workgroup: the growth of its `valid` counter over a step is m, the number of updates
the workgroup's barrier finds pending -- which selects the path phase 2 takes (csrc/meshenv_kernels.h, step_group_body):
1 <= m, 2m <= G: every update gets a reward helper; m >= 5: some SIMD runs two updates; 2m > G: no helpers, the update
waves compute the reward themselves.

Two action streams on boundary(), 400 steps: uniform over the action box, and the suite's biased generator (60 % of the rows
redrawn from the box valid extractions come from).  Seed 3 was chosen with the CPU oracle (oracle.ref_lib.RefBatch, m per
workgroup and step counted from n_elem): G = 16, biased: m >= 5 in 100 steps, m = 9 (2m > G) in one, 53 episodes end;
G = 16, uniform: m <= 7, helpers in 392 steps; G = 8: biased m >= 5 (2m > G) in 6 steps, uniform in 1; d1, 100 steps:
m >= 5 in 50 steps, m = 9 in two.  The tests assert the occurrences from the counters, so none passes without them."""
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

SEED = 3
STATE_KEYS = ("n", "ring_ids", "ring_xy", "cand_key", "cand_stamp", "ref_index", "n_elem", "failed_num", "n_vert", "status",
              "domain", "n0", "current_area", "base_length")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    return torch


def _uniform(rng, T, n):
    return rng.uniform([-1, -1.5, 0], [1, 1.5, 1.5], size=(T, n, 3)).astype(np.float32)


def _biased(rng, T, n, frac=0.6):
    """tests/test_gpu_configs.py's generator."""
    a = rng.uniform([-1, -1.5, 0], [1, 1.5, 1.5], size=(T, n, 3))
    pick = rng.random((T, n)) < frac
    b = np.stack([rng.uniform(-1, 1, (T, n)), rng.uniform(0.2, 1.0, (T, n)), rng.uniform(0.3, 1.2, (T, n))], axis=2)
    a[pick] = b[pick]
    return a.astype(np.float32)


def _make(group, dom, n):
    from reinforcementlearning4meshgeneration_amd import MeshVecEnv
    before = os.environ.get("MESHENV_GROUP")
    os.environ["MESHENV_GROUP"] = str(group)      # read once, by meshenv_create
    try:
        return MeshVecEnv([dom], n_envs=n)
    finally:
        if before is None:
            del os.environ["MESHENV_GROUP"]
        else:
            os.environ["MESHENV_GROUP"] = before


def _bits(torch, x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x.view(torch.int64) if x.dtype == torch.float64 else x


def _same_state(sa, sb, where):
    for k in STATE_KEYS:
        a, b = sa[k], sb[k]
        if isinstance(a, np.ndarray):
            same = a.shape == b.shape and np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a,
                                                         b.view(np.int64) if b.dtype == np.float64 else b)
        elif isinstance(a, float):
            same = np.float64(a).view(np.int64) == np.float64(b).view(np.int64)
        else:
            same = a == b
        assert same, (where, k, a, b)


def _lockstep(torch, dom, G, want_kernel, acts):
    """Two workgroups of G envs on the CU-group kernel against one k_step handle per workgroup; returns m per (step, workgroup)."""
    T, n = acts.shape[0], 2 * G
    got = _make(G, dom, n)
    refs = [_make(1, dom, G) for _ in range(2)]
    try:
        assert got.step_kernel == want_kernel, got.step_kernel
        assert all("k_step<" in r.step_kernel for r in refs), refs[0].step_kernel
        got.reset()
        for w, r in enumerate(refs):
            r.reset()
            assert torch.equal(_bits(torch, r.obs), _bits(torch, got.obs[w * G:(w + 1) * G]))
        a = torch.from_numpy(acts).cuda()
        m = np.zeros((T, 2), np.int64)
        seen = [0, 0]
        finished = 0
        for t in range(T):
            o1, r1, d1, c1 = got.step(a[t])
            for w, r in enumerate(refs):
                s = slice(w * G, (w + 1) * G)
                o0, r0, d0, c0 = r.step(a[t, s].contiguous())
                for name, x, y in (("obs", o0, o1[s]), ("reward", r0, r1[s]), ("done", d0, d1[s]), ("complete", c0, c1[s]),
                                   ("terminal_obs", r.terminal_obs, got.terminal_obs[s])):
                    assert torch.equal(_bits(torch, x), _bits(torch, y)), (name, t, w)
                v = r.counters()["valid"]
                m[t, w] = v - seen[w]
                seen[w] = v
            finished += int(d1.sum())
        k = got.counters()
        ks = [r.counters() for r in refs]
        assert k == {key: ks[0][key] + ks[1][key] for key in k}, (k, ks)
        assert k["steps"] == T * n and k["valid"] == int(m.sum())
        for e in range(n):
            _same_state(refs[e // G].get_state(e % G), got.get_state(e), (want_kernel, e))
        print(want_kernel, "steps", T, "extractions", k["valid"], "finished episodes", finished, "m histogram", np.bincount(m.ravel()).tolist())
        return m, finished
    finally:
        got.close()
        for r in refs:
            r.close()


def _d1():
    d1 = [tuple(p) for p in np.load(os.path.join(GOLDEN_DIR, "boundary16_biased_s2.npz"))["domain_xy"]]
    assert len(d1) == 120
    return d1


@pytest.mark.parametrize("G", [16, 8])
def test_uniform_stream_helper_path(torch_cuda, G):
    """Uniform actions (valid rate ~0.11): nearly every step deals one to four updates, each with a reward helper."""
    from reinforcementlearning4meshgeneration_amd.domains import boundary
    m, finished = _lockstep(torch_cuda, boundary(0), G, f"meshenv::k_step_group<{G}, true, false, true>",
                            _uniform(np.random.default_rng(SEED), 400, 2 * G))
    helped = (m >= 1) & (2 * m <= G) & (m <= 8)
    assert int(helped.any(axis=1).sum()) >= 300 and int(((m >= 2) & (m <= 4)).sum()) >= 50, np.bincount(m.ravel())
    assert finished >= 10


@pytest.mark.parametrize("G", [16, 8])
def test_biased_stream_five_pending_updates_and_no_helpers(torch_cuda, G):
    """Biased actions: steps with five and more pending updates in one workgroup (two updates on one SIMD), and steps with
    2m > G, where no helper is dealt and the update waves compute the reward themselves."""
    from reinforcementlearning4meshgeneration_amd.domains import boundary
    m, finished = _lockstep(torch_cuda, boundary(0), G, f"meshenv::k_step_group<{G}, true, false, true>",
                            _biased(np.random.default_rng(SEED), 400, 2 * G))
    assert int((m >= 5).sum()) >= 1, np.bincount(m.ravel())
    assert int((2 * m > G).sum()) >= 1, np.bincount(m.ravel())
    assert int(((m >= 1) & (2 * m <= G)).sum()) >= 100
    assert finished >= 10


def test_long_rings_general_instantiation(torch_cuda):
    """d1 (120 vertices, two 64-slot chunks), G = 16, 100 biased steps: the instantiation without the ring-stride assumption."""
    m, _ = _lockstep(torch_cuda, _d1(), 16, "meshenv::k_step_group<16, true, false, false>",
                     _biased(np.random.default_rng(SEED), 100, 32))
    assert int((m >= 5).sum()) >= 1 and int((2 * m > 16).sum()) >= 1 and int(((m >= 1) & (2 * m <= 16)).sum()) >= 50, np.bincount(m.ravel())


@pytest.mark.parametrize("small", [True, False])
def test_fused_actor_kernel_follows(torch_cuda, small):
    """k_step_group_actor shares the body: 50 closed-loop steps of the fused launch (two workgroups, MESHENV_GROUP = 16)
    against step() on k_step followed by k_actor_forward, as tests/test_gpu_actor.py does at 4096 envs."""
    torch = torch_cuda
    from reinforcementlearning4meshgeneration_amd.actor import FusedActor
    from reinforcementlearning4meshgeneration_amd.domains import boundary
    torch.manual_seed(7)
    lin = [torch.nn.Linear(18, 128), torch.nn.Linear(128, 128), torch.nn.Linear(128, 128)]
    mu, ls = torch.nn.Linear(128, 3), torch.nn.Linear(128, 3)
    with torch.no_grad():
        mu.weight.mul_(6.0)
        ls.bias.fill_(-0.5)
    actor = FusedActor.from_torch(lin, mu, ls)
    dom, n = (boundary(0) if small else _d1()), 32
    a_env, b_env = _make(1, dom, n), _make(16, dom, n)
    try:
        assert "k_step<" in a_env.step_kernel and "k_step_group<16" in b_env.step_kernel, (a_env.step_kernel, b_env.step_kernel)
        obs_a = a_env.reset()
        b_env.reset()
        act_a = actor.sample(obs_a, seed=5, counter=0).clone()
        act_b = act_a.clone()
        for t in range(50):
            o1, r1, d1f, c1 = [x.clone() for x in a_env.step(act_a)]
            act_a = actor.sample(o1, seed=5, counter=t + 1).clone()
            o2, r2, d2f, c2, nxt = b_env.step_actor(actor, act_b, seed=5, counter=t + 1)
            for name, x, y in (("obs", o1, o2), ("reward", r1, r2), ("done", d1f, d2f), ("complete", c1, c2), ("actions", act_a, nxt)):
                assert torch.equal(_bits(torch, x), _bits(torch, y)), (name, t)
            act_b = nxt
        ka, kb = a_env.counters(), b_env.counters()
        assert ka == kb and ka["valid"] >= 32, (ka, kb)
        for e in range(n):
            _same_state(a_env.get_state(e), b_env.get_state(e), ("actor", small, e))
    finally:
        a_env.close()
        b_env.close()
        actor.close()
