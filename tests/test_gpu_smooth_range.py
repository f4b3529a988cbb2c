"""GPU: the three smoothing kernels (k_smooth_interior, k_smooth_final, k_smooth_front + the rebuild) in lockstep with the
CPU oracle on scaled and shifted domains, x -> scale x + shift.

The smoothers promise the reference's vertex tables bit for bit, and their exactness argument depends on magnitude: both
relaxations stop on |sum(x + y) - previous sum| <= 0.001, an absolute threshold on a serially accumulated sum (under a
shift of 1e8 one ulp of that sum is of the order of 1e-6, so the sweep count hangs on the summation order; scaled up the
sweeps run longer, scaled down they collapse), the front smoother squares with the restated libm pow(x, 2.0) and builds
vertices through tan / cos / sqrt, smooth() estimates vertices through atan2 / sin / cos.  tests/test_gpu_smooth.py has
the replays of the reference's own records (the *_xf_* fixtures among them); here: batches against oracle.ref_lib under
five transforms, and the 64-vertex chunks past the first of the serial sums, of build_segment_lists and of the level
fixpoint (more than 128 generated vertices in one call)."""
import os
import time

import numpy as np
import pytest

from conftest import GOLDEN_DIR
from test_gpu_geometry_range import TRANSFORMS
from test_gpu_smooth import SMOOTH_FINAL_M0, _biased, _golden_domain

pytestmark = pytest.mark.gpu

SMOOTH_TRANSFORMS = [t for t in TRANSFORMS if t[0] in ("x1em2", "x1e2", "dx1e6", "dx1e8", "x1e3_d1e6")]
_IDS = [t[0] for t in SMOOTH_TRANSFORMS]
assert len(SMOOTH_TRANSFORMS) == 5


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    return torch


def _xf(ring, scale, dx, dy):
    return [(scale * float(x) + dx, scale * float(y) + dy) for x, y in ring]


def _interior_domains():
    from reinforcementlearning4meshgeneration_amd import boundary
    return [boundary(0), _golden_domain("boundary16_biased_s2"), _golden_domain("random1_1_biased_s1")]


_plain_interior_max = []


def _oracle_interior_max_sweeps_untransformed():
    """The largest sweep count of the interior batch below run untransformed, in the oracle alone (computed once)."""
    if not _plain_interior_max:
        _plain_interior_max.append(_interior_batch(None, None, _interior_domains())["max_sweeps"])
    return _plain_interior_max[0]


def _compare_interior_call(env, refs, sweeps, sample, where):
    """One smooth_pave(interior=True) call already made on the device: the oracle's call on every env (sweeps of ALL
    envs equal), element / vertex tables bit-equal and the candidate list equal on the sampled envs.  Returns the
    oracle's sweep counts."""
    ref_sw = np.array([e.smooth_interior(400)[0] for e in refs], np.int32)
    assert np.array_equal(sweeps, ref_sw), (where, np.nonzero(sweeps != ref_sw)[0][:8], sweeps[sweeps != ref_sw][:8],
                                             ref_sw[sweeps != ref_sw][:8])
    for k in sample:
        q, v = env.get_elements(int(k))
        q_ref, v_ref = refs[int(k)].elements()
        assert np.array_equal(q, q_ref), (where, k)
        assert np.array_equal(v, v_ref), (where, k, float(np.abs(v - v_ref).max()))
        st = env.get_state(int(k))
        ids, keys = refs[int(k)].candidates()
        assert np.array_equal(st["cand_order_ids"], ids), (where, k)
        assert np.abs(st["cand_order_keys"] - keys).max(initial=0) <= 1e-9, (where, k)
    return ref_sw


def _interior_batch(torch, tid, doms):
    """384 envs mixed over the domains, 40 steps, smooth_pave(iteration=400) every 10.  torch None: the oracle alone."""
    from oracle.ref_lib import RefBatch, RefEnv
    n, T, every = 384, 40, 10
    env_domain = (np.arange(n) % len(doms)).astype(np.int32)
    refs = [RefEnv.from_points(doms[env_domain[k]], cap_new=256) for k in range(n)]
    batch = RefBatch(refs)
    env = None
    if torch is not None:
        from reinforcementlearning4meshgeneration_amd import MeshVecEnv
        env = MeshVecEnv(doms, env_domain=env_domain, log_capacity=256, auto_reset=True)
        assert np.array_equal(env.reset().cpu().numpy(), batch.reset())
    else:
        batch.reset()
    rng = np.random.default_rng(77)
    out = dict(calls=0, moved_envs=0, max_sweeps=0, max_n_new=0, max_obs=0.0)
    for t in range(T):
        a = _biased(rng, n)
        o_ref, r_ref, d_ref, c_ref = batch.step(a, auto_reset=True, threads=16)
        if env is not None:
            o, r, d, c = env.step(torch.from_numpy(a).cuda())
            assert np.array_equal(d.cpu().numpy(), d_ref) and np.array_equal(c.cpu().numpy(), c_ref), (tid, t)
            err = float(np.abs(o.cpu().numpy().astype(np.float64) - o_ref).max())
            out["max_obs"] = max(out["max_obs"], err)
            assert err <= 1e-5, (tid, t, err)
            assert np.abs(r.cpu().numpy() - r_ref).max() <= 1e-5, (tid, t)
        if (t + 1) % every == 0:
            if env is not None:
                sweeps, _ = env.smooth_pave(iteration=400)
                sample = rng.choice(n, size=48, replace=False)
                ref_sw = _compare_interior_call(env, refs, sweeps.cpu().numpy(), sample, (tid, t))
            else:
                rng.choice(n, size=48, replace=False)      # the same action stream as the device run
                ref_sw = np.array([e.smooth_interior(400)[0] for e in refs], np.int32)
            out["calls"] += 1
            out["moved_envs"] += int((ref_sw > 1).sum())
            out["max_sweeps"] = max(out["max_sweeps"], int(ref_sw.max()))
            out["max_n_new"] = max(out["max_n_new"], max(e.scalars()["n_vert"] - e.n0 for e in refs))
    if env is not None:
        env.close()
    return out


@pytest.mark.parametrize("tid,scale,dx,dy", SMOOTH_TRANSFORMS, ids=_IDS)
def test_interior_smoothing_on_transformed_domains_lockstep_with_oracle(torch_cuda, tid, scale, dx, dy):
    """k_smooth_interior + the rebuild on transformed boundary(0) / boundary16 / random1_1: sweep counts of all 384 envs,
    vertex tables (bit for bit) and candidate lists of 48 sampled envs at each of the 4 calls, trajectories within 1e-5
    in between and after."""
    t0 = time.time()
    doms = [_xf(r, scale, dx, dy) for r in _interior_domains()]
    st = _interior_batch(torch_cuda, tid, doms)
    plain = _oracle_interior_max_sweeps_untransformed()
    print(f"{tid}: interior calls {st['calls']}, envs with > 1 sweep {st['moved_envs']}, max sweeps {st['max_sweeps']} "
          f"(untransformed, oracle: {plain}), largest n_new {st['max_n_new']}, vertex deviation 0 (bit-equal), "
          f"largest obs error {st['max_obs']:.3g} in {time.time() - t0:.1f} s")
    assert st["moved_envs"] > 0
    if tid in ("x1e2", "x1e3_d1e6"):       # the absolute 0.001 stop rule: a scaled-up mesh needs more sweeps
        assert st["max_sweeps"] > plain, (st["max_sweeps"], plain)


def _compare_front_call(env, refs, sweeps, obs_after, vertex_envs, where):
    """One smooth_pave(interior=False) call already made on the device against smooth_pave_full of the oracle on every
    env: code, sweeps, observation (as float32) equal; vertex tables of vertex_envs bit-equal.  Returns the sweeps."""
    from reinforcementlearning4meshgeneration_amd import _capi
    ref_sw = np.zeros(len(refs), np.int32)
    for k, ref in enumerate(refs):
        code, sw, o_ref = ref.smooth_pave_full(400)
        # on these domains the reference never raises inside the front smoother: every env has an observation afterwards
        assert code == 0, (where, k, code)
        assert int(sweeps[k]) == sw, (where, k, int(sweeps[k]), sw)
        assert not (env.get_state(k)["status"] & _capi.ST_NO_REFERENCE), (where, k)
        assert np.array_equal(obs_after[k], o_ref.astype(np.float32)), (where, k)
        ref_sw[k] = sw
    worst = 0.0
    for k in vertex_envs:
        q, v = env.get_elements(int(k))
        q_ref, v_ref = refs[int(k)].elements()
        assert np.array_equal(q, q_ref), (where, k)
        worst = max(worst, float(np.abs(v - v_ref).max()))
    assert env.libm_exact == 1, "this libm's pow differs from the restated one (regenerate csrc/meshenv_libm_tables.h)"
    assert worst == 0.0, (where, worst)
    return ref_sw


@pytest.mark.parametrize("tid,scale,dx,dy", SMOOTH_TRANSFORMS, ids=_IDS)
def test_front_smoothing_on_transformed_domains_lockstep_with_oracle(torch_cuda, tid, scale, dx, dy):
    """k_smooth_front + the interior relaxation + the rebuild + find_next_state on transformed boundary(0), 256 envs: code,
    sweeps and observation of every env, vertex tables of 32 envs bit for bit; then 30 steps through the tie-breaking
    k_step instantiation with no differing observation entry."""
    torch = torch_cuda
    from oracle.ref_lib import RefBatch, RefEnv
    from reinforcementlearning4meshgeneration_amd import MeshVecEnv, boundary
    t0 = time.time()
    n = 256
    dom = _xf(boundary(0), scale, dx, dy)
    env = MeshVecEnv([dom], n_envs=n, auto_reset=True, log_capacity=96)
    refs = [RefEnv.from_points(dom, cap_new=96) for _ in range(n)]
    batch = RefBatch(refs)
    assert np.array_equal(env.reset().cpu().numpy(), batch.reset())
    rng = np.random.default_rng(33)
    differing = 0
    for t in range(40):
        a = _biased(rng, n)
        o, r, d, c = env.step(torch.from_numpy(a).cuda())
        o_ref, r_ref, d_ref, c_ref = batch.step(a, auto_reset=True, threads=16)
        assert np.array_equal(d.cpu().numpy(), d_ref) and np.array_equal(c.cpu().numpy(), c_ref), (tid, t)
        assert np.abs(o.cpu().numpy().astype(np.float64) - o_ref).max() <= 1e-5, (tid, t)
    sweeps, _ = env.smooth_pave(iteration=400, interior=False)
    sweeps = sweeps.cpu().numpy().copy()
    obs_after = env.obs.cpu().numpy().copy()
    ref_sw = _compare_front_call(env, refs, sweeps, obs_after, range(0, n, 8), tid)
    max_n_new = max(e.scalars()["n_vert"] - e.n0 for e in refs)
    assert env._L.meshenv_step_kernel(env._handle) == 3
    assert env.step_kernel == "meshenv::k_step<false, true, true, false, false>", env.step_kernel
    for t in range(30):
        a = _biased(rng, n)
        o, r, d, c = env.step(torch.from_numpy(a).cuda())
        o_ref, r_ref, d_ref, c_ref = batch.step(a, auto_reset=True, threads=16)
        assert np.array_equal(d.cpu().numpy(), d_ref) and np.array_equal(c.cpu().numpy(), c_ref), (tid, t)
        differing += int((o.cpu().numpy() != o_ref.astype(np.float32)).sum())
    print(f"{tid}: front smoothing sweeps mean {ref_sw.mean():.2f} max {int(ref_sw.max())}, envs with > 1 sweep "
          f"{int((ref_sw > 1).sum())}, largest n_new {max_n_new}, vertex deviation 0 on 32 envs, differing observation "
          f"entries in 30 later steps {differing} in {time.time() - t0:.1f} s")
    assert differing == 0
    assert (ref_sw > 1).any()
    env.close()


def _final_tol(doms):
    """The smooth() vertex tolerance of tests/test_gpu_smooth.py: 1e-11 at coordinates up to M0, the same number of ulps
    at the transformed domains' largest |coordinate| M."""
    M = max(float(np.abs(np.asarray(d)).max()) for d in doms)
    return 1e-11 * M / SMOOTH_FINAL_M0, M


@pytest.mark.parametrize("tid,scale,dx,dy", SMOOTH_TRANSFORMS, ids=_IDS)
def test_finished_mesh_smoothing_on_transformed_domains_against_oracle(torch_cuda, tid, scale, dx, dy):
    """k_smooth_final on the transformed ring13 (fronts of 5) and star (fronts of 4) domains, 512 envs without auto-reset
    until > 30 % have ended complete: sweeps of every finished env equal, vertex tables and rings of every 7th within
    the scaled tolerance, unfinished envs refused."""
    torch = torch_cuda
    from oracle.ref_lib import RefBatch, RefEnv
    from reinforcementlearning4meshgeneration_amd import MeshVecEnv, _capi
    t0 = time.time()
    doms = [_xf(_golden_domain("smoothfinal_ring13_s4"), scale, dx, dy),
            _xf(_golden_domain("smoothfinal_star_s6"), scale, dx, dy)]
    tol, M = _final_tol(doms)
    n, T = 512, 160
    env_domain = (np.arange(n) % 2).astype(np.int32)
    env = MeshVecEnv(doms, env_domain=env_domain, log_capacity=128, auto_reset=False)
    refs = [RefEnv.from_points(doms[env_domain[k]], cap_new=128) for k in range(n)]
    batch = RefBatch(refs)
    assert np.array_equal(env.reset().cpu().numpy(), batch.reset())
    rng = np.random.default_rng(12)
    finished = np.zeros(n, bool)
    for t in range(T):
        a = _biased(rng, n)
        o, r, d, c = env.step(torch.from_numpy(a).cuda())
        d = d.cpu().numpy().astype(bool); c = c.cpu().numpy().astype(bool)
        o_ref, r_ref, d_ref, c_ref = batch.step(a, auto_reset=False, threads=16)
        live = ~finished
        assert np.array_equal(d[live], d_ref[live].astype(bool)), (tid, t)
        newly = live & d
        trunc = newly & ~c
        if trunc.any():   # truncated by 100 failures: start over, in both
            env.reset(mask=torch.from_numpy(trunc.astype(np.uint8)).cuda())
            for k in np.nonzero(trunc)[0]:
                refs[k].reset()
        finished |= newly & c
        if finished.mean() > 0.7:
            break
    assert finished.sum() > 0.3 * n, finished.sum()
    sweeps, _ = env.smooth(mask=torch.ones(n, dtype=torch.uint8, device="cuda"), iteration=400)
    sweeps = sweeps.cpu().numpy()
    assert (sweeps[~finished] == _capi.SMOOTH_NOT_FINISHED).all()
    fin = np.nonzero(finished)[0]
    ref_sw = np.array([refs[k].smooth_final(400)[0] for k in fin], np.int32)
    assert np.array_equal(sweeps[fin], ref_sw), (tid, fin[sweeps[fin] != ref_sw][:8])
    worst = worst_ring = 0.0
    fronts = set()
    for k in fin[::7]:
        v = env.get_elements(int(k))[1]
        v_ref = refs[k].elements()[1]
        worst = max(worst, float(np.abs(v - v_ref).max()))
        st = env.get_state(int(k))
        fronts.add(st["n"])
        worst_ring = max(worst_ring, float(np.abs(st["ring_xy"] - refs[k].ring()[1]).max()))   # the front moved too
    print(f"{tid}: smooth() of {len(fin)} finished meshes after {t + 1} steps, fronts {sorted(fronts)}, sweeps mean "
          f"{ref_sw.mean():.2f} max {int(ref_sw.max())}, at the cap {int((ref_sw == 400).sum())}, largest vertex "
          f"deviation {worst} = {worst / np.spacing(M):.3g} ulps of M = {M} (tolerance {tol:.3g}), ring {worst_ring} "
          f"in {time.time() - t0:.1f} s")
    assert worst <= tol and worst_ring <= tol, (worst, worst_ring, tol)
    assert fronts == {4, 5}
    env.close()


def test_smooth_of_the_archived_episode_on_a_shifted_domain(torch_cuda):
    """meshenv_smooth_final(which = 1) under x -> 1e3 x + (1e6, -1e6): the archived episode of an auto-resetting batch
    against the running one of a batch without auto-reset on the same actions -- same sweeps, same tables, and the
    running one is the oracle's within the scaled tolerance."""
    torch = torch_cuda
    from oracle.ref_lib import RefBatch, RefEnv
    from reinforcementlearning4meshgeneration_amd import MeshVecEnv
    tid, scale, dx, dy = [t for t in SMOOTH_TRANSFORMS if t[0] == "x1e3_d1e6"][0]
    doms = [_xf(_golden_domain("smoothfinal_ring13_s4"), scale, dx, dy),
            _xf(_golden_domain("smoothfinal_star_s6"), scale, dx, dy)]
    tol, M = _final_tol(doms)
    n, T = 256, 60
    env_domain = (np.arange(n) % 2).astype(np.int32)
    a_env = MeshVecEnv(doms, env_domain=env_domain, log_capacity=128, auto_reset=False)
    b_env = MeshVecEnv(doms, env_domain=env_domain, log_capacity=128, auto_reset=True)
    refs = [RefEnv.from_points(doms[env_domain[k]], cap_new=128) for k in range(n)]
    batch = RefBatch(refs)
    a_env.reset(); b_env.reset(); batch.reset()
    rng = np.random.default_rng(31)
    checked = 0
    fronts = set()
    worst = 0.0
    max_sw = 0
    for t in range(T):
        a_np = _biased(rng, n)
        a = torch.from_numpy(a_np).cuda()
        _, _, d_a, c_a = a_env.step(a)
        _, _, d_b, c_b = b_env.step(a)
        _, _, d_ref, c_ref = batch.step(a_np, auto_reset=False, threads=16)
        assert torch.equal(d_a, d_b) and torch.equal(c_a, c_b), t
        assert np.array_equal(d_a.cpu().numpy(), d_ref) and np.array_equal(c_a.cpu().numpy(), c_ref), t
        fin = (d_a != 0) & (c_a != 0)
        if fin.any():
            sw_a, _ = a_env.smooth(mask=fin.to(torch.uint8), iteration=400, which="current")
            sw_a = sw_a.cpu().numpy().copy()
            sw_b, _ = b_env.smooth(mask=fin.to(torch.uint8), iteration=400, which="last")
            sw_b = sw_b.cpu().numpy().copy()
            idx = np.nonzero(fin.cpu().numpy())[0]
            assert np.array_equal(sw_a[idx], sw_b[idx]) and (sw_a[idx] >= 1).all(), t
            for k in idx:
                assert refs[k].smooth_final(400)[0] == sw_a[k], (t, k)
                max_sw = max(max_sw, int(sw_a[k]))
                qa, va = a_env.get_elements(int(k))
                le = b_env.get_last_episode(int(k))
                assert le["is_complete"] and np.array_equal(qa, le["quads"]) and np.array_equal(va, le["vertex_xy"]), (t, k)
                worst = max(worst, float(np.abs(va - refs[k].elements()[1]).max()))
                fronts.add(a_env.get_state(int(k))["n"])
                checked += 1
        ended = d_a != 0
        if ended.any():      # A and the oracle start over what ended, as B did by itself
            a_env.reset(mask=ended.to(torch.uint8))
            for k in np.nonzero(ended.cpu().numpy())[0]:
                refs[k].reset()
    print(f"{tid}: archived against running smooth(): meshes compared {checked}, fronts {sorted(fronts)}, max sweeps "
          f"{max_sw}, largest deviation from the oracle {worst} = {worst / np.spacing(M):.3g} ulps of M = {M}")
    assert checked > 50 and fronts == {4, 5}
    assert worst <= tol, (worst, tol)
    a_env.close(); b_env.close()


LARGE_LOG_TRANSFORMS = [("plain", 1.0, 0.0, 0.0)] + [t for t in SMOOTH_TRANSFORMS if t[0] == "dx1e6"]


@pytest.mark.parametrize("tid,scale,dx,dy", LARGE_LOG_TRANSFORMS, ids=[t[0] for t in LARGE_LOG_TRANSFORMS])
def test_smoothing_with_more_than_128_generated_vertices(torch_cuda, tid, scale, dx, dy):
    """64 envs on boundary16 stepped (truncated / finished episodes reset in both) until one holds more than 128 generated
    vertices: the interior smoother and then the front smoother against the oracle with the third 64-vertex chunk of the
    serial sums, of build_segment_lists and of the level fixpoint in use."""
    torch = torch_cuda
    from oracle.ref_lib import RefBatch, RefEnv
    from reinforcementlearning4meshgeneration_amd import MeshVecEnv
    t0 = time.time()
    n, bound = 64, 700
    dom = _xf(_golden_domain("boundary16_biased_s2"), scale, dx, dy)
    env = MeshVecEnv([dom], n_envs=n, auto_reset=False, log_capacity=512)
    refs = [RefEnv.from_points(dom, cap_new=512) for _ in range(n)]
    batch = RefBatch(refs)
    assert np.array_equal(env.reset().cpu().numpy(), batch.reset())
    rng = np.random.default_rng(5)
    n_new = np.zeros(n, int)
    for t in range(bound):
        a = _biased(rng, n)
        o, r, d, c = env.step(torch.from_numpy(a).cuda())
        o_ref, r_ref, d_ref, c_ref = batch.step(a, auto_reset=False, threads=16)
        d = d.cpu().numpy()
        assert np.array_equal(d, d_ref) and np.array_equal(c.cpu().numpy(), c_ref), (tid, t)
        assert np.abs(o.cpu().numpy().astype(np.float64) - o_ref).max() <= 1e-5, (tid, t)
        if d.any():
            env.reset(mask=torch.from_numpy(d.astype(np.uint8)).cuda())
            for k in np.nonzero(d)[0]:
                refs[k].reset()
        n_new = np.array([e.scalars()["n_vert"] - e.n0 for e in refs])
        if n_new.max() > 128:
            break
    assert n_new.max() > 128, f"largest n_new after {bound} steps: {int(n_new.max())}"
    big = int(n_new.argmax())
    assert env.get_state(big)["n_vert"] - env.get_state(big)["n0"] == n_new[big]
    sweeps, _ = env.smooth_pave(iteration=400)
    sw_int = _compare_interior_call(env, refs, sweeps.cpu().numpy(), range(n), (tid, "interior"))
    sweeps, _ = env.smooth_pave(iteration=400, interior=False)
    sw_front = _compare_front_call(env, refs, sweeps.cpu().numpy().copy(), env.obs.cpu().numpy().copy(), range(n),
                                   (tid, "front"))
    print(f"{tid}: after {t + 1} steps largest n_new {int(n_new.max())} (envs past 64: {int((n_new > 64).sum())}, past "
          f"128: {int((n_new > 128).sum())}); interior sweeps max {int(sw_int.max())}, of the largest env "
          f"{int(sw_int[big])}; front sweeps max {int(sw_front.max())}, of the largest env {int(sw_front[big])}; vertex "
          f"deviation 0 on all {n} envs in {time.time() - t0:.1f} s")
    assert sw_int[big] > 1
    env.close()
