"""GPU: the domain pipeline on the device (BASELINE.json configs[4]): meshenv_create_random generates,
orients, densifies and rounds one GenerateRandomPolygon-style ring per env from random.Random(seed + k) and computes
its constants in HIP kernels.  Bar: the rings are BIT-IDENTICAL to the host restatement domains.random_domain(seed + k)
(whose generator is pinned against the reference by tests/test_domains_cpu.py) for 8192 seeds; constants within 1e-12
relative of the host's (BLAS dot / pow(x, 2) order effects); envs created this way step like envs created from the same
rings through meshenv_create.  The last section varies what the tests above keep fixed: density, fixed vertex counts in
density mode, num_verts 5..7, an edge longer than every polygon edge, the constants of every short ring, and the refusal of
seeds whose polygon the host regenerates."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_device_rings_equal_host_restatement_8192_seeds():
    from reinforcementlearning4meshgeneration_amd import MeshVecEnv
    from reinforcementlearning4meshgeneration_amd.domains import domain_constants, random_domain
    n, seed = 8192, 50_000
    env = MeshVecEnv.from_random(n, seed)
    sizes = []
    worst = 0.0
    for k in range(n):
        ring, consts = env.get_domain(k)
        host = random_domain(seed + k)
        assert ring.shape == (len(host), 2), (k, ring.shape, len(host))
        assert np.array_equal(ring, np.asarray(host, np.float64)), k          # bit for bit
        sizes.append(len(host))
        if k % 16 == 0:
            c = domain_constants(host)
            ref = np.array([c.original_area, c.est_min_l ** 2, c.est_crit_l ** 2])
            rel = np.abs(np.array(consts) - ref) / ref
            worst = max(worst, float(rel.max()))
            assert rel.max() <= 1e-12, (k, consts, ref)
    sizes = np.array(sizes)
    print(f"device-generated rings: {n} identical to the host's, sizes {sizes.min()}..{sizes.max()} "
          f"(mean {sizes.mean():.1f}), constants within {worst:.2e}")
    assert len(np.unique(sizes)) > 20 and (sizes % 2 == 0).all()
    assert env.max_ring == sizes.max()
    env.close()


@pytest.mark.parametrize("num_verts,seed", [(16, 7), (8, 2 ** 33 + 5), (64, 123456789)])
def test_fixed_vertex_count_and_wide_seeds(num_verts, seed):
    """numVerts fixed (the reference's own call uses 16) and seeds beyond 32 bits (two key words in init_by_array)."""
    from reinforcementlearning4meshgeneration_amd import MeshVecEnv
    from reinforcementlearning4meshgeneration_amd.domains import random_domain
    env = MeshVecEnv.from_random(64, seed, num_verts=num_verts, edge=0.3)
    for k in range(64):
        ring, _ = env.get_domain(k)
        host = random_domain(seed + k, num_verts=num_verts, edge=0.3)
        assert np.array_equal(ring, np.asarray(host, np.float64)), k
    env.close()


def test_generated_envs_step_like_host_built_envs():
    """Same rings through meshenv_create (host arrays) and meshenv_create_random (device): identical trajectories, and
    both in lockstep with the oracle."""
    import torch
    from oracle.ref_lib import RefBatch, RefEnv
    from reinforcementlearning4meshgeneration_amd import MeshVecEnv
    from reinforcementlearning4meshgeneration_amd.domains import random_domain
    n, seed, T = 1024, 900, 48
    dev_env = MeshVecEnv.from_random(n, seed)
    doms = [random_domain(seed + k) for k in range(n)]
    host_env = MeshVecEnv(doms, env_domain=np.arange(n, dtype=np.int32))
    refs = [RefEnv.from_points(d, cap_new=64) for d in doms]
    batch = RefBatch(refs)
    assert torch.equal(dev_env.reset(), host_env.reset())
    assert np.array_equal(dev_env.obs.cpu().numpy(), batch.reset())
    rng = np.random.default_rng(3)
    a = rng.uniform([-1, -1.5, 0], [1, 1.5, 1.5], size=(T, n, 3))
    pick = rng.random((T, n)) < 0.5
    b = np.stack([rng.uniform(-1, 1, (T, n)), rng.uniform(0.2, 1.0, (T, n)), rng.uniform(0.3, 1.2, (T, n))], axis=2)
    a[pick] = b[pick]
    a = a.astype(np.float32)
    acts = torch.from_numpy(a).cuda()
    for t in range(T):
        o1, r1, d1, c1 = dev_env.step(acts[t])
        o2, r2, d2, c2 = host_env.step(acts[t])
        o_ref, r_ref, d_ref, c_ref = batch.step(a[t], auto_reset=True, threads=8)
        assert torch.equal(o1, o2) and torch.equal(d1, d2) and torch.equal(c1, c2), t
        # the reward's speed term uses the area range, which the device computes with x * x where the host uses pow(x, 2)
        assert float((r1 - r2).abs().max()) <= 1e-12, t
        assert np.abs(o1.cpu().numpy().astype(np.float64) - o_ref).max() <= 1e-5 and np.array_equal(d1.cpu().numpy(), d_ref)
        assert np.abs(r1.cpu().numpy() - r_ref).max() <= 1e-5
    assert dev_env.counters()["valid"] == host_env.counters()["valid"] > 0
    dev_env.close(); host_env.close()


def test_config5_full_size_65536_generated_envs_sampled_oracle_shadow():
    """BASELINE.json configs[4] at its FULL size on one GPU (65 536 envs, each on its own device-generated ring): 40 steps,
    with 1 024 evenly spaced envs shadowed by the oracle on the same actions (flags exact, obs / reward within 1e-5, rings
    of 64 of them bit-exact at the end), plus the size-independent bookkeeping identity on every env."""
    import torch
    from oracle.ref_lib import RefBatch, RefEnv
    from reinforcementlearning4meshgeneration_amd import MeshVecEnv
    n, seed, T, S = 65536, 2_000_000, 40, 1024
    env = MeshVecEnv.from_random(n, seed)
    pick = np.arange(0, n, n // S)
    refs = []
    for k in pick:
        ring, _ = env.get_domain(int(k))
        refs.append(RefEnv.from_points([tuple(p) for p in ring], cap_new=64))
    batch = RefBatch(refs)
    obs0 = env.reset()
    assert np.array_equal(obs0[pick].cpu().numpy(), batch.reset())
    g = torch.Generator(device="cuda"); g.manual_seed(17)
    lo = torch.tensor([-1.0, -1.5, 0.0], device="cuda"); hi = torch.tensor([1.0, 1.5, 1.5], device="cuda")
    blo = torch.tensor([-1.0, 0.2, 0.3], device="cuda"); bhi = torch.tensor([1.0, 1.0, 1.2], device="cuda")
    idx = torch.from_numpy(pick).cuda()
    for t in range(T):
        u = torch.rand((n, 3), device="cuda", generator=g)
        a = torch.where(torch.rand((n, 1), device="cuda", generator=g) < 0.5, blo + (bhi - blo) * u, lo + (hi - lo) * u).contiguous()
        o, r, d, c = env.step(a)
        o_ref, r_ref, d_ref, c_ref = batch.step(a[idx].cpu().numpy(), auto_reset=True, threads=16)
        assert np.abs(o[idx].cpu().numpy().astype(np.float64) - o_ref).max() <= 1e-5, t
        assert np.abs(r[idx].cpu().numpy() - r_ref).max() <= 1e-5, t
        assert np.array_equal(d[idx].cpu().numpy(), d_ref) and np.array_equal(c[idx].cpu().numpy(), c_ref), t
    for j in range(0, S, 16):
        st = env.get_state(int(pick[j]))
        ids, xy = refs[j].ring()
        assert np.array_equal(st["ring_ids"], ids) and np.array_equal(st["ring_xy"], xy)
    cnt = env.counters()
    assert cnt["steps"] == n * T and cnt["valid"] > 0.005 * n * T
    print(f"config 5 at full size: {n} envs x {T} steps, {cnt['valid']} valid extractions, max ring {env.max_ring}")
    env.close()


# ------------------------------------------------------------------------------------------------ the reference's densifier
def _fx():
    import json
    import os
    from conftest import GOLDEN_DIR
    return json.load(open(os.path.join(GOLDEN_DIR, "domain_pipeline.json")))


def test_device_calculate_density_equals_the_reference_vectors():
    """Density.calculate_density (ui/tk-ui.py:252-276) + clockwise rule + / 100 on the device (meshenv_density_rings) against
    the vectors recorded from the reference's own function (tests/golden/domain_pipeline.json: 8 calculate_density cases
    with per-vertex densities, 7 whole-pipeline cases): bit for bit, ZeroDivisionError cases reported as status 1."""
    from reinforcementlearning4meshgeneration_amd import domains as D
    fx = _fx()
    polys, dens, bl, want = [], [], [], []
    for case in fx["calculate_density"]:
        polys.append([tuple(p) for p in case["points"]]); dens.append(case["densities"]); bl.append(case["base_length"])
        want.append(None if case["result"] is None else
                    [(p[0] / 100, p[1] / 100) for p in D.normalise_clockwise([tuple(p) for p in case["result"]])])
    for case in fx["pipeline"]:
        polys.append([tuple(p) for p in case["raw"]]); dens.append([1.0] * len(case["raw"])); bl.append(case["base_length"])
        want.append(None if case["ring"] is None else [tuple(p) for p in case["ring"]])
    n_ok = n_raise = 0
    for k in range(len(polys)):                       # one call per case: base_length differs
        rings, st = D.device_density_rings([polys[k]], bl[k], [dens[k]])
        if want[k] is None:
            assert st[0] == 1 and rings[0] is None, (k, st)
            n_raise += 1
        else:
            assert st[0] == 0, (k, st)
            assert rings[0].shape == (len(want[k]), 2) and np.array_equal(rings[0], np.asarray(want[k], np.float64)), k
            n_ok += 1
    assert n_ok >= 8 and n_raise >= 2


def test_device_density_mode_equals_host_restatement_on_generated_polygons():
    """meshenv_create_random_density: generator + calculate_density + orientation on the device for a block of 49 152 + 16 384 seeds
    at two spacings; the raise flags equal the host restatement's ZeroDivisionError seed by seed, and the rings of the
    envs built from the defined seeds are domains.random_density_domain(seed, base_length) bit for bit."""
    import ctypes as C
    import torch
    from reinforcementlearning4meshgeneration_amd import MeshVecEnv, _capi
    from reinforcementlearning4meshgeneration_amd.domains import random_density_domain
    L = _capi.load()
    total_defined = 0
    for base_length, seed0, blk in ((20.0, 300_000, 49152), (12.0, 900_000, 16384)):
        rz = np.zeros(blk, np.uint8)
        rc = L.meshenv_create_random_density(0, blk, C.c_uint64(seed0), None, 0, base_length, 1.0, None, None, None, rz.ctypes.data)
        assert rc in (0, _capi.E_STATE)
        host_raises = np.zeros(blk, np.uint8)
        host_rings = {}
        for k in range(blk):
            try:
                host_rings[k] = random_density_domain(seed0 + k, base_length)
            except ZeroDivisionError:
                host_raises[k] = 1
        ok = rz != 2      # 2: a polygon of fewer than 5 distinct pixels, which the device does not regenerate (a handful per 10^5)
        assert ok.mean() > 0.999 and np.array_equal(rz[ok], host_raises[ok]), np.nonzero(rz != host_raises)[0][:8]
        defined = np.nonzero(rz == 0)[0]
        assert len(defined) > 50
        env = MeshVecEnv.from_random_density(len(defined), 0, base_length=base_length, seeds=seed0 + defined)
        for j, k in enumerate(defined):
            ring, _ = env.get_domain(j)
            host = np.asarray(host_rings[int(k)], np.float64)
            assert ring.shape == host.shape and np.array_equal(ring, host), (base_length, int(k))
            assert len(host) % 2 == 0
        total_defined += len(defined)
        env.close()
    print("density mode: rings identical to the host restatement on", total_defined, "generated polygons")
    assert total_defined >= 8192
    # and the seed search of the Python wrapper
    env = MeshVecEnv.from_random_density(512, 300_000, base_length=20.0)
    assert len(env.seeds) == 512 and (np.diff(env.seeds.astype(np.int64)) > 0).all()
    ring, _ = env.get_domain(5)
    assert np.array_equal(ring, np.asarray(random_density_domain(int(env.seeds[5]), 20.0), np.float64))
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    lo = torch.tensor([-1.0, 0.2, 0.3], device="cuda"); hi = torch.tensor([1.0, 1.0, 1.2], device="cuda")
    valid0 = env.counters()["valid"]
    for _ in range(40):
        env.step((lo + (hi - lo) * torch.rand((512, 3), device="cuda", generator=g)).contiguous())
    assert env.counters()["valid"] - valid0 > 200       # the rings are meshable domains
    env.close()


def test_density_rings_extreme_spacings_are_reported_not_written():
    """meshenv_density_rings accepts pixel coordinates up to 1e9 and any base_length > 0: an edge whose point count exceeds a
    whole ring (or the int range) must come back as status 2, never as a write past the 2048-point staging array."""
    from reinforcementlearning4meshgeneration_amd import domains as D
    far = [(0, 0), (900_000_000, 0), (900_000_000, 900_000_000), (0, 900_000_000)]
    rings, st = D.device_density_rings([far, far, [(0, 0), (400, 0), (400, 400), (0, 400)]], 1e-6)
    assert list(st) == [2, 2, 2] and all(r is None for r in rings)
    rings, st = D.device_density_rings([far, [(0, 0), (400, 0), (400, 400), (0, 400)]], 20.0)
    assert st[0] == 2 and st[1] == 0 and rings[1].shape[0] == 80       # the neighbour of a refused ring is still produced


def test_random_density_probe_skips_seeds_the_device_cannot_generate():
    """from_random_density at a spacing where some generated polygons densify beyond 2048 points: those seeds are flagged per
    ring (2) and left out by the probe; the envs are built from the others; naming a flagged seed explicitly is an error
    that lists it."""
    import ctypes as C
    from reinforcementlearning4meshgeneration_amd import MeshVecEnv, _capi
    L = _capi.load()
    base_length, seed0, blk = 0.6, 40_000, 512
    rz = np.zeros(blk, np.uint8)
    rc = L.meshenv_create_random_density(0, blk, C.c_uint64(seed0), None, 0, base_length, 1.0, None, None, None, rz.ctypes.data)
    assert rc == _capi.E_STATE and (rz == 2).any() and (rz == 0).any(), np.bincount(rz, minlength=3)
    env = MeshVecEnv.from_random_density(64, seed0, base_length=base_length)
    flagged = set((seed0 + np.nonzero(rz != 0)[0]).tolist())
    assert len(env.seeds) == 64 and not (set(env.seeds.tolist()) & flagged)
    assert env.max_ring <= 2048 and env.get_domain(0)[0].shape[0] >= 4
    env.close()
    bad = seed0 + int(np.nonzero(rz == 2)[0][0])
    with pytest.raises(_capi.MeshEnvError, match=str(bad)):
        MeshVecEnv.from_random_density(2, 0, base_length=base_length, seeds=[int(env.seeds[0]), bad])


# ------------------------------------------------------------------------------------------------ beyond the recorded parameters
def _regenerates(seed, num_verts=None):
    """True where domains.random_polygon_px draws a second polygon from the stream of ``seed`` (fewer than 5 distinct pixels
    in the first): the device does not restate that and must refuse the seed."""
    import random
    from reinforcementlearning4meshgeneration_amd.domains import generate_polygon
    rng = random.Random(seed)
    nv = num_verts if num_verts is not None else rng.randint(8, 64)
    pts = []
    for p in generate_polygon(num_verts=nv, rng=rng):
        if not pts or p != pts[-1]:
            pts.append(p)
    if len(pts) > 1 and pts[0] == pts[-1]:
        pts.pop()
    return len(pts) < 5


def _assert_rings_and_constants(env, hosts):
    """Every ring bit for bit, and the constants of EVERY ring within 1e-12 relative of domains.domain_constants (the bar
    and its reason: test_device_rings_equal_host_restatement_8192_seeds)."""
    from reinforcementlearning4meshgeneration_amd.domains import domain_constants
    worst = 0.0
    for k, host in enumerate(hosts):
        ring, consts = env.get_domain(k)
        want = np.asarray(host, np.float64)
        assert ring.shape == want.shape and np.array_equal(ring, want), k
        c = domain_constants(host)
        ref = np.array([c.original_area, c.est_min_l ** 2, c.est_crit_l ** 2])
        rel = np.abs(np.array(consts) - ref) / ref
        worst = max(worst, float(rel.max()))
        assert rel.max() <= 1e-12, (k, consts, ref)
    return worst


@pytest.mark.parametrize("num_verts,seed", [(5, 548), (6, 100), (7, 100)])
@pytest.mark.parametrize("edge", [0.45, 10.0])
def test_uniform_mode_at_the_smallest_vertex_counts(num_verts, seed, edge):
    """num_verts 5, 6 and 7 (the least the C-ABI accepts), 64 consecutive seeds none of which regenerates; at edge 10.0 every
    edge is one piece, the rings have 5 to 8 unequal edges, and which sorted edge srt[1] / srt[n - 2] is decides the constants."""
    from reinforcementlearning4meshgeneration_amd import MeshVecEnv
    from reinforcementlearning4meshgeneration_amd.domains import random_domain
    assert not any(_regenerates(seed + k, num_verts) for k in range(64))
    hosts = [random_domain(seed + k, num_verts=num_verts, edge=edge) for k in range(64)]
    if edge == 10.0:
        assert max(map(len, hosts)) == num_verts + num_verts % 2          # one piece per edge, one more on an odd count
    env = MeshVecEnv.from_random(64, seed, num_verts=num_verts, edge=edge)
    worst = _assert_rings_and_constants(env, hosts)
    print(f"num_verts {num_verts}, edge {edge}: 64 rings of {min(map(len, hosts))}..{max(map(len, hosts))} points, constants within {worst:.2e}")
    env.close()


def test_uniform_mode_one_piece_per_edge_bumped_and_unbumped():
    """edge = 10.0 with the vertex count drawn per stream: every edge is one piece, so the even-count bump on the last lane
    alone decides the ring length -- polygons of an odd count get one more point, those of an even count none."""
    from reinforcementlearning4meshgeneration_amd import MeshVecEnv
    from reinforcementlearning4meshgeneration_amd.domains import random_domain, random_polygon_px
    n, seed = 256, 4000
    assert not any(_regenerates(seed + k) for k in range(n))
    raw = [len(random_polygon_px(seed + k)) for k in range(n)]
    hosts = [random_domain(seed + k, edge=10.0) for k in range(n)]
    assert all(len(h) == r + r % 2 for h, r in zip(hosts, raw))
    bumped = sum(r % 2 for r in raw)
    assert bumped >= 64 and n - bumped >= 64 and min(raw) <= 10 and max(raw) >= 60
    env = MeshVecEnv.from_random(n, seed, edge=10.0)
    worst = _assert_rings_and_constants(env, hosts)
    assert env.max_ring == max(map(len, hosts))
    print(f"edge 10.0: {n} rings of {min(raw)}..{max(raw)} edges, {bumped} bumped, constants within {worst:.2e}")
    env.close()


@pytest.mark.parametrize("num_verts,bad", [(5, 67), (5, 69), (5, 72), (6, 30), (7, 7758), (8, 2767)])
def test_uniform_mode_refuses_a_seed_whose_polygon_regenerates(num_verts, bad):
    """random_polygon_px draws a second polygon from the same stream on these seeds (found on the host); the device does
    not restate that, so a batch containing one must fail loudly and return no environment -- never some other ring.  The
    same call one seed later succeeds and equals the host, unless the host says another such seed is among its four."""
    from reinforcementlearning4meshgeneration_amd import MeshVecEnv, _capi
    from reinforcementlearning4meshgeneration_amd.domains import random_domain
    assert _regenerates(bad, num_verts)
    for start in (bad, bad - 3):                      # the bad seed first and last among the four
        with pytest.raises(_capi.MeshEnvError, match="could not be generated"):
            MeshVecEnv.from_random(4, start, num_verts=num_verts)
    nxt = bad + 1
    if any(_regenerates(nxt + k, num_verts) for k in range(4)):
        assert (num_verts, bad) in ((5, 67), (5, 69))         # 69 and 72 follow within four seeds
        with pytest.raises(_capi.MeshEnvError, match="could not be generated"):
            MeshVecEnv.from_random(4, nxt, num_verts=num_verts)
        return
    env = MeshVecEnv.from_random(4, nxt, num_verts=num_verts)
    _assert_rings_and_constants(env, [random_domain(nxt + k, num_verts=num_verts) for k in range(4)])
    env.close()


@pytest.mark.parametrize("density,base_length,num_verts", [(0.5, 12.6, 0), (1.5, 4.1, 0), (0.5, 40.2, 5), (1.5, 13.4, 5),
                                                           (0.5, 6.6, 64), (1.5, 2.2, 64)])
def test_density_mode_at_other_densities_and_fixed_vertex_counts(density, base_length, num_verts):
    """GenParams::density and fixed_verts together with density_mode: a block of 512 seeds at density 0.5 and 1.5, with
    the vertex count drawn per stream, 5 and 64.  The base lengths were chosen on the host so that calculate_density is
    defined on at least 64 seeds of the block and raises on others.  Raise flags equal the host's seed by seed wherever
    the device generated the polygon (flag != 2); flag 2 only where the host regenerates or its ring exceeds 2048 points;
    the rings of the defined seeds bit for bit."""
    import ctypes as C
    from reinforcementlearning4meshgeneration_amd import MeshVecEnv, _capi
    from reinforcementlearning4meshgeneration_amd.domains import random_density_domain
    L = _capi.load()
    seed0, blk = 700_000, 512
    nv = num_verts or None
    host_flags = np.zeros(blk, np.uint8)
    host_rings = {}
    for k in range(blk):
        try:
            host_rings[k] = random_density_domain(seed0 + k, base_length, density, nv)
        except ZeroDivisionError:
            host_flags[k] = 1
    usable = [k for k, r in host_rings.items() if len(r) <= 2048 and not _regenerates(seed0 + k, nv)]
    assert len(usable) >= 64 and host_flags.sum() >= 3, (len(usable), int(host_flags.sum()))
    rz = np.zeros(blk, np.uint8)
    rc = L.meshenv_create_random_density(0, blk, C.c_uint64(seed0), None, num_verts, base_length, density, None, None, None, rz.ctypes.data)
    assert rc in (0, _capi.E_STATE)
    ok = rz != 2
    assert np.array_equal(rz[ok], host_flags[ok]), (np.nonzero(ok & (rz != host_flags))[0][:8], rz[ok].sum(), host_flags[ok].sum())
    for k in np.nonzero(~ok)[0]:
        assert _regenerates(seed0 + int(k), nv) or (int(k) in host_rings and len(host_rings[int(k)]) > 2048), int(k)
    defined = np.nonzero(rz == 0)[0]
    assert set(defined.tolist()) == set(usable)
    env = MeshVecEnv.from_random_density(len(defined), 0, base_length=base_length, density=density, num_verts=num_verts,
                                         seeds=seed0 + defined)
    for j, k in enumerate(defined):
        ring, _ = env.get_domain(j)
        host = np.asarray(host_rings[int(k)], np.float64)
        assert ring.shape == host.shape and np.array_equal(ring, host), (int(k), ring.shape, host.shape)
        assert len(host) % 2 == 0
    print(f"density {density}, base_length {base_length}, num_verts {num_verts}: {len(defined)} rings identical, "
          f"{int(host_flags.sum())} raise, {int((~ok).sum())} not generated")
    env.close()
