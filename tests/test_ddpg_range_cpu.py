"""Host only: the exact-arithmetic inputs of tests/ddpg_exact.py, which tests/test_gpu_ddpg_range.py feeds DDPG's gradient kernels
at the sizes of the chunk schedule.  Their precondition and their exactness in three fp32 summation orders at all six sizes;
the rounding counts at those sizes; what the exact check catches that the fp64 bounds of tests/ddpg_grad_ref.py do not (four
mistakes in the batch sum); the restated loss bounds; and the conditions of the default-weight cases of the GPU file."""
import concurrent.futures
import functools

import numpy as np
import pytest
import torch

import ddpg_exact as X
import ddpg_grad_ref as G
import policy_ref as R


@pytest.fixture(scope="module")
def rows():
    return R.input_rows()


@functools.lru_cache(maxsize=2)
def _case(B):
    """The exact case at B rows with both float64 evaluations and the precondition asserted."""
    case = X.build(B)
    ce = X.critic_eval(case.critic_model, case.obs, case.actions, case.y)
    ae = X.actor_eval(case.actor_model, case.actor_obs)
    pow2 = B & (B - 1) == 0
    units = [X.assert_exact_precondition(ce, f"critic B={B}", pow2), X.assert_exact_precondition(ae, f"actor B={B}", pow2)]
    return case, ce, ae, pow2, max(units)


def _names(all_names, pow2):
    return [k for k in all_names if pow2 or not k.endswith("_loss")]


# ----------------------------------------------------------------------------------------------------------- 1. the schedule
def test_schedule_and_rounding_counts_at_the_tables_sizes():
    assert [G.reduction_roundings(B) for B in X.SIZES] == [127, 132, 149, 332, 1087, 1087]
    for B, row in X.SCHEDULE.items():
        tiles, T, chunks, last, tail = row
        assert X.schedule(B) == row and G.reduction_roundings(B) == min(16 * T, 16 * tiles) + chunks - 1
        assert (chunks - 1) * T + last == tiles and 16 * (tiles - 1) + tail == B and 1 <= last <= T and chunks <= G.MAX_CHUNKS
    # what the sizes reach: the cap of 64 chunks (twice ragged below it), T = 4, 5, 6, 17 and 64, short last chunks, the row limit
    assert {r[1] for r in X.SCHEDULE.values()} == {4, 5, 6, 17, 64} and [r[2] for r in X.SCHEDULE.values()] == [64, 53, 54, 61, 64, 64]
    assert [r[3] for r in X.SCHEDULE.values()] == [4, 1, 3, 5, 64, 64] and max(X.SIZES) == G.MAX_ROWS
    assert max(G.GPU_BS) == 4101 and X.schedule(4101)[1:4] == (5, 52, 2)                # what was tested before


def test_the_inputs_are_what_the_docstring_says():
    case = X.build(4168)
    _, Lc = G.live_layers(case.critic_model)
    LA, Lf = G.live_layers(case.actor_model)
    (w1, b1), (w2, b2), (wo, bo) = Lc
    assert w1.shape == (400, 21) and (np.count_nonzero(w1, axis=1) == 2).all() and set(np.unique(w1)) == {-1.0, 0.0, 1.0}
    assert w2.shape == (300, 400) and (np.count_nonzero(w2, axis=1) == 3).all() and set(np.unique(w2)) == {-1.0, 0.0, 1.0}
    assert set(np.unique(b1)) == set(np.unique(b2)) == {-1.0, 0.0, 1.0} and set(np.unique(wo)) == {-1.0, 1.0} and bo[0] == 0
    assert all(set(np.unique(v)) == {-1.0, 0.0, 1.0} for v in (case.obs, case.actions, case.actor_obs))
    c = X.head_scale(4168)
    assert c == 4168 / 8192 and np.count_nonzero(Lf[2][0]) == 64 and set(np.unique(np.abs(Lf[2][0]))) == {0.0, c}
    assert all(np.array_equal(a, b) for la, lb in zip(Lc[:2], Lf[:2]) for a, b in zip(la, lb))
    (a1, ab1), (a2, ab2), (a3, ab3) = LA
    assert np.array_equal(case.actor_obs[:, 9:], case.actor_obs[:, :9])
    assert not a1[:200, 9:].any() and not a1[200:, :9].any() and np.array_equal(a1[200:, 9:], a1[:200, :9]) and np.array_equal(ab1[200:], ab1[:200])
    assert not a2[:150, 200:].any() and not a2[150:, :200].any() and np.array_equal(a2[150:, 200:], a2[:150, :200]) and np.array_equal(ab2[150:], ab2[:150])
    assert np.array_equal(a3[:, 150:], -a3[:, :150]) and set(np.unique(a3)) == {-1.0, 0.0, 1.0} and not ab3.any()
    # the targets: s in -2..2, nonzero where a lost row, tile or chunk would otherwise go unseen
    _, T, chunks, _, _ = X.schedule(4168)
    assert set(np.unique(case.s)) == {-2.0, -1.0, 0.0, 1.0, 2.0} and (case.s[case.forced] != 0).all()
    assert {0, 4167, 80 * (chunks - 1), 79, 80} <= set(case.forced) and 16 * T == 80
    # the live and the target networks alike (the forward kernels read the targets)
    for live, tgt in ((case.actor_model.actor.mu, case.actor_model.actor_target.mu),
                      (case.actor_model.critic.q_networks[0], case.actor_model.critic_target.q_networks[0])):
        assert all(torch.equal(p, q) for p, q in zip(live.parameters(), tgt.parameters()))
    # a smaller batch is a prefix of a larger one
    big = X.build(5128)
    assert np.array_equal(big.obs[:4168], case.obs) and np.array_equal(big.actor_obs[:4168], case.actor_obs)


def test_grid_exponent_and_the_comparison():
    assert X.grid_exponent(np.array([0.0, 6.0, -20.0])) == 1 and X.grid_exponent(np.array([0.75, 8.0])) == -2
    assert X.grid_exponent(np.zeros(3)) is None and X.grid_exponent(np.array([3.0 * 2.0 ** -30, 2.0 ** 40])) == -30
    assert X.first_difference(np.array([-0.0, 1.0], np.float32), np.array([0.0, 1.0])) is None
    assert X.first_difference(np.array([[0.0, 1.0], [np.nan, 2.0]], np.float32), np.array([[0.0, 1.0], [0.0, 2.0]])) == (1, 0)
    assert X.first_difference(np.array([1.0 + 2.0 ** -23], np.float32), np.array([1.0])) == (0,)
    with pytest.raises(AssertionError, match=r"q1\[4167\] \(row 4167: tile 260, chunk 52\)"):
        X.assert_same_numbers({"q1": np.arange(4168.0) + (np.arange(4168) == 4167)}, {"q1": np.arange(4168.0)}, ["q1"], "x", 4168)
    # the precondition refuses a sum that outgrows 24 bits and a value off the fp32 grid
    ones = np.ones((2 ** 12, 1))
    ok = {"sums": {"w1": (4095.0 * ones, ones)}, "chains": []}
    assert X.assert_exact_precondition(ok, "ok", False) == 4095.0 * 2 ** 12
    with pytest.raises(AssertionError, match="reaches 2\\^24"):
        X.assert_exact_precondition({"sums": {"w1": (4097.0 * ones, ones)}, "chains": []}, "big", False)
    with pytest.raises(AssertionError, match="reaches 2\\^24"):          # fine values, one of them on a far finer grid
        X.assert_exact_precondition({"sums": {"w1": (np.array([[1.0], [2.0 ** -24]]), 3.0 * np.ones((2, 1)))}, "chains": []}, "fine", False)
    with pytest.raises(AssertionError, match="not representable"):
        X.assert_exact_precondition(dict(ok, q1=np.array([1.0 + 2.0 ** -30])), "off grid", False)


# ----------------------------------------------------------------------------------------------------------- 2. exactness
@pytest.mark.parametrize("B", X.SIZES)
def test_exact_in_three_fp32_orders(B):
    """The precondition, from the float64 values alone; then float64 autograd of SB3's statements gives the helper's float64
    values, and three float32 evaluations with three orders of the batch sums give them too, as numbers: numpy's pairwise sums
    (ddpg_grad_ref.critic_grad_f32 / actor_grad_f32), torch float32 autograd (the critic statement) and the kernels' own chunk
    order (ddpg_exact.chunk_sums32).  The two losses are part of it where B is a power of two, and lie within ddpg_grad_ref's
    bound elsewhere."""
    case, ce, ae, pow2, units = _case(B)
    cn, an = _names(X.CRITIC_OUT, pow2), _names(X.ACTOR_OUT, pow2)
    assert units < X.LIMIT and float(np.abs(ae["actions_pi"]).max()) == 0.0
    shares = {k: np.count_nonzero(v[k]) / v[k].size for v, names in ((ce, G.CRITIC_GRADS), (ae, G.ACTOR_GRADS)) for k in names}
    assert min(shares.values()) > 0.7, shares                      # the gradients are dense: a misplaced column shows
    # ---- float64 autograd: the helper's evaluations are SB3's statements
    want, acts = G.critic_torch(case.critic_model, case.obs, case.actions, case.y)
    X.assert_same_numbers(want, ce, X.CRITIC_OUT, f"critic autograd B={B}", B)
    assert all(np.array_equal(a, b) for a, b in zip(acts, ce["acts1"]))
    want = G.actor_torch(case.actor_model, case.actor_obs)
    X.assert_same_numbers(want, ae, X.ACTOR_OUT + ("c.w2", "c.b2"), f"actor autograd B={B}", B)
    assert all(np.array_equal(a, b) for k in ("acts", "acts1") for a, b in zip(want[k], ae[k]))
    # ---- fp32, numpy pairwise (by far the longest part at the large sizes: the two statements side by side, numpy's loops
    # run without the interpreter lock)
    with concurrent.futures.ThreadPoolExecutor(2) as pool:
        fc = pool.submit(G.critic_grad_f32, case.critic_model, case.obs, case.actions, case.y)
        fa = pool.submit(G.actor_grad_f32, case.actor_model, case.actor_obs)
        (got, acts), got_actor = fc.result(), fa.result()
    X.assert_same_numbers(got, ce, cn, f"critic pairwise B={B}", B)
    assert all(np.array_equal(a, b) for a, b in zip(acts, ce["acts1"]))
    closs = {"pairwise": got["critic_loss"]}
    got = got_actor
    X.assert_same_numbers(got, ae, an, f"actor pairwise B={B}", B)
    assert all(np.array_equal(a, b) for k in ("acts", "acts1") for a, b in zip(got[k], ae[k]))
    aloss = {"pairwise": got["actor_loss"]}
    # ---- fp32, torch
    got, _ = G.critic_torch(case.critic_model, case.obs, case.actions, case.y, dtype=torch.float32)
    X.assert_same_numbers(got, ce, cn, f"critic torch32 B={B}", B)
    closs["torch32"] = got["critic_loss"]
    # ---- fp32, the kernels' chunk order
    gc = X.gradients_from_sums(ce, "c.", B)[None]
    ga = X.gradients_from_sums(ae, "a.", B)[None]
    assert set(gc) == set(G.CRITIC_GRADS) | {"critic_loss"} and set(ga) == set(G.ACTOR_GRADS) | {"actor_loss"}
    X.assert_same_numbers(gc, ce, _names(gc, pow2), f"critic chunk order B={B}")
    X.assert_same_numbers(ga, ae, _names(ga, pow2), f"actor chunk order B={B}")
    closs["chunks"], aloss["chunks"] = gc["critic_loss"], ga["actor_loss"]
    # ---- the losses where they are not exact: inside ddpg_grad_ref's bound
    if not pow2:
        cb = X.critic_loss_bound(case.critic_model, case.obs, case.actions, case.y)
        ab = X.actor_loss_bound(case.actor_model, case.actor_obs)
        assert cb[0] == ce["critic_loss"] and ab[0] == ae["actor_loss"]
        r = [R.assert_within(np.asarray(v), cb, f"critic_loss {k} B={B}") for k, v in closs.items()]
        r += [R.assert_within(np.asarray(v), ab, f"actor_loss {k} B={B}") for k, v in aloss.items()]
        print(f"\nB={B}: losses |fp32 - fp64| / bound at most {max(r):.4f}")
    print(f"\nB={B}: sum |terms| / grid at most {units:.3g} (2^24 = {X.LIMIT:.3g}); nonzero shares {min(shares.values()):.2f}..{max(shares.values()):.2f}")


def test_the_restated_loss_bounds_are_ddpg_grad_refs():
    """critic_loss_bound / actor_loss_bound against critic_grad / actor_grad themselves, on the exact inputs (a ragged B) and on
    the default weights."""
    rows = R.input_rows()
    case = X.build(4168)
    for m, obs, act, y, mo, ao in ((case.critic_model, case.obs, case.actions, case.y, case.actor_model, case.actor_obs),
                                   (G.model(), *G.batch(100, rows), G.model(), G.batch(100, rows)[0])):
        for ls in G.LOSS_SCALES:
            ref, _ = G.critic_grad(m, obs, act, y, ls)
            got = X.critic_loss_bound(m, obs, act, y, ls)
            assert got[0] == ref["critic_loss"][0] and got[1] == ref["critic_loss"][1] and got[1] > 0
        ref, _ = G.actor_grad(mo, ao)
        got = X.actor_loss_bound(mo, ao)
        assert got[0] == ref["actor_loss"][0] and got[1] == ref["actor_loss"][1] and got[1] > 0


# ----------------------------------------------------------------------------------------------------------- 3. the mutants
def test_the_exact_check_catches_every_lost_or_doubled_piece_at_65528():
    """The batch sum in the kernels' chunk order with the last row, the last row tile or the last chunk left out, or the last
    chunk added twice, on the exact inputs at B = 65528 (T = 64, 64 chunks, eight rows in the last tile): EVERY gradient of both
    statements differs from the float64 value under each of the four.  (Hence s is forced nonzero on the rows at the chunks'
    edges: a row with d = 0 would be lost unseen.)"""
    B = 65528
    case, ce, ae, pow2, _ = _case(B)
    assert not pow2 and case.s[B - 1] != 0
    for ev, prefix, names in ((ce, "c.", G.CRITIC_GRADS), (ae, "a.", G.ACTOR_GRADS)):
        g = X.gradients_from_sums(ev, prefix, B, X.SUM_MUTANTS, losses=False)
        X.assert_same_numbers(g[None], ev, names, f"{prefix} chunk order")
        for mutant in X.SUM_MUTANTS:
            same = [k for k in names if X.first_difference(g[mutant][k], ev[k]) is None]
            assert not same, f"{mutant}: {same} equal the float64 value"
            changed = {k: int((g[mutant][k] != ev[k].reshape(g[mutant][k].shape)).sum()) / ev[k].size for k in names}
            print(f"\n{prefix} {mutant}: share of elements changed " + " ".join(f"{k}={v:.2f}" for k, v in changed.items()))


def test_what_the_fp64_bounds_miss_at_16385(rows):
    """The same four mistakes on torch's default weights at B = 16385 (T = 17, 61 chunks, one row in the last tile), against
    ddpg_grad_ref's bounds: the unmutated chunk-order sum is inside every bound, and which mistakes push a gradient outside is
    printed, not asserted, because nothing promises it.  Measured (the outputs with an element outside its bound):

                           critic statement                 actor statement
        drop_last_row      c.w1, c.b1                       none
        drop_last_tile     c.w1, c.b1 (the same one row)    none
        drop_last_chunk    all six                          all but a.w0
        last_chunk_twice   all six                          all but a.w0

    NOT caught: a lost last row (or tile) in c.w0, c.b0, c.w2, c.b2 and in every gradient of the actor statement, and a lost or
    doubled chunk of 80 rows in a.w0.  Where the lost row is seen, it is in elements of neurons that few rows activate, whose
    sum |terms| is small; an element every row feeds has one row at 6.1e-5 of sum |terms| under a bound of gamma_332 = 2.0e-5
    of it plus the terms' own errors.  At 65 536 rows gamma_1087 = 6.5e-5 against one row's 1.5e-5.  That is why the large sizes
    are checked on the exact inputs.  Also here: the ambiguous shares of the reference alone stay under their caps at 4161 and
    16385 rows with the observations made distinct (critic statement 1.7e-5 and 1.6e-5; the actor statement's actor 1.4e-5 and
    2.5e-5, its critic 1.3e-4 and 1.4e-4)."""
    m = G.model()
    for B in (4161, 16385):
        obs, act, y = X.distinct_batch(B, rows)
        cref, cinfo = G.critic_grad(m, obs, act, y)
        aref, ainfo = G.actor_grad(m, obs)
        G.assert_critic_conditions(cinfo, f"critic B={B}")
        G.assert_actor_conditions(ainfo, f"actor B={B}")
        print(f"\nB={B}: ambiguous shares: critic statement {cinfo['share']:.1e}; actor statement: actor {ainfo['actor_share']:.1e} critic {ainfo['critic_share']:.1e}")
    assert X.schedule(B)[1:] == (17, 61, 5, 1)
    for ev, ref, prefix, names in ((X.critic_eval(m, obs, act, y), cref, "c.", G.CRITIC_GRADS), (X.actor_eval(m, obs), aref, "a.", G.ACTOR_GRADS)):
        for k in names:                                                           # the two float64 evaluations agree
            assert np.allclose(ev[k].reshape(ref[k][0].shape), ref[k][0], rtol=1e-9, atol=1e-30), k
        g = X.gradients_from_sums(ev, prefix, B, X.SUM_MUTANTS, losses=False)
        assert G.outside(g[None], {k: ref[k] for k in names}) == []
        caught = {mutant: G.outside(g[mutant], {k: ref[k] for k in names}) for mutant in X.SUM_MUTANTS}
        print(f"\n{prefix} B={B}: outputs outside ddpg_grad_ref's bounds: {caught}")
