"""CPU: the fp64 references of tests/policy_ref.py have teeth.

* The host Philox4x32-10 reproduces the Random123 known-answer vectors.
* The per-element bound is not too tight: fp32 forwards summed in other orders (torch CPU; numpy with a sequential
  k-sum) stay inside it on every element, for the 12 policy instantiations and the SAC actor.
* The bound is tight enough: each deliberate kernel mistake, applied to the fp64 forward on the inputs the GPU tests use,
  leaves it on at least one element."""
import numpy as np
import pytest

import policy_ref as R

SEQ_ROWS = 1500            # rows of the (slow) numpy sequential-sum forward


@pytest.fixture(scope="module")
def rows():
    x = R.input_rows()
    return x, R.noise_rows(len(x))


# ------------------------------------------------------------------------------------------------------------ Philox
@pytest.mark.parametrize("ctr, key, want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, want):
    got = R.philox4x32(*[np.array([c], np.uint64) for c in ctr], *key)
    assert tuple(int(w[0]) for w in got) == want


def test_philox_normal_fp32_inside_bound_and_mutants_outside():
    seed, counter = (7 << 32) | 12345, (3 << 32) | 99
    env = np.arange(65536 - 20000, 65536 + 20000, dtype=np.uint64)
    ref = R.philox_normal(seed, counter, env)
    f32 = R.philox_normal_f32(seed, counter, env)
    r = R.assert_within(f32, ref, "fp32 Box-Muller")
    print(f"philox eps: fp32 restatement max |err| / bound = {r:.3f}, max bound {ref[1].max():.2e}")
    assert ref[1].max() < 1e-5 and np.abs(ref[0]).max() > 4
    for m in ("drop_counter_hi", "swap_env_counter", "comp2_words01"):
        mut = R.philox_normal(seed, counter, env, mutant=m)[0]
        assert R.ratio(mut, ref)[1].any(), m


# ------------------------------------------------------------------------------------------------------------ fp32 forwards
def _torch_policy(case, m, obs, eps):
    import torch
    kind, H, act = case
    f = torch.relu if act == "relu" else torch.tanh
    low, high = torch.from_numpy(R.ACTION_LOW), torch.from_numpy(R.ACTION_HIGH)
    obs, eps = torch.from_numpy(obs), torch.from_numpy(eps)
    with torch.no_grad():
        h = f(m["pi"][1](f(m["pi"][0](obs))))
        if kind == "actor_critic":
            mean = m["action_net"](h)
            std = m["log_std"].exp().expand_as(mean)
            ba = mean + std * eps
            lp = torch.distributions.Normal(mean, std).log_prob(ba).sum(-1)
            v = m["value_net"](f(m["vf"][1](f(m["vf"][0](obs)))))[:, 0]
            out = dict(actions=torch.clamp(ba, low, high), buffer_actions=ba, log_prob=lp, value=v)
        else:
            s = torch.clamp(torch.tanh(m["mu"](h)) + m["sigma"] * eps, -1, 1)
            out = dict(actions=low + 0.5 * (s + 1) * (high - low), buffer_actions=s)
    return {k: v.numpy() for k, v in out.items()}


def _seq_linear(x, W, b, act=None):
    """fp32 y = act(sum_k W[:, k] x[:, k] + b), products rounded and summed one k at a time."""
    acc = np.zeros((x.shape[0], W.shape[0]), np.float32)
    for k in range(W.shape[1]):
        acc = acc + x[:, k:k + 1] * W[None, :, k]
    acc = acc + b
    return np.maximum(acc, np.float32(0)) if act == "relu" else np.tanh(acc) if act == "tanh" else acc


def _seq_policy(case, spec, obs, eps):
    L = R.spec_weights(spec)
    act = spec.activation
    low, high = R.ACTION_LOW, R.ACTION_HIGH

    def tw(layers):
        (w1, b1), (w2, b2), (wh, bh) = layers
        return _seq_linear(_seq_linear(_seq_linear(obs, w1, b1, act), w2, b2, act), wh, bh)
    mean = tw(L["pi"])
    if case[0] == "actor_critic":
        std = np.exp(spec.weights["log_std_or_sigma"])
        ba = mean + std * eps
        d = ba - mean
        lpc = -(d * d) / (np.float32(2) * (std * std)) - np.log(std) - np.float32(R.LOG_SQRT_2PI)
        return dict(actions=np.clip(ba, low, high), buffer_actions=ba, log_prob=(lpc[:, 0] + lpc[:, 1]) + lpc[:, 2],
                    value=tw(L["vf"])[:, 0])
    s = np.clip(np.tanh(mean) + spec.weights["log_std_or_sigma"] * eps, np.float32(-1), np.float32(1))
    return dict(actions=low + np.float32(0.5) * (s + np.float32(1)) * (high - low), buffer_actions=s)


@pytest.mark.parametrize("head_scale", [1.0, 6.0])
@pytest.mark.parametrize("case", R.POLICY_CASES, ids=R.case_id)
def test_policy_bound_admits_other_fp32_orders(case, head_scale, rows):
    obs, eps = rows
    m = R.policy_modules(case, head_scale=head_scale)
    spec = R.policy_spec(case, m)
    worst = {}
    for name, fwd, x, e in (("torch", _torch_policy(case, m, obs, eps), obs, eps),
                            ("sequential", _seq_policy(case, spec, obs[:SEQ_ROWS], eps[:SEQ_ROWS]), obs[:SEQ_ROWS], eps[:SEQ_ROWS])):
        ref = R.policy_forward(spec, x, e, ba_kernel=fwd["buffer_actions"])
        assert set(fwd) <= set(ref)
        for k, v in fwd.items():
            worst[(name, k)] = R.assert_within(v, ref[k], f"{name} {k}")
        R.check_clamps(fwd, ref)
    print(R.case_id(case), head_scale, {f"{a}/{b}": round(v, 4) for (a, b), v in worst.items()})


def test_actor_bound_admits_other_fp32_orders(rows):
    import torch
    obs, eps = rows
    lin, mu, ls = R.actor_modules()
    low, high = torch.from_numpy(R.ACTION_LOW), torch.from_numpy(R.ACTION_HIGH)
    with torch.no_grad():
        h = torch.from_numpy(obs)
        for layer in lin:
            h = torch.relu(layer(h))
        m_, s_ = mu(h), ls(h).clamp(-20, 2).exp()
        for e in (None, eps):
            z = m_ if e is None else m_ + s_ * torch.from_numpy(e)
            a = (low + 0.5 * (torch.tanh(z) + 1) * (high - low)).numpy()
            r = R.assert_within(a, R.actor_forward(lin, mu, ls, obs, e)["actions"], "torch actor")
            print("sac actor torch fp32: max |err| / bound", round(r, 4))
    w = [(R._np32(x.weight), R._np32(x.bias)) for x in lin]
    x = obs[:SEQ_ROWS]
    h = x
    for W, b in w:
        h = _seq_linear(h, W, b, "relu")
    heads = _seq_linear(h, np.concatenate([R._np32(mu.weight), R._np32(ls.weight)]), np.concatenate([R._np32(mu.bias), R._np32(ls.bias)]))
    z = heads[:, :3] + np.exp(np.clip(heads[:, 3:], np.float32(-20), np.float32(2))) * eps[:SEQ_ROWS]
    a = R.ACTION_LOW + np.float32(0.5) * (np.tanh(z) + np.float32(1)) * (R.ACTION_HIGH - R.ACTION_LOW)
    R.assert_within(a, R.actor_forward(lin, mu, ls, x, eps[:SEQ_ROWS])["actions"], "sequential actor")


# ------------------------------------------------------------------------------------------------------------ mutants
FORWARD_MUTANTS = ("swap_in_16_17", "drop_in_17", "swap_k_layer2", "bias_next_neuron", "tf32", "shift_last_row")
AC_MUTANTS = ("lp_two_components", "std_for_var", "value_col1")


def _caught(ref, mut, keys):
    return [k for k in keys if R.ratio(mut[k][0], ref[k])[1].any()]


@pytest.mark.parametrize("case", R.POLICY_CASES, ids=R.case_id)
def test_policy_bound_rejects_mutants(case, rows):
    obs, eps = rows
    spec = R.policy_spec(case, R.policy_modules(case))
    ref = R.policy_forward(spec, obs, eps)
    keys = [k for k in ("buffer_actions", "log_prob", "value") if k in ref]
    mutants = FORWARD_MUTANTS + (AC_MUTANTS if case[0] == "actor_critic" else ())
    for m in mutants:
        mut = R.policy_forward(spec, obs, eps, mutant=m)
        caught = _caught(ref, mut, keys)
        assert caught, f"{R.case_id(case)}: mutant {m} stays inside the bound"
        if m == "shift_last_row":   # only the last env differs
            assert all(not R.ratio(mut[k][0][:-1], (ref[k][0][:-1], ref[k][1][:-1]))[1].any() for k in keys)


def test_actor_bound_rejects_mutants(rows):
    obs, eps = rows
    lin, mu, ls = R.actor_modules()
    for e in (None, eps):
        ref = R.actor_forward(lin, mu, ls, obs, e)
        for m in FORWARD_MUTANTS:
            mut = R.actor_forward(lin, mu, ls, obs, e, mutant=m)
            assert _caught(ref, mut, ["actions"]), f"sac actor: mutant {m} stays inside the bound"


def test_comparator_rejects_non_finite():
    ref = (np.array([1.0, 2.0, 3.0]), np.array([1e-6, 1e-6, 1e-6]))
    assert R.ratio(np.array([1.0, 2.0, 3.0]), ref)[0] == 0.0
    for bad in (np.nan, np.inf, -np.inf):
        got = np.array([1.0, bad, 3.0])
        r, mask = R.ratio(got, ref)
        assert r == np.inf and mask.tolist() == [False, True, False]
        with pytest.raises(AssertionError, match="outside the fp64 bound"):
            R.assert_within(got.astype(np.float32), ref, "non-finite")


def test_inputs_cover_the_observation_range(rows):
    obs, _ = rows
    real = obs[33:]              # the 28 special rows hold 5 real rows interleaved: 33 rows before the rest
    assert np.abs(real).max() < 10
    assert len(real) >= 4000 and real.min() < -1.57 and real.max() > 6.28
    nz = (obs[:33] != 0).sum(axis=1)
    assert (nz == 1).sum() >= 18 and (nz == 0).sum() >= 2 and (np.abs(obs[:33]).max(axis=1) == 100).sum() == 8


def test_input_rows_do_not_change_when_fixtures_are_added():
    """input_rows() draws its real observations from the recorded traces under tests/golden/: a new fixture with an `obs`
    array would silently change the inputs of every policy / gradient test, the bit-recorded ones included.  The rows are
    pinned; a fixture added later is excluded by name in policy_ref.input_rows (as the smooth*_xf_* records are)."""
    import hashlib
    x = R.input_rows()
    assert x.shape == (5028, 18) and x.dtype == np.float32
    assert hashlib.sha256(x.tobytes()).hexdigest() == "7c506f41970a2853c4f8015569accfdd6066c18ccaf1ebaf183b141bf7479e9f"
