"""GPU: the gradient kernels, the TD target and the sampled rollout policy reproduce recorded outputs BIT FOR BIT.

tests/golden/grad_bits.json holds the SHA-256 digest of the raw bytes of every output of

    FusedTDTarget        SAC and TD3, in-kernel Philox noise (tag 2), every part
    FusedCriticGrad      SAC and TD3, every part
    FusedActorGrad       in-kernel Philox noise (tag 3) and given noise, every part
    FusedTD3ActorGrad    every part
    FusedPPOGrad         H = 64 / 128 x Tanh / ReLU, normalize_advantage on, every part
    FusedPolicy.sample   actor-critic ReLU 128 (the tag-0 stream)

at B = 1 (one partial tile), 17 (a full tile and one row), 1043 (66 tiles on 64 workgroups: two of them walk two tiles) and
8200 (513 tiles: kCgMaxGroups workgroups), as a library built from the sources BEFORE the tile helpers of
csrc/meshenv_grad_tile.h were shared computed them.  The helpers change no arithmetic expression and no reduction order, so the
in-tree library must give the same bytes; the fp64 tests beside this one would let a reordered sum pass.

The digests pin this compiler's tanhf / logf / expf / sincosf (ocml) as well as the kernels.  After a ROCm upgrade that changes
one of them, re-record the fixture from the UNCHANGED sources (`python tests/test_gpu_grad_bits.py --record`, with MESHENV_LIB
naming the library to record from, or the in-tree one) and only then look at kernel changes.

Inputs and weights are exact integer arithmetic (a multiplicative hash of the flat index mod 2^32, its top 16 bits scaled by a
power of two in float32): no library RNG and no transcendental function, the same bits on any machine.  The scales keep the
pre-activations on both sides of zero; `--record` first checks on the CPU, with critic_grad_ref / ppo_grad_ref, that between a
quarter and three quarters of the ReLU masks are set and that PPO's surrogate both passes and clips rows."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, "golden", "grad_bits.json")
BS = (1, 17, 1043, 8200)
SEED = (0x5EED << 32) | 77          # both words of seed and counter reach the Philox key / counter
COUNTER = (3 << 32) | 1000
M32 = 0xFFFFFFFF
PPO_CASES = [(H, act) for H in (64, 128) for act in ("tanh", "relu")]
CASES = (["td_target-sac", "td_target-td3", "critic_grad-sac", "critic_grad-td3", "actor_grad-philox", "actor_grad-noise",
          "td3_actor_grad"] + [f"ppo_grad-{act}{H}" for H, act in PPO_CASES] + ["policy-sample"])


# ----------------------------------------------------------------------------------------------------------- inputs
def fill(shape, salt, scale, shift=0.0):
    """float32 array: element i = k_i * (scale / 32768) + shift with k_i in [-32768, 32767] the top 16 bits of a hash of
    (i, salt); scale a power of two, so every value is exact."""
    n = int(np.prod(shape))
    h = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(salt) * np.uint64(0x9E3779B9) + np.uint64(12345)) & np.uint64(M32)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(2246822519)) & np.uint64(M32)
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(3266489917)) & np.uint64(M32)
    h ^= h >> np.uint64(16)
    k = (h >> np.uint64(16)).astype(np.int64) - 32768
    v = k.astype(np.float32) * np.float32(scale / 32768.0) + np.float32(shift)
    return np.ascontiguousarray(v.reshape(shape))


def _scale(fan_in):
    return 0.25 if fan_in <= 21 else (0.125 if fan_in <= 128 else 0.0625)


def _set(layers, salt):
    """Overwrite weight and bias of the torch Linear layers, in order, with fill()."""
    import torch
    with torch.no_grad():
        for i, l in enumerate(layers):
            l.weight.copy_(torch.from_numpy(fill(tuple(l.weight.shape), salt + 2 * i, _scale(l.weight.shape[1]))))
            l.bias.copy_(torch.from_numpy(fill(tuple(l.bias.shape), salt + 2 * i + 1, 0.0625)))


def sac_modules():
    import td_target_ref as T
    m = T.sac_modules()
    _set(m["lin"] + [m["mu"], m["ls"]], 100)
    _set(m["q1"], 120)
    _set(m["q2"], 140)
    return m


def td3_modules():
    import td_target_ref as T
    m = T.td3_modules()
    _set(m["lin"] + [m["mu"]], 200)
    _set(m["q1"], 220)
    _set(m["q2"], 240)
    return m


def ppo_modules(H, act):
    import torch

    import policy_ref as R
    m = R.policy_modules(("actor_critic", H, act))
    _set(m["pi"] + [m["action_net"]], 300 + H)
    _set(m["vf"] + [m["value_net"]], 320 + H)
    m["log_std"] = torch.nn.Parameter(torch.tensor([-0.5, 0.0, 0.25]))
    m.update(act=act, H=H, a2c=False)
    return m


def batch(B):
    """The batch of every case: what a case does not read it ignores."""
    done = (fill((B,), 6, 1.0) > 0.5).astype(np.float32)
    return dict(obs=fill((B, 18), 1, 2.0), actions=fill((B, 3), 2, 1.0), y=fill((B,), 3, 1.0), noise=fill((B, 3), 4, 2.0),
                rewards=fill((B,), 5, 1.0), dones=done, old_log_prob=fill((B,), 7, 2.0, -4.0), adv=fill((B,), 8, 1.0, 0.25),
                returns=fill((B,), 9, 1.0))


PPO_HYPER = dict(clip_range=0.2, ent_coef=0.01, vf_coef=0.5, normalize_advantage=True, max_grad_norm=0.5)


def check_fractions():
    """CPU, fp64 references: the inputs exercise both sides of every ReLU and of PPO's clip.  Returns the fractions."""
    import critic_grad_ref as G
    import ppo_grad_ref as P
    b, out = batch(1043), {}
    for kind, m in (("sac", sac_modules()), ("td3", td3_modules())):
        _, info = G.critic_grad(dict(kind=kind, q1=m["q1"], q2=m["q2"]), b["obs"], b["actions"], b["y"])
        for c in (1, 2):
            for l, mk in enumerate(info[c]["mask"]):
                out[f"critic-{kind} q{c} layer {l} mask"] = float(np.mean(mk))
    m = ppo_modules(128, "relu")
    data = dict(observations=b["obs"], actions=b["actions"], old_log_prob=b["old_log_prob"], advantages=b["adv"], returns=b["returns"])
    ref, info = P.ppo_grad(m, data, P.hyper(**PPO_HYPER))
    for t in ("pi", "vf"):
        for l, mk in enumerate(info[f"mask_{t}"]):
            out[f"ppo-relu128 {t} layer {l} mask"] = float(np.mean(mk))
    out["ppo-relu128 pass share"] = float(info["pass_share"])
    out["ppo-relu128 clip_fraction"] = float(ref["clip_fraction"][0])
    for k, v in out.items():
        lo, hi = (0.05, 0.95) if k.startswith("ppo-relu128 pass") or k.endswith("clip_fraction") else (0.25, 0.75)
        assert lo <= v <= hi, f"{k}: {v:.3f} outside [{lo}, {hi}]"
    return out


# ----------------------------------------------------------------------------------------------------------- the launches
def _cuda(layers):
    return [l.cuda() for l in layers]


def _flat(prefix, v, out):
    if isinstance(v, (list, tuple)):
        for i, x in enumerate(v):
            _flat(f"{prefix}.{i}", x, out)
    elif v is not None:
        out[prefix] = v


def _grads(handle, out):
    for i, (p, _) in enumerate(handle.spec.offsets()):
        out[f"grad.{i}"] = p.grad


def make_case(name):
    """(run, close): run(b) launches the case on the device batch b (a dict of CUDA tensors) and returns {output: tensor}."""
    import torch

    import reinforcementlearning4meshgeneration_amd as pkg   # noqa: F401
    from reinforcementlearning4meshgeneration_amd.actor_grad import FusedActorGrad
    from reinforcementlearning4meshgeneration_amd.critic_grad import FusedCriticGrad
    from reinforcementlearning4meshgeneration_amd.policy import FusedPolicy
    from reinforcementlearning4meshgeneration_amd.ppo_grad import FusedPPOGrad
    from reinforcementlearning4meshgeneration_amd.td3_actor_grad import FusedTD3ActorGrad
    from reinforcementlearning4meshgeneration_amd.td_target import FusedTDTarget
    family, _, variant = name.partition("-")
    lec = lambda: torch.full((1,), -0.5, device="cuda", requires_grad=True)   # noqa: E731

    def finish(h, res, with_grads=True):
        out = {}
        for k, v in res.items():
            _flat(k, v, out)
        if with_grads:
            _grads(h, out)
        return out

    if family == "td_target":
        m = sac_modules() if variant == "sac" else td3_modules()
        lin, mu, q1, q2 = _cuda(m["lin"]), m["mu"].cuda(), _cuda(m["q1"]), _cuda(m["q2"])
        h = (FusedTDTarget.sac(lin, mu, m["ls"].cuda(), q1, q2, 0.99, log_ent_coef=lec()) if variant == "sac"
             else FusedTDTarget.td3(lin, mu, q1, q2, 0.99))

        def run(b):
            y, parts = h.target(next_observations=b["obs"], rewards=b["rewards"], dones=b["dones"], seed=SEED, counter=COUNTER,
                                return_parts=True)
            return finish(h, dict(target=y, **parts), with_grads=False)
    elif family == "critic_grad":
        m = sac_modules() if variant == "sac" else td3_modules()
        h = (FusedCriticGrad.sac if variant == "sac" else FusedCriticGrad.td3)(_cuda(m["q1"]), _cuda(m["q2"]))

        def run(b):
            loss, parts = h.backward(observations=b["obs"], actions=b["actions"], target_q_values=b["y"], return_parts=True)
            return finish(h, dict(loss=loss, **parts))
    elif family == "actor_grad":
        m = sac_modules()
        h = FusedActorGrad.sac(_cuda(m["lin"]), m["mu"].cuda(), m["ls"].cuda(), _cuda(m["q1"]), _cuda(m["q2"]), log_ent_coef=lec())

        def run(b):
            kw = dict(seed=SEED, counter=COUNTER) if variant == "philox" else dict(noise=b["noise"])
            la, le, parts = h.backward(observations=b["obs"], return_parts=True, **kw)
            return finish(h, dict(actor_loss=la, ent_coef_loss=le, **parts))
    elif family == "td3_actor_grad":
        m = td3_modules()
        h = FusedTD3ActorGrad.td3(_cuda(m["lin"]), m["mu"].cuda(), _cuda(m["q1"]))

        def run(b):
            loss, parts = h.backward(observations=b["obs"], return_parts=True)
            return finish(h, dict(loss=loss, **parts))
    elif family == "ppo_grad":
        act, H = variant[:4], int(variant[4:])
        m = ppo_modules(H, act)
        log_std = torch.nn.Parameter(m["log_std"].detach().cuda())
        h = FusedPPOGrad.actor_critic(_cuda(m["pi"]), _cuda(m["vf"]), m["action_net"].cuda(), m["value_net"].cuda(), log_std,
                                      activation=act)

        def run(b):
            res = h.backward(observations=b["obs"], actions=b["actions"], old_log_prob=b["old_log_prob"], advantages=b["adv"],
                             returns=b["returns"], return_parts=True, **PPO_HYPER)
            return finish(h, res)
    else:
        import policy_ref as R
        case = ("actor_critic", 128, "relu")
        m = ppo_modules(128, "relu")
        m["log_std"] = m["log_std"].detach()
        h = FusedPolicy(R.policy_spec(case, m))

        def run(b):
            return finish(h, h.sample(b["obs"], SEED, COUNTER), with_grads=False)
    return run, h.close


def digests(name):
    """{str(B): {output: sha256 of its bytes}} of one case on the loaded library."""
    import torch
    run, close = make_case(name)
    out = {}
    for B in BS:
        b = {k: torch.from_numpy(v).cuda() for k, v in batch(B).items()}
        res = run(b)
        torch.cuda.synchronize()
        out[str(B)] = {k: hashlib.sha256(v.detach().cpu().contiguous().numpy().tobytes()).hexdigest() for k, v in sorted(res.items())}
    close()
    return out


# ----------------------------------------------------------------------------------------------------------- the test
@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("name", CASES)
def test_outputs_reproduce_recorded_bits(name, recorded):
    got, want = digests(name), recorded["cases"][name]
    assert set(got) == set(want) == {str(B) for B in BS}
    bad = []
    for B in got:
        assert set(got[B]) == set(want[B]), (name, B, sorted(set(got[B]) ^ set(want[B])))
        bad += [f"B={B} {k}" for k in got[B] if got[B][k] != want[B][k]]
    assert not bad, f"{name}: {len(bad)} outputs differ from the recorded bits: {bad[:12]}"


def record():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from source_state import state
    fractions = check_fractions()
    for k, v in fractions.items():
        print(f"{k}: {v:.3f}", flush=True)
    st = state()
    fixture = dict(recorded_from=dict(library=st["library"], library_built_from=st["library_built_from"]), batch_sizes=list(BS),
                   cases={name: digests(name) for name in CASES})
    with open(FIXTURE, "w") as f:
        json.dump(fixture, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {sum(len(o) for c in fixture['cases'].values() for o in c.values())} digests of {len(CASES)} cases to {FIXTURE}")


if __name__ == "__main__":
    if "--check" in sys.argv:
        for k, v in check_fractions().items():
            print(f"{k}: {v:.3f}")
    elif "--record" in sys.argv:
        record()
    else:
        sys.exit("usage: python tests/test_gpu_grad_bits.py --record | --check")
