"""GPU: every refusal of the bind and backward entry points of the critic (SAC and TD3 kinds), SAC actor, TD3 actor, PPO
(hidden 64 ReLU, 128 Tanh) and FNN gradient handles, through the C-ABI itself (DDPG's are pinned in
tests/test_gpu_ddpg_range.py): the code, the exact text of *_last_error (tests/grad_refusals.py), a NaN-filled gradient
buffer and loss left as they were, nothing half-bound, and after all of them one good bind and backward that is bit-equal to
the same call on a handle that saw no refusal.

B = 33: two full 16-row tiles and a one-row tail.  A refused call reads no device memory, and the misaligned pointers lie
inside live tensors."""
import copy
import ctypes as C

import numpy as np
import pytest

import actor_grad_ref as AG
import critic_grad_ref as CG
import fnn_grad_ref as FG
import fnn_ref as FR
import grad_refusals as X
import policy_ref as R
import ppo_grad_ref as PG
import td3_actor_grad_ref as TG
import td_target_ref as T

pytestmark = pytest.mark.gpu

B = 33
NAN = float("nan")


@pytest.fixture(scope="module")
def rows():
    return R.input_rows()


def _arr(ptrs):
    return (C.c_void_p * len(ptrs))(*ptrs)


def _cuda(layers):
    return [copy.deepcopy(l).cuda() for l in layers]


def _dev(torch, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


class Family:
    """One family on the GPU: `fused`, the library's own class bound to the tensors (the handle that sees no refusal), and
    what the raw calls take.  bind(h, arrays, counts, grad, n_grad) and the backward argument list are the entry point's."""

    def __init__(self, torch, key, family, fused, nets, bind, create_args, args, required, loss, outputs, options=(), parts=(),
                 count_nets=None):
        self.torch, self.key, self.family, self.fused, self.nets, self.create_args = torch, key, family, fused, nets, create_args
        self.L, self.prefix = fused._L, fused.PREFIX
        self._bind, self.args, self.required, self.loss, self.outputs = bind, args, required, loss, outputs
        self.options, self.parts = options, parts          # [(overrides, text key)], [(argument, text key)]
        self.count_nets = [[k] for k in range(len(nets))] if count_nets is None else count_nets   # nets behind each count argument
        self.n_grad = X.BINDS[key]["n_grad"]
        assert fused.spec.n_grad == self.n_grad and [len(n) for n in nets] == [n["count"] for n in X.BINDS[key]["nets"]]
        self.grad = torch.full((self.n_grad,), NAN, device="cuda")      # the gradient buffer of the handle that is refused
        self.n_loss = None          # the floats of the loss output that the entry point defines: all of them

    def fn(self, name):
        return getattr(self.L, f"{self.prefix}_{name}")

    def create(self):
        h = C.c_void_p()
        stream = self.torch.cuda.current_stream().cuda_stream
        assert self.fn("create")(0, C.c_void_p(stream), *self.create_args, C.byref(h)) == 0
        return h

    def bind(self, h, case=("good",), grad=None):
        """The bind of `case` (grad_refusals.bind_cases), or None where the entry point has no such argument."""
        ptrs = [[t.data_ptr() for t in net] for net in self.nets]
        assert all(p % 16 == 0 for net in ptrs for p in net)
        counts = [len(p) for p in ptrs]
        arrays = None
        g, n_grad = (self.grad if grad is None else grad).data_ptr(), self.n_grad
        kind = case[0]
        if kind == "count":
            if self.count_nets == []:
                return None
            counts = [c + case[2] if any(k in nets and case[1] in nets for nets in self.count_nets) else c for k, c in enumerate(counts)]
        elif kind == "n_grad":
            n_grad = case[1]
        elif kind == "null_grad":
            g = None
        elif kind == "null_tensor":
            ptrs[case[1]][case[2]] = None
        elif kind == "off4":
            ptrs[case[1]][case[2]] += 4
        elif kind == "grad_off2":
            g += 2
        arrays = [_arr(p) for p in ptrs]
        if kind == "null_array":
            arrays[case[1]] = None
        return self._bind(h, arrays, counts, g, n_grad)

    def backward(self, h, **over):
        a = dict(self.args, **over)
        return self.fn("backward")(h, *a.values())

    def error(self, h):
        msg = self.fn("last_error")(h)
        return None if msg is None else msg.decode()


def _refusals(f):
    torch, L = f.torch, f.L
    from reinforcementlearning4meshgeneration_amd import _capi
    loss_t = f.keep_loss
    f.fused.grad_buffer.fill_(NAN)
    loss_t.fill_(NAN)

    def refused(h, rc, code, text, what):
        torch.cuda.synchronize()
        assert rc == code and f.error(h) == text, (f.key, what, rc, code, f.error(h), text)
        assert bool(torch.isnan(f.grad).all()) and bool(torch.isnan(f.fused.grad_buffer).all()) and bool(torch.isnan(loss_t).all()), (f.key, what)

    state = X.backward_text(f.family, "state")
    h = f.create()
    # ---- a fresh handle: a backward before a bind, every refusal of the bind, and still nothing bound
    refused(h, f.backward(h), _capi.E_STATE, state, "backward before bind")
    seen = 0
    for case, text in X.bind_cases(f.key):
        if not text:
            continue
        rc = f.bind(h, case)
        if rc is None:
            continue
        refused(h, rc, _capi.E_ARG, text, case)
        seen += 1
    assert seen >= 8
    refused(h, f.backward(h), _capi.E_STATE, state, "backward after refused binds")
    # ---- the handle bound: every refusal of the backward
    assert f.bind(h) == 0, f.error(h)
    required = X.backward_text(f.family, "required")
    for n in (0, -1):
        refused(h, f.backward(h, n=n), _capi.E_ARG, required, f"n = {n}")
    for name in f.required:
        refused(h, f.backward(h, **{name: None}), _capi.E_ARG, required, f"{name} = NULL")
    for over, what in f.options:
        refused(h, f.backward(h, **over), _capi.E_ARG, X.backward_text(f.family, what), over)
    for name, what in f.parts:
        ptrs = list(f.args[name])
        for i in range(len(ptrs)):
            p = list(ptrs)
            p[i] = None
            refused(h, f.backward(h, **{name: _arr(p)}), _capi.E_ARG, X.backward_text(f.family, what), f"{name}[{i}] = NULL")
    # ---- one good call on the handle that was refused and on the one that was not: the same bits everywhere
    got = []
    for handle, grad in ((h, f.grad), (f.fused._h, f.fused.grad_buffer)):
        for t in f.outputs:
            t.fill_(NAN)
        assert f.backward(handle) == 0, f.error(handle)
        torch.cuda.synchronize()
        got.append([grad.clone()] + [t.clone() for t in f.outputs])
    for a, b in zip(*got):
        assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), f.key
    assert not any(bool(torch.isnan(f.grad[at:at + p.numel()]).any()) for p, at in f.fused.spec.offsets()), f.key
    assert not bool(torch.isnan(loss_t[:f.n_loss]).any()), f.key
    f.fn("destroy")(h)
    f.fused.close()


def _family(torch, key, family, fused, nets, bind, create_args, args, loss, outputs, **kw):
    f = Family(torch, key, family, fused, nets, bind, create_args, args, kw.pop("required"), loss, outputs, **kw)
    f.keep_loss = next(t for t in outputs if t.data_ptr() == args[loss])
    return f


def _empty(torch, *shape):
    return torch.empty(*shape, device="cuda")


@pytest.mark.parametrize("kind", ["sac", "td3"])
def test_critic(kind, rows):
    import torch
    from reinforcementlearning4meshgeneration_amd.critic_grad import FusedCriticGrad
    m = CG.critic_modules(kind)
    q1, q2 = _cuda(m["q1"]), _cuda(m["q2"])
    fused = (FusedCriticGrad.sac if kind == "sac" else FusedCriticGrad.td3)(q1, q2)
    s, L = fused.spec, fused._L
    H, NL = (128, 3) if kind == "sac" else (256, 2)
    obs, act, y = _dev(torch, *CG.batch(B, rows))
    loss, qa, qb = _empty(torch, 1), _empty(torch, B), _empty(torch, B)
    acts1, acts2 = [_empty(torch, B, H) for _ in range(NL)], [_empty(torch, B, H) for _ in range(NL)]
    p1, p2 = [t.data_ptr() for t in acts1], [t.data_ptr() for t in acts2]
    args = dict(n=B, obs=obs.data_ptr(), actions=act.data_ptr(), target=y.data_ptr(), loss=loss.data_ptr(), q1=qa.data_ptr(),
                q2=qb.data_ptr(), acts1=_arr(p1), acts2=_arr(p2))
    f = _family(torch, f"critic-{kind}", "critic", fused, [list(s.q1), list(s.q2)],
                lambda h, a, c, g, n: L.meshenv_critic_grad_bind(h, a[0], a[1], c[0], g, n), (s.kind,), args, "loss",
                [loss, qa, qb, *acts1, *acts2], required=("obs", "actions", "target", "loss"),
                options=[(dict(acts2=None), "pair"), (dict(acts1=None), "pair")], count_nets=[[0, 1]])
    # (a null in either array with the other whole)
    f.parts = [("acts1", "acts"), ("acts2", "acts")]
    _refusals(f)


def test_sac_actor(rows):
    import torch
    from reinforcementlearning4meshgeneration_amd.actor_grad import FusedActorGrad
    m = T.sac_modules()
    lin, q1, q2 = _cuda(m["lin"]), _cuda(m["q1"]), _cuda(m["q2"])
    mu, ls = _cuda([m["mu"], m["ls"]])
    lec = torch.full((1,), -0.5, device="cuda", requires_grad=True)
    fused = FusedActorGrad.sac(lin, mu, ls, q1, q2, log_ent_coef=lec)
    s, L = fused.spec, fused._L
    obs, eps = _dev(torch, *AG.batch(B, rows))
    losses, eps_out = _empty(torch, 2), _empty(torch, B, 3)
    parts = [_empty(torch, *sh) for sh in ((B, 3), (B,), (B,), (B,), (B, 3), (B, 3), (B, 3))]
    acts = [_empty(torch, B, 128) for _ in range(9)]
    args = dict(n=B, obs=obs.data_ptr(), noise=eps.data_ptr(), sample=0, seed=C.c_uint64(7), counter=C.c_uint64(0),
                losses=losses.data_ptr(), eps_out=eps_out.data_ptr(), parts=_arr([t.data_ptr() for t in parts]),
                acts=_arr([t.data_ptr() for t in acts]))
    f = _family(torch, "actor", "actor", fused, [list(s.actor), list(s.q1), list(s.q2)],
                lambda h, a, c, g, n: L.meshenv_actor_grad_bind(h, a[0], c[0], a[1], a[2], c[1], lec.data_ptr(), g, n),
                (s.ent_coef, s.target_entropy), args, "losses", [losses, eps_out, *parts, *acts], required=("obs", "losses"),
                options=[(dict(sample=1), "exclusive"), (dict(noise=None), "eps")], parts=[("parts", "parts"), ("acts", "acts")],
                count_nets=[[0], [1, 2]])
    _refusals(f)


def test_td3_actor(rows):
    import torch
    from reinforcementlearning4meshgeneration_amd.td3_actor_grad import FusedTD3ActorGrad
    m = TG.modules()
    lin, q1 = _cuda(m["lin"]), _cuda(m["q1"])
    mu, = _cuda([m["mu"]])
    fused = FusedTD3ActorGrad.td3(lin, mu, q1)
    s, L = fused.spec, fused._L
    obs, _ = _dev(torch, *TG.batch(B, rows))
    loss = _empty(torch, 1)
    parts = [_empty(torch, *sh) for sh in ((B, 3), (B,), (B, 3), (B, 3))]
    acts = [_empty(torch, B, 256) for _ in range(4)]
    args = dict(n=B, obs=obs.data_ptr(), loss=loss.data_ptr(), parts=_arr([t.data_ptr() for t in parts]),
                acts=_arr([t.data_ptr() for t in acts]))
    f = _family(torch, "td3-actor", "td3-actor", fused, [list(s.actor), list(s.q1)],
                lambda h, a, c, g, n: L.meshenv_td3_actor_grad_bind(h, a[0], c[0], a[1], c[1], g, n), (), args, "loss",
                [loss, *parts, *acts], required=("obs", "loss"), parts=[("parts", "parts"), ("acts", "acts")])
    _refusals(f)


@pytest.mark.parametrize("case", ["ppo-relu64", "ppo-tanh128"])
def test_ppo(case, rows):
    import torch
    from reinforcementlearning4meshgeneration_amd import _capi
    from reinforcementlearning4meshgeneration_amd.ppo_grad import ACTIVATIONS, OUTPUTS, FusedPPOGrad
    m = PG.modules(case)
    data = PG.batch(m, B, rows)
    pi, vf = _cuda(m["pi"]), _cuda(m["vf"])
    an, vn = _cuda([m["action_net"], m["value_net"]])
    log_std = torch.nn.Parameter(m["log_std"].detach().clone().cuda())
    fused = FusedPPOGrad.actor_critic(pi, vf, an, vn, log_std, m["act"])
    s, L = fused.spec, fused._L
    H, act = s.hidden, ACTIVATIONS[s.activation]
    d = {k: torch.from_numpy(v).cuda() for k, v in data.items()}
    out = _empty(torch, _capi.PPO_GRAD_OUTPUTS)
    parts = [_empty(torch, B) for _ in range(5)]
    acts = [_empty(torch, B, H) for _ in range(4)]
    args = dict(n=B, obs=d["observations"].data_ptr(), actions=d["actions"].data_ptr(), old=d["old_log_prob"].data_ptr(),
                adv=d["advantages"].data_ptr(), ret=d["returns"].data_ptr(), a2c=0, clip_range=0.2, ent_coef=0.01, vf_coef=0.5,
                normalize=1, clip_grad=1, max_grad_norm=0.1, out=out.data_ptr(), parts=_arr([t.data_ptr() for t in parts]),
                acts=_arr([t.data_ptr() for t in acts]))
    bad = [dict(clip_range=NAN), dict(clip_range=float("inf")), dict(ent_coef=NAN), dict(vf_coef=float("-inf")), dict(max_grad_norm=NAN),
           dict(clip_range=0.0), dict(max_grad_norm=0.0)]
    f = _family(torch, f"ppo-{H}", "ppo", fused, [list(s.params)],
                lambda h, a, c, g, n: L.meshenv_ppo_grad_bind(h, H, act, a[0], c[0], g, n), (), args, "out",
                [out, *parts, *acts], required=("obs", "actions", "adv", "ret", "out"),
                options=[(dict(old=None), "old")] + [(o, "coefficients") for o in bad], parts=[("parts", "parts"), ("acts", "acts")])
    f.n_loss = len(OUTPUTS)     # (out_dev has a spare eighth float)
    # ---- the shape refusals in front of the bind's count check, on a handle of their own
    h = f.create()
    g = f.grad.data_ptr()
    ptrs = _arr([t.data_ptr() for t in s.params])
    for hidden, activation, text in ((256, act, X.PPO_BIND_WIDTH_256), (32, act, X.PPO_BIND_SHAPE), (H, 2, X.PPO_BIND_SHAPE)):
        assert L.meshenv_ppo_grad_bind(h, hidden, activation, ptrs, 13, g, f.n_grad) == _capi.E_ARG and f.error(h) == text
    assert f.backward(h) == _capi.E_STATE and f.error(h) == X.backward_text("ppo", "state")
    f.fn("destroy")(h)
    _refusals(f)


def test_fnn():
    import torch
    from reinforcementlearning4meshgeneration_amd import FusedFNNTrain
    seed = FG.STUDENTS[1]
    pol = copy.deepcopy(FR.make_policy(seed)).cuda()
    fused = FusedFNNTrain(pol, torch.optim.Adam(pol.parameters(), lr=FG.LR))
    s, L = fused.spec, fused._L
    x_np, y_np, _ = FG.batch(seed, B)
    x, y = _dev(torch, x_np, y_np)
    out = _empty(torch, 4)
    args = dict(n=B, N=B, x=x.data_ptr(), y=y.data_ptr(), rows=None, out=out.data_ptr(), accum=None)
    f = _family(torch, "fnn", "fnn", fused, [list(s.params)], lambda h, a, c, g, n: L.meshenv_fnn_grad_bind(h, a[0], g, n), (), args,
                "out", [out], required=("x", "y", "out"), options=[(dict(n=B + 1), "required"), (dict(N=0), "required")], count_nets=[])
    _refusals(f)
