"""What the fused train-step classes recognise of SB3 2.x's SAC / TD3 / PPO / A2C objects, and the checks of the LIVE
parameters they bind: one place for every refusal.  Duck-typed (SB3 is not imported; the tests use stand-ins): layers are
``torch.nn.Linear``-like objects (``.weight [out][in]``, ``.bias``), networks are what ``create_mlp`` builds.

The networks are the ones the reference trains (rl/baselines/RL_Mesh.py:179-222): ``SUPPORTED``."""
from __future__ import annotations

from . import _capi

KIND_SAC, KIND_TD3, KIND_DDPG = 0, 1, 2
OBS_DIM, ACT_DIM = _capi.OBS_DIM, _capi.ACT_DIM
Q_IN = OBS_DIM + ACT_DIM
HIDDEN = {KIND_SAC: (128, 3), KIND_TD3: (256, 2)}     # width, hidden layers
SUPPORTED = ("SAC: ReLU [128, 128, 128] actor (mu and log_std heads) with twin ReLU [128, 128, 128] critics and either the "
             "learned log_ent_coef tensor or a fixed ent_coef; TD3: ReLU [256, 256] tanh actor with twin ReLU [256, 256] "
             "critics; DDPG (FusedPolicy, FusedTDTarget and FusedDDPGGrad only): ReLU [400, 300] tanh actor with one ReLU "
             "[400, 300] critic (n_critics = 1); 18 observations, 3 actions, critic input cat(obs, action) = 21; float32 "
             "contiguous parameters")
DDPG_WIDTHS = (400, 300)                              # SB3's TD3Policy default net_arch, what DDPG('MlpPolicy', env) builds


def _refuse(what):
    raise ValueError(f"{what}; supported: {SUPPORTED}")


def _sequential(seq):
    """The Linear layers and the activations of an SB3 ``create_mlp`` nn.Sequential (Linear, act, Linear, act, ...)."""
    mods = list(seq)
    linears = [m for m in mods if type(m).__name__ == "Linear"]
    acts = {type(m).__name__.lower() for m in mods if type(m).__name__ != "Linear"}
    return linears, acts


def _param(x, what, shape, refuse=None):
    """A live parameter: float32, contiguous, of the expected shape (a torch tensor: its storage is what gets bound)."""
    refuse = refuse or _refuse
    if not hasattr(x, "data_ptr") or not hasattr(x, "is_contiguous"):
        refuse(f"{what} is {type(x).__name__}, not a torch tensor")
    if str(x.dtype) != "torch.float32":
        refuse(f"{what} has dtype {x.dtype}; parameters must be float32")
    if tuple(x.shape) != tuple(shape):
        refuse(f"{what} has shape {tuple(x.shape)}, expected {tuple(shape)}")
    if not x.is_contiguous():
        refuse(f"{what} is not contiguous")
    return x


def _mlp(layers, head_layers, n_in, kind, what):
    """[w1, b1, ..., head_w, head_b, ...] of an MLP of the kind's width and depth; each head has (name, n_out, layer)."""
    H, NL = HIDDEN[kind]
    layers = list(layers)
    widths = [tuple(getattr(l.weight, "shape", ())) for l in layers]
    if len(layers) != NL or any(w[:1] != (H,) for w in widths):
        _refuse(f"{what}: hidden layers {[w[0] if w else None for w in widths]}")
    out, k = [], n_in
    for i, l in enumerate(layers):
        out += [_param(l.weight, f"{what}[{i}].weight", (H, k)), _param(l.bias, f"{what}[{i}].bias", (H,))]
        k = H
    for name, n_out, l in head_layers:
        out += [_param(l.weight, f"{what} {name}.weight", (n_out, H)), _param(l.bias, f"{what} {name}.bias", (n_out,))]
    return out


def _widths(layers):
    """The output widths of Linear-like layers (None where a weight has no shape)."""
    return [(tuple(getattr(getattr(l, "weight", None), "shape", ())) or (None,))[0] for l in layers]


def ddpg_mlp(layers, head, n_in, n_out, what):
    """[w1, b1, w2, b2, head_w, head_b] of a [400, 300] MLP: DDPG's actor (18 -> 3) or critic (21 -> 1)."""
    layers = list(layers)
    if tuple(_widths(layers)) != DDPG_WIDTHS:
        _refuse(f"{what}: hidden layers {_widths(layers)}")
    H1, H2 = DDPG_WIDTHS
    return [_param(layers[0].weight, f"{what}[0].weight", (H1, n_in)), _param(layers[0].bias, f"{what}[0].bias", (H1,)),
            _param(layers[1].weight, f"{what}[1].weight", (H2, H1)), _param(layers[1].bias, f"{what}[1].bias", (H2,)),
            _param(head.weight, f"{what} output.weight", (n_out, H2)), _param(head.bias, f"{what} output.bias", (n_out,))]


def ddpg_actor_params(actor_layers, mu):
    """The six tensors of DDPG's actor in bind order: w1 b1 w2 b2 mu_w mu_b."""
    return ddpg_mlp(actor_layers, mu, OBS_DIM, ACT_DIM, "actor")


def ddpg_critic_params(q, what="q_networks[0]"):
    """The six tensors of DDPG's one q_network (an nn.Sequential(Linear, ReLU, Linear, ReLU, Linear) or its Linear layers)."""
    linears = _relu_linears(q, what, 2)
    return ddpg_mlp(linears[:-1], linears[-1], Q_IN, 1, what)


def is_ddpg(model, actor_attr="actor_target", critic_attr="critic_target") -> bool:
    """Whether ``model`` is a DDPG model as SB3 constructs it: ``<actor_attr>.mu`` and ONE q_network (``n_critics == 1``), both
    of hidden widths [400, 300] (the activations are judged where the layers are read).  Every other single-critic model (a
    TD3 or SAC model built with n_critics = 1 at its own widths) is not, and meets twin_critics' refusal."""
    actor, critic = getattr(model, actor_attr, None), getattr(model, critic_attr, None)
    if not hasattr(actor, "mu") or critic is None or not hasattr(critic, "q_networks"):
        return False
    qs = list(critic.q_networks)
    if int(getattr(critic, "n_critics", len(qs))) != 1 or len(qs) != 1:
        return False
    mu = [m for m in actor.mu if type(m).__name__ == "Linear"]
    q = [m for m in qs[0] if type(m).__name__ == "Linear"]
    return tuple(_widths(mu[:-1])) == DDPG_WIDTHS and tuple(_widths(q[:-1])) == DDPG_WIDTHS


def ddpg_target_nets(model):
    """(actor_target's hidden layers, its mu, critic_target.q_networks[0]) of a model is_ddpg() took."""
    _flatten_only(model.critic_target, "critic_target", shared=bool(getattr(model.critic_target, "share_features_extractor", False)))
    layers, mu = td3_actor(model.actor_target)
    return layers, mu, list(model.critic_target.q_networks)[0]


def _relu_linears(seq, what, at_least=0):
    linears, acts = _sequential(seq)
    if acts - {"relu"}:
        _refuse(f"{what}: activations {sorted(acts)}")
    if len(linears) < at_least:
        _refuse(f"{what}: {len(linears)} Linear layers")
    return linears


def _critic(q, kind, what):
    """A q_network: an nn.Sequential(Linear, ReLU, ..., Linear) or a list of its Linear layers."""
    linears = _relu_linears(q, what, 2)
    return _mlp(linears[:-1], [("output", 1, linears[-1])], Q_IN, kind, what)


def sac_actor_params(actor_layers, mu, log_std):
    """The ten tensors of the SAC actor in bind order: w1 b1 w2 b2 w3 b3 mu_w mu_b log_std_w log_std_b."""
    return _mlp(actor_layers, [("mu", ACT_DIM, mu), ("log_std", ACT_DIM, log_std)], OBS_DIM, KIND_SAC, "actor")


def twin_params(kind, q1, q2):
    return _critic(q1, kind, "q_networks[0]"), _critic(q2, kind, "q_networks[1]")


def critic_kind(q, what):
    """SAC or TD3 from the widths of a q_network (the refusals of a shape that is neither come from _critic)."""
    linears, _ = _sequential(q)
    widths = [tuple(getattr(l.weight, "shape", ()))[:1] for l in linears[:-1]]
    for kind, (H, NL) in HIDDEN.items():
        if widths == [(H,)] * NL:
            return kind
    _refuse(f"{what}: hidden layers {[w[0] if w else None for w in widths]}")


def _flatten_only(owner, what, shared=False):
    fe = getattr(owner, "features_extractor", None)
    if fe is not None and type(fe).__name__ != "FlattenExtractor":
        how = " (share_features_extractor=True)" if shared else ""
        _refuse(f"{what}.features_extractor{how} is {type(fe).__name__}; only the MLP policies' FlattenExtractor is supported")


def twin_critics(model, attr, who="SAC / TD3", ddpg=False):
    """The two q_networks of ``model.<attr>`` (``critic``: the live ones, ``critic_target``).  who: the algorithms the caller
    takes; ddpg: whether a single critic may be DDPG's, which the refusal then says."""
    critic = getattr(model, attr, None)
    if critic is None or not hasattr(critic, "q_networks"):
        _refuse(f"{type(model).__name__} has no {attr}.q_networks: not an SB3 {who} model")
    qs = list(critic.q_networks)
    n_critics = int(getattr(critic, "n_critics", len(qs)))
    if n_critics != 2 or len(qs) != 2:
        hint = " (DDPG: one critic, no twin minimum)" if ddpg and n_critics == 1 else ""
        _refuse(f"{attr}.n_critics = {n_critics}{hint}; the twin critics of {who} (n_critics = 2) are supported")
    _flatten_only(critic, attr, shared=bool(getattr(critic, "share_features_extractor", False)))
    return qs


def first_critic(model, attr="critic", who="FusedTD3ActorGrad"):
    """``q_networks[0]`` of ``model.<attr>`` for n_critics >= 1: what TD3's / DDPG's ``critic.q1_forward`` evaluates."""
    critic = getattr(model, attr, None)
    if critic is None or not hasattr(critic, "q_networks"):
        _refuse(f"{type(model).__name__} has no {attr}.q_networks: not an SB3 TD3 / DDPG model")
    qs = list(critic.q_networks)
    n_critics = int(getattr(critic, "n_critics", len(qs)))
    if n_critics < 1 or len(qs) < 1:
        _refuse(f"{attr}.n_critics = {n_critics}; {who} reads q_networks[0]")
    _flatten_only(critic, attr, shared=bool(getattr(critic, "share_features_extractor", False)))
    return qs[0]


def td3_live_actor(model):
    """(hidden Linear layers, output Linear) of the LIVE actor of an SB3 TD3 / DDPG model (``model.actor``, not
    ``actor_target``); a SAC model is refused with the name of the class that takes it."""
    actor = getattr(model, "actor", None)
    if hasattr(actor, "latent_pi"):
        _refuse(f"{type(model).__name__} is a SAC model (actor.latent_pi): FusedActorGrad computes SAC's actor loss gradient")
    if not hasattr(actor, "mu"):
        _refuse(f"{type(model).__name__} has no actor.mu: not an SB3 TD3 / DDPG model")
    mods = list(actor.mu)
    tail = type(mods[-1]).__name__ if mods else "nothing"
    if tail != "Tanh":
        _refuse(f"actor.mu ends in {tail}; SB3's TD3 actor ends in Tanh")
    return td3_actor(actor, "actor")


def deterministic_live_params(model):
    """((width 1, width 2), the six live tensors) of the live actor of a TD3 ([256, 256]) or DDPG ([400, 300]) model."""
    layers, mu = td3_live_actor(model)
    if tuple(_widths(layers)) == DDPG_WIDTHS:
        return DDPG_WIDTHS, ddpg_actor_params(layers, mu)
    H = HIDDEN[KIND_TD3][0]
    return (H, H), td3_actor_params(layers, mu)


def td3_actor_params(actor_layers, mu):
    """The six tensors of the TD3 actor in bind order: w1 b1 w2 b2 w3 b3."""
    return _mlp(actor_layers, [("mu", ACT_DIM, mu)], OBS_DIM, KIND_TD3, "actor")


def sac_actor(actor, what="actor"):
    """The hidden Linear layers of an SB3 SAC ``Actor`` (``latent_pi``; its heads are ``actor.mu`` / ``actor.log_std``)."""
    _flatten_only(actor, what)
    if getattr(actor, "use_sde", False):
        _refuse(f"{what}.use_sde=True (gSDE actor) is not supported")
    linears = _relu_linears(actor.latent_pi, f"{what}.latent_pi")
    if type(actor.log_std).__name__ != "Linear":
        _refuse(f"{what}.log_std is {type(actor.log_std).__name__}, not a Linear head (gSDE?)")
    return linears


def td3_actor(actor, what="actor_target"):
    """(hidden Linear layers, output Linear) of an SB3 TD3 ``Actor``: ``mu`` = Sequential(Linear, ReLU, ..., Linear, Tanh)."""
    _flatten_only(actor, what)
    mods = list(actor.mu)
    if not mods or type(mods[-1]).__name__ != "Tanh":
        _refuse(f"{what}.mu must end in Tanh (SB3's TD3 actor)")
    linears = _relu_linears(mods[:-1], f"{what}.mu", 2)
    return linears[:-1], linears[-1]


# ---------------------------------------------------------------------------------------- PPO / A2C: ActorCriticPolicy
AC_GRAD_WIDTHS = (64, 128)            # what k_ppo_grad is built for; k_policy_forward also takes 256
AC_SUPPORTED = ("an SB3 ActorCriticPolicy (PPO, A2C) with a FlattenExtractor, pi and vf towers of two hidden layers of the same "
                "width 64 or 128 and one activation (ReLU or Tanh), action_net [3], value_net [1] and a state-independent "
                "log_std [3] (DiagGaussianDistribution, no gSDE, no squash_output); 18 observations; float32 contiguous "
                "parameters")


def _refuse_ac(what):
    raise ValueError(f"{what}; supported: {AC_SUPPORTED}")


def actor_critic_params(pi_layers, vf_layers, action_net, value_net, log_std, activation, widths=AC_GRAD_WIDTHS):
    """(hidden, 'relu' / 'tanh', the 13 live tensors in bind order: pi w1 b1 w2 b2 wh bh, vf likewise, log_std) of an
    actor-critic MLP policy.  widths: the hidden widths the caller's kernels are built for."""
    name = activation if isinstance(activation, str) else (activation.__name__ if isinstance(activation, type) else type(activation).__name__)
    name = name.lower()
    if name not in ("relu", "tanh"):
        _refuse_ac(f"activation {activation!r}")
    towers = []
    for what, layers, head, n_out in (("pi", pi_layers, action_net, ACT_DIM), ("vf", vf_layers, value_net, 1)):
        layers = list(layers)
        shapes = [tuple(getattr(getattr(l, "weight", None), "shape", ())) for l in layers]
        if len(layers) != 2 or any(len(sh) != 2 for sh in shapes):
            _refuse_ac(f"{what} tower: hidden layers {[sh[0] if sh else None for sh in shapes]}")
        towers.append((what, layers, head, n_out, shapes[0][0]))
    H, Hv = towers[0][4], towers[1][4]
    if H != Hv:
        _refuse_ac(f"pi width {H} and vf width {Hv} differ")
    if H == 256 and 256 not in widths:
        _refuse_ac("width 256 is not supported by the gradient kernel (its dW_2 needs a column split that is not built)")
    if H not in widths:
        _refuse_ac(f"hidden width {H}")
    out = []
    for what, layers, head, n_out, _ in towers:
        k = OBS_DIM
        for i, l in enumerate(layers):
            out += [_param(l.weight, f"{what}[{i}].weight", (H, k), _refuse_ac), _param(l.bias, f"{what}[{i}].bias", (H,), _refuse_ac)]
            k = H
        hn = "action_net" if what == "pi" else "value_net"
        out += [_param(head.weight, f"{hn}.weight", (n_out, H), _refuse_ac), _param(head.bias, f"{hn}.bias", (n_out,), _refuse_ac)]
    out.append(_param(log_std, "log_std", (ACT_DIM,), _refuse_ac))
    return H, name, out


def actor_critic_live(model, widths=AC_GRAD_WIDTHS):
    """(hidden, activation, 13 tensors) of a live SB3 ``ActorCriticPolicy``: ``mlp_extractor.policy_net`` / ``.value_net``,
    ``action_net``, ``value_net``, ``log_std``.  A ``PPO`` / ``A2C`` object is taken through its ``.policy``."""
    policy = model
    if not hasattr(policy, "mlp_extractor") and hasattr(policy, "policy"):
        policy = policy.policy
    if not hasattr(policy, "mlp_extractor"):
        _refuse_ac(f"{type(model).__name__} has no mlp_extractor: not an SB3 ActorCriticPolicy")
    if getattr(policy, "use_sde", False):
        _refuse_ac("use_sde=True (gSDE: a state-dependent noise matrix in place of log_std [3])")
    if getattr(policy, "squash_output", False):
        _refuse_ac("squash_output=True")
    fes = {a: getattr(policy, a, None) for a in ("features_extractor", "pi_features_extractor", "vf_features_extractor")}
    for attr, fe in fes.items():
        if fe is not None and type(fe).__name__ != "FlattenExtractor":
            _refuse_ac(f"{attr} is {type(fe).__name__}; only the MLP policies' FlattenExtractor is supported")
    if not getattr(policy, "share_features_extractor", True):
        pf, vf = fes["pi_features_extractor"], fes["vf_features_extractor"]
        if type(pf) is not type(vf):
            _refuse_ac(f"share_features_extractor=False with differing extractors ({type(pf).__name__}, {type(vf).__name__})")
    ext = policy.mlp_extractor
    pi, pi_acts = _sequential(ext.policy_net)
    vf, vf_acts = _sequential(ext.value_net)
    acts = pi_acts | vf_acts
    if len(acts) != 1:
        _refuse_ac(f"mixed activations {sorted(acts)}")
    for attr in ("action_net", "value_net", "log_std"):
        if not hasattr(policy, attr):
            _refuse_ac(f"the policy has no {attr}")
    if type(policy.action_net).__name__ != "Linear":
        _refuse_ac(f"action_net is {type(policy.action_net).__name__}, not a Linear (DiagGaussianDistribution's mean head)")
    return actor_critic_params(pi, vf, policy.action_net, policy.value_net, policy.log_std, acts.pop(), widths)


def no_value_clip(model):
    """PPO's ``clip_range_vf`` must be None: the kernel's value loss is the plain mse_loss."""
    crv = getattr(model, "clip_range_vf", None)
    if crv is not None:
        _refuse_ac(f"clip_range_vf = {crv!r} (a clipped value loss); clip_range_vf must be None")


def finite(x, what) -> float:
    v = float(x)
    if not v == v or abs(v) == float("inf"):
        raise ValueError(f"{what} must be finite, got {x!r}")
    return v


def ent_coef(log_ent_coef, ent_coef):
    """(the learned [1] tensor or None, the fixed coefficient or 0.0): SAC takes exactly one of the two."""
    if (log_ent_coef is None) == (ent_coef is None):
        _refuse("SAC needs exactly one of log_ent_coef (the learned tensor) and ent_coef (a fixed float)")
    if log_ent_coef is None:
        return None, finite(ent_coef, "ent_coef")
    if not hasattr(log_ent_coef, "numel") or log_ent_coef.numel() != 1:
        _refuse(f"log_ent_coef must be a tensor of one element, got {log_ent_coef!r}")
    return _param(log_ent_coef, "log_ent_coef", tuple(log_ent_coef.shape)), 0.0


def model_ent_coef(model) -> dict:
    """The keyword of an SB3 SAC model's entropy coefficient: ``log_ent_coef`` (ent_coef="auto") or ``ent_coef``."""
    lec = getattr(model, "log_ent_coef", None)
    if lec is not None:
        return dict(log_ent_coef=lec)
    fixed = getattr(model, "ent_coef_tensor", None)
    if fixed is None:
        _refuse("the SAC model has neither log_ent_coef nor ent_coef_tensor")
    return dict(ent_coef=float(fixed))


def check_device(tensors, device, who, what="parameter") -> None:
    """Every bound tensor lives on `device` (a torch.device): the kernels read them through raw pointers."""
    for x in tensors:
        if x.device != device:
            raise ValueError(f"a {what} of shape {tuple(x.shape)} is on {x.device}; {who} binds float32 contiguous CUDA tensors "
                             f"on {device}")
