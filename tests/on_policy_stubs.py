"""SB3-2.x-shaped PPO / A2C models for the tests of the on-policy optimiser step and the rollout buffer (stable_baselines3 is
not in the image): ``.policy`` is an ActorCriticPolicy stand-in (``mlp_extractor.policy_net / value_net``, ``action_net``,
``value_net``, ``log_std``, ``optimizer``) built from tests/ppo_grad_ref.py's modules, with the reference's two recipes:
PPO ReLU [128, 128] with Adam(lr=3e-4, eps=1e-5) and SB3's default A2C, Tanh [64, 64] with RMSprop(lr=7e-4, alpha=0.99,
eps=1e-5)."""
import types

import ppo_grad_ref as P

RECIPES = {"ppo": "ppo-relu128", "a2c": "a2c-tanh64"}


def policy(kind, device="cpu", seed=11, optimizer=None):
    """(the ActorCriticPolicy stand-in, its 13 parameters in FusedPPOGrad's bind order)."""
    import torch
    m = P.modules(RECIPES[kind], seed=seed)
    act = torch.nn.Tanh if m["act"] == "tanh" else torch.nn.ReLU
    seq = lambda ls: torch.nn.Sequential(ls[0], act(), ls[1], act()).to(device)   # noqa: E731
    fe = type("FlattenExtractor", (torch.nn.Module,), {})()
    pol = types.SimpleNamespace(mlp_extractor=types.SimpleNamespace(policy_net=seq(m["pi"]), value_net=seq(m["vf"])),
                                action_net=m["action_net"].to(device), value_net=m["value_net"].to(device),
                                log_std=torch.nn.Parameter(m["log_std"].detach().clone().to(device)), use_sde=False, squash_output=False,
                                features_extractor=fe, pi_features_extractor=fe, vf_features_extractor=fe, share_features_extractor=True)
    params = [p for mod in (pol.mlp_extractor.policy_net, pol.action_net, pol.mlp_extractor.value_net, pol.value_net)
              for p in mod.parameters()] + [pol.log_std]
    if optimizer is None:
        optimizer = "rmsprop" if kind == "a2c" else "adam"
    pol.optimizer = (torch.optim.RMSprop(params, lr=7e-4, alpha=0.99, eps=1e-5) if optimizer == "rmsprop" else
                     torch.optim.Adam(params, lr=3e-4, eps=1e-5))
    return pol, params


def model(kind, device="cpu", seed=11, optimizer=None):
    """An SB3-shaped PPO / A2C model around policy(kind): the hyper-parameters PPO.train / A2C.train read."""
    pol, params = policy(kind, device, seed, optimizer)
    a2c = kind == "a2c"
    return types.SimpleNamespace(policy=pol, gamma=0.99, gae_lambda=1.0 if a2c else 0.95, clip_range=None if a2c else (lambda _: 0.2),
                                 clip_range_vf=None, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, normalize_advantage=not a2c,
                                 n_epochs=1 if a2c else 2, batch_size=None if a2c else 16, target_kl=None,
                                 _current_progress_remaining=1.0), params
