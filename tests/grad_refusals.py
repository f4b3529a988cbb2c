"""What the entry points of the loss-gradient handles (critic, SAC actor, TD3 actor, DDPG, PPO / A2C, FNN) refuse, and in
which words: the texts of *_last_error, transcribed from csrc/meshenv_hip.hip as the six families stood when each bind wrote
its own checks.  tests/test_grad_bind_cpu.py holds csrc/meshenv_grad_bind.h to them on the host,
tests/test_gpu_grad_refusals.py the entry points themselves."""

KINDS = ("supported kinds: 0 (SAC: twin ReLU [128, 128, 128] critics) or 1 (TD3: twin ReLU [256, 256] critics); "
         "input cat(obs, action) = 21, float32")
FNN_SHAPES = ("supported network: fc1 [64][18], fc2 [128][64], fc3 [64][128], fc4 [32][64], fc5 [16][32], action_head "
              "[2][16], type_head [3][16], each with a bias of its rows (general/EBRD.py Policy)")
PPO_SHAPES = ("supported: pi and vf towers of two hidden layers of the same width 64 or 128, activation 0 (ReLU) or 1 "
              "(Tanh), action_net [3], value_net [1], log_std [3], 18 observations, float32")
PPO_TAKES = "takes 13 tensors: pi w1 b1 w2 b2 wh bh, vf w1 b1 w2 b2 wh bh, log_std"
WEIGHT = "weight tensor {i} is not 16-byte aligned"


def inner_weights(count):
    """The rule of five of the six binds: every weight behind the first layer's, i.e. the even indices >= 2."""
    return tuple(i for i in range(count) if i % 2 == 0 and i >= 2)


def _net(count, null, align, aligned=None):
    return dict(count=count, null=null, align=align, aligned=inner_weights(count) if aligned is None else aligned)


# key -> the bind: fn (the entry point), row (its description in csrc/meshenv_grad_bind.h), n_grad (floats of the gradient
# buffer), nets (the tensor arrays in argument order: count, the refusal of a null tensor, of a misaligned one, the indices
# read 16 bytes at a time), takes (the refusal of a null array or a wrong count), size (of a null or wrongly sized buffer)
BINDS = {
    "critic-sac": dict(
        fn="meshenv_critic_grad_bind", row="kCriticGradBind[0]", n_grad=72064,
        nets=[_net(8, "null critic tensor", WEIGHT)] * 2,
        takes="kind 0 takes 8 tensors per critic; " + KINDS,
        size="the gradient buffer of kind 0 has 72064 floats, got {got}"),
    "critic-td3": dict(
        fn="meshenv_critic_grad_bind", row="kCriticGradBind[1]", n_grad=143488,
        nets=[_net(6, "null critic tensor", WEIGHT)] * 2,
        takes="kind 1 takes 6 tensors per critic; " + KINDS,
        size="the gradient buffer of kind 1 has 143488 floats, got {got}"),
    "actor": dict(
        fn="meshenv_actor_grad_bind", row="kActorGradBind", n_grad=36288,
        nets=[_net(10, "null actor tensor", "actor " + WEIGHT)] + [_net(8, "null critic tensor", "critic " + WEIGHT)] * 2,
        takes="takes 10 actor tensors and 8 tensors per critic (SAC: actor ReLU [128, 128, 128] with mu / log_std heads, twin "
              "ReLU [128, 128, 128] critics, float32)",
        size="the gradient buffer has 36288 floats, got {got}"),
    "td3-actor": dict(
        fn="meshenv_td3_actor_grad_bind", row="kTd3ActorGradBind", n_grad=71488,
        nets=[_net(6, "null tensor", WEIGHT)] * 2,
        takes="takes 6 actor tensors and 6 tensors of the first critic (TD3 / DDPG: actor ReLU [256, 256] with a Linear(256, 3) "
              "+ Tanh head, critic ReLU [256, 256], float32)",
        size="the gradient buffer has 71488 floats, got {got}"),
    "ddpg": dict(
        fn="meshenv_ddpg_grad_bind", row="kDdpgGradBind", n_grad=258240,
        nets=[_net(6, "null tensor", WEIGHT)] * 2,
        takes="takes 6 actor tensors and 6 tensors of the critic (DDPG: actor ReLU [400, 300] with a Linear(300, 3) + Tanh head, "
              "critic ReLU [400, 300], float32)",
        size="the gradient buffer has 258240 floats, got {got}",
        grad_off2="the gradient buffer is not 4-byte aligned"),
    "ppo-64": dict(
        fn="meshenv_ppo_grad_bind", row="kPpoGradBind[0]", n_grad=11072,
        nets=[_net(13, "null tensor", WEIGHT, aligned=(2, 4, 8, 10))], takes=PPO_TAKES,
        size="the gradient buffer has 11072 floats at width 64, got {got}"),
    "ppo-128": dict(
        fn="meshenv_ppo_grad_bind", row="kPpoGradBind[1]", n_grad=38464,
        nets=[_net(13, "null tensor", WEIGHT, aligned=(2, 4, 8, 10))], takes=PPO_TAKES,
        size="the gradient buffer has 38464 floats at width 128, got {got}"),
    "fnn": dict(
        fn="meshenv_fnn_grad_bind", row="kFnnGradBind", n_grad=20544,
        nets=[_net(14, "null tensor", WEIGHT)], takes="takes 14 tensors; " + FNN_SHAPES,
        size="the gradient buffer has 20544 floats, got {got}"),
}

# in front of meshenv_ppo_grad_bind's count check, in the entry point itself
PPO_BIND_WIDTH_256 = ("meshenv_ppo_grad_bind: width 256 is not supported (its dW_2 needs the column split of the TD3 critic kernel); "
                      + PPO_SHAPES)
PPO_BIND_SHAPE = "meshenv_ppo_grad_bind: unsupported shape; " + PPO_SHAPES


def bind_cases(key):
    """[(case, text)] of one bind, in the order tests/test_grad_bind_cpu.py's program prints them: text is the whole refusal,
    '' where the call is accepted.  A case is a tuple: ("good",), ("null_array", net), ("count", net, delta), ("n_grad", got),
    ("null_grad",), ("null_tensor", net, i), ("off4", net, i) (4 bytes added to tensor i), ("grad_off2",) (2 bytes added to
    grad_dev)."""
    b = BINDS[key]
    say = lambda text: f"{b['fn']}: {text}" if text else ""   # noqa: E731
    nets = range(len(b["nets"]))
    out = [(("good",), "")]
    out += [(("null_array", k), say(b["takes"])) for k in nets]
    out += [(("count", k, d), say(b["takes"])) for k in nets for d in (-1, 1)]
    out += [(("n_grad", got), say(b["size"].format(got=got))) for got in (b["n_grad"] - 1, b["n_grad"] + 1, 0)]
    out += [(("null_grad",), say(b["size"].format(got=b["n_grad"])))]
    out += [(("null_tensor", k, i), say(net["null"])) for k, net in enumerate(b["nets"]) for i in range(net["count"])]
    out += [(("off4", k, i), say(net["align"].format(i=i)) if i in net["aligned"] else "")
            for k, net in enumerate(b["nets"]) for i in range(net["count"])]
    out += [(("grad_off2",), say(b.get("grad_off2", "")))]
    return out


# ---- the backward calls: family -> what each refusal says behind "<fn>: "
BACKWARD = {
    "critic": dict(
        fn="meshenv_critic_grad_backward", state="no tensors bound (meshenv_critic_grad_bind)",
        required="n > 0, obs_dev, actions_dev, target_dev and loss_dev are required",
        pair="acts1_dev and acts2_dev go together", acts="null activation output"),
    "actor": dict(
        fn="meshenv_actor_grad_backward", state="no tensors bound (meshenv_actor_grad_bind)",
        required="n > 0, obs_dev and losses_dev are required", exclusive="noise_dev and sample are exclusive",
        eps="eps_out_dev needs noise_dev or sample", parts="null per-sample output", acts="null activation output"),
    "td3-actor": dict(
        fn="meshenv_td3_actor_grad_backward", state="no tensors bound (meshenv_td3_actor_grad_bind)",
        required="0 < n <= 2^24 - 16, obs_dev and loss_dev are required", parts="null per-sample output",
        acts="null activation output"),
    "ppo": dict(
        fn="meshenv_ppo_grad_backward", state="no tensors bound (meshenv_ppo_grad_bind)",
        required="0 < n <= 2^24 - 16 and obs, actions, advantages, returns and out are required",
        old="PPO's loss needs old_log_prob_dev",
        coefficients="clip_range and max_grad_norm must be finite and > 0, ent_coef and vf_coef finite",
        parts="null per-row output", acts="null activation output"),
    "fnn": dict(
        fn="meshenv_fnn_grad_backward", state="no tensors bound (meshenv_fnn_grad_bind)",
        required="0 < n, N <= 2^24, n <= N without rows_dev, and x, y and out are required"),
}


def backward_text(family, what):
    b = BACKWARD[family]
    return f"{b['fn']}: {b[what]}"
