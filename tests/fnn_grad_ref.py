"""Host side of the FNN-training tests (tests/test_fnn_grad_cpu.py, tests/test_gpu_fnn_grad.py,
tests/test_gpu_fnn_grad_range.py): the statement of
general/EBRD.py's train_ch3 (:272-320) for one minibatch,

    action, logits = model(x)
    loss = CrossEntropyLoss(reduction='sum')(logits, cls) + MSELoss(reduction='sum')(action, y[:, 1:])

restated in float64 numpy with its fourteen gradients, the eager module in float32 and float64 (the yardstick of every
tolerance here: eager float32 against float64, never the kernel), the shared data, the ReLU condition, and the eager loops the
fit test compares with.  Nothing here needs a GPU."""
import copy
import functools

import numpy as np

import fnn_ref as R

NAMES = tuple(f"{name}.{part}" for name, _, _ in R.LAYERS for part in ("weight", "bias"))
LOSSES = ("loss", "classification_loss", "regression_loss")
TEACHER = (12, 40.0)            # fnn_ref.forward_policy: its fp64 argmax is 1 or 2 on every row
STUDENTS = (11, 6)              # fnn_ref.make_policy seeds
# A student KEY names the net and the rows every helper below works on (policy, rows_of):
#   seed                 fnn_ref.make_policy(seed) on data(): near-uniform softmax, logits in [-0.153, 0.099]
#   (seed, type_scale)   fnn_ref.forward_policy(seed, type_scale) on data(): the same trunk, type_head.weight scaled
#   ("dead", seed)       make_policy(seed) with crafted units in fc1 .. fc5 (dead_policy) on data()
#   ("sampler", seed)    make_policy(seed) on sampler_rows()
# CONFIDENT: logits in [-25, 39] with a spread up to 63.5 (the fp64 argmax is class 0 on every row), and in [-194, 121] with a
# spread up to 313 (classes 1 / 2 on 332 / 3769 rows): a softmax without the row maximum overflows float32 on the second
# (exp(121)) and not on the first, and exp(l - m) underflows to 0 on the second (exp(-313)).
# forward_policy(12, s) is no student: it shares the teacher's trunk, its regression loss is 3e-17 and the yardstick collapses.
CONFIDENT = ((11, 400.0), (6, 4000.0))
DEAD = ("dead", 11)
SAMPLER = (("sampler", 11), ("sampler", 6))
POOL = 4101                     # rows of the shared data
DEEP_B = 6145                   # 385 tiles on 128 workgroups: workgroup 0 walks four, the others three; the last tile has one row
GPU_BS = (1, 15, 16, 17, 33, 128, 2065)   # 2065: 130 tiles on at most 128 workgroups, so two of them walk two tiles; the last tile has one row
UNDECIDED_CAP = 0.01
LR = 1e-3


# ------------------------------------------------------------------------------------------------------------ the data
@functools.lru_cache(maxsize=None)
def data(n=POOL):
    """x [n, 18] = forward_observations(n) (zero rows included); y [n, 3] = (type, out0, out1): the teacher's float32 actions and
    argmax(logits) / 2, every fifth row's class set to 0 (the teacher never picks it)."""
    x = R.forward_observations(n)
    a, l = R.eager(R.forward_policy(*TEACHER), x)
    cls = l.argmax(axis=1)
    cls[::5] = 0
    y = np.concatenate([cls[:, None].astype(np.float32) / 2, a.astype(np.float32)], axis=1)
    return x, np.ascontiguousarray(y, dtype=np.float32)


def params64(policy):
    return {k: v.detach().cpu().numpy().astype(np.float64) for k, v in policy.state_dict().items()}


# ------------------------------------------------------------------------------------------------------------ fp64 numpy
def pre_activations(P, x):
    """[z_1 .. z_5] and [a_0 .. a_5] of the five hidden layers, in P's dtype."""
    h, zs, hs = x.astype(P["fc1.weight"].dtype), [], []
    hs.append(h)
    for name, _, _ in R.LAYERS[:5]:
        z = h @ P[f"{name}.weight"].T + P[f"{name}.bias"]
        h = np.maximum(z, 0)
        zs.append(z)
        hs.append(h)
    return zs, hs


def restated(P, x, y):
    """The loss and its gradients in float64 numpy: dict of the 14 gradients (NAMES), the three LOSSES, 'hits'."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    n = len(x)
    cls = np.rint(2 * y[:, 0]).astype(np.int64)
    zs, hs = pre_activations(P, x)
    action = hs[5] @ P["action_head.weight"].T + P["action_head.bias"]
    logits = hs[5] @ P["type_head.weight"].T + P["type_head.bias"]
    m = logits.max(axis=1, keepdims=True)
    logp = (logits - m) - np.log(np.exp(logits - m).sum(axis=1, keepdims=True))
    ce = -logp[np.arange(n), cls].sum()
    diff = action - y[:, 1:]
    mse = (diff * diff).sum()
    dl = np.exp(logp)
    dl[np.arange(n), cls] -= 1.0
    da = 2.0 * diff
    g = {"action_head.weight": da.T @ hs[5], "action_head.bias": da.sum(axis=0),
         "type_head.weight": dl.T @ hs[5], "type_head.bias": dl.sum(axis=0)}
    dh = da @ P["action_head.weight"] + dl @ P["type_head.weight"]
    for i in range(4, -1, -1):
        name = R.LAYERS[i][0]
        dz = dh * (zs[i] > 0)
        g[f"{name}.weight"], g[f"{name}.bias"] = dz.T @ hs[i], dz.sum(axis=0)
        dh = dz @ P[f"{name}.weight"]
    g.update(loss=ce + mse, classification_loss=ce, regression_loss=mse, hits=int((logits.argmax(axis=1) == cls).sum()))
    return g


# ------------------------------------------------------------------------------------------------------------ eager torch
def torch_loss(model, x, y):
    import torch
    action, logits = model(x)
    cls = (2 * y[:, 0]).round().long()
    ce = torch.nn.CrossEntropyLoss(reduction="sum")(logits, cls)
    mse = torch.nn.MSELoss(reduction="sum")(action, y[:, 1:])
    return ce + mse, ce, mse, logits


def eager(policy, x, y, double=False, device="cpu"):
    """Autograd on a copy of the module: the same dict as restated(), as float64 numpy arrays."""
    import torch
    dt = torch.float64 if double else torch.float32
    model = copy.deepcopy(policy).to(device=device, dtype=dt)
    xt, yt = torch.as_tensor(x).to(device=device, dtype=dt), torch.as_tensor(y).to(device=device, dtype=dt)
    loss, ce, mse, logits = torch_loss(model, xt, yt)
    loss.backward()
    g = {k: p.grad.detach().cpu().numpy().astype(np.float64) for k, p in model.named_parameters()}
    cls = (2 * yt[:, 0]).round().long()
    g.update(loss=float(loss.detach()), classification_loss=float(ce.detach()), regression_loss=float(mse.detach()),
             hits=int((logits.argmax(dim=1) == cls).sum()))
    return g


# ------------------------------------------------------------------------------------------------------------ students, conditions
def crafted_units(out):
    """Per hidden layer of `out` units: (units with a zero weight row and bias -1, the unit with a zero weight row and bias 0)."""
    return (0, out - 1), 1


def dead_policy(seed):
    """make_policy(seed) in which, for each of fc1 .. fc5, units 0 and out - 1 have a zero weight row and bias -1 (dead on every
    row) and unit 1 a zero weight row and bias 0: its pre-activation is exactly 0, where relu' is 0 in torch."""
    import torch
    p = R.make_policy(seed)
    with torch.no_grad():
        for name, out, _ in R.LAYERS[:5]:
            fc, (minus, zero) = getattr(p, name), crafted_units(out)
            for u in (*minus, zero):
                fc.weight[u].zero_()
                fc.bias[u] = 0.0 if u == zero else -1.0
    return p


def dead_zero_blocks():
    """[(gradient name, index)] of what dead_policy's crafted units make exactly zero: their weight rows and bias entries
    (relu' is 0 at -1 and at 0) and, their activation being 0, the matching columns of the next layer's weight gradient --
    fc5's in both heads."""
    blocks = []
    for i, (name, out, _) in enumerate(R.LAYERS[:5]):
        minus, zero = crafted_units(out)
        units = [*minus, zero]
        blocks += [(f"{name}.weight", (units, slice(None))), (f"{name}.bias", (units,))]
        for nxt in ([R.LAYERS[i + 1][0]] if i < 4 else ["action_head", "type_head"]):
            blocks.append((f"{nxt}.weight", (slice(None), units)))
    return blocks


def policy(key):
    """The eager module of a student key (STUDENTS' comment)."""
    if isinstance(key, tuple) and key[0] == "dead":
        return dead_policy(key[1])
    if isinstance(key, tuple) and key[0] == "sampler":
        return R.make_policy(key[1])
    if isinstance(key, tuple):
        return R.forward_policy(*key)
    return R.make_policy(key)


@functools.lru_cache(maxsize=None)
def sampler_rows():
    """(x [90, 18], y [90, 3]) float32: the data the trainer exists for.  Of the reference's recorded candidates
    (tests/golden/quality_augment_scores.npz) the rows accepted at threshold 0.7 and the extra_* rows: 30 per type, x in
    [-1.57, 4.51], targets in [0.04, 1.82]."""
    import os
    z = np.load(os.path.join(R.GOLDEN_DIR, "quality_augment_scores.npz"))
    at = int(np.flatnonzero(z["thresholds"] == 0.7)[0])
    keep = z["accept"][:, at]
    x = np.concatenate([z["prop_obs"][z["prop"]][keep], z["extra_obs"]]).astype(np.float32)
    y = np.concatenate([z["act"][keep], z["extra_act"]]).astype(np.float32)
    return np.ascontiguousarray(x), np.ascontiguousarray(y)


def rows_of(key, n=POOL):
    """(x, y) a student key works on."""
    return sampler_rows() if isinstance(key, tuple) and key[0] == "sampler" else data(n)


@functools.lru_cache(maxsize=None)
def relu_undecided(key, n=POOL):
    """bool [rows]: rows of rows_of(key, n) on which some hidden pre-activation of policy(key) has |z64| <= 8 max |z32 - z64| of
    its layer: float32 and float64 may disagree about its ReLU mask, and a gradient compared across them says nothing there.
    A unit whose pre-activation is identical in float32 and float64 on every row (dead_policy's) is decided whatever its value:
    it is left out, or the unit at exactly 0 would flag every row."""
    import torch
    x, _ = rows_of(key, n)
    pol = policy(key)
    P64 = params64(pol)
    z64, _ = pre_activations(P64, x.astype(np.float64))
    with torch.no_grad():
        h, z32 = torch.from_numpy(x), []
        for name, _, _ in R.LAYERS[:5]:
            z = getattr(pol, name)(h)
            z32.append(z.numpy().astype(np.float64))
            h = torch.relu(z)
    bad = np.zeros(len(x), bool)
    for a, b in zip(z32, z64):
        exact = (a == b).all(axis=0)
        bad |= ((np.abs(b) <= 8 * np.abs(a - b).max()) & ~exact).any(axis=1)
    return bad


@functools.lru_cache(maxsize=None)
def margin_undecided(key, n=POOL):
    """bool [rows]: rows whose fp64 top-two logit margin is <= 8 max |l32 - l64|: float32 and float64 may disagree about the
    argmax, and `hits` compared across them says nothing there."""
    x, _ = rows_of(key, n)
    pol = policy(key)
    _, l32 = R.eager(pol, x)
    _, l64 = R.eager(pol, x, double=True)
    top = np.sort(l64, axis=1)
    return top[:, 2] - top[:, 1] <= 8 * float(np.abs(l32 - l64).max())


def undecided(key, n=POOL):
    """bool [rows]: the rows left out of every batch of student `key`.  The ReLU condition; for the keyed students (tuples) the
    hits condition as well.  The plain seeds keep the rows they had: their hits are pinned batch by batch
    (tests/test_fnn_grad_cpu.py)."""
    bad = relu_undecided(key, n)
    return bad | margin_undecided(key, n) if isinstance(key, tuple) else bad


@functools.lru_cache(maxsize=None)
def decided_pool(key):
    """(x, y) of rows_of(key) without the undecided rows of policy(key): what every batch of that student is cut from."""
    x, y = rows_of(key)
    keep = ~undecided(key)
    return np.ascontiguousarray(x[keep]), np.ascontiguousarray(y[keep])


def batch(key, B, gather=False):
    """(x, y, rows) for student `key`: the first B decided rows (rows None), or the whole decided pool with rows = B distinct
    shuffled indices into it.  B past the pool (DEEP_B): the pool cycled to B rows, or rows a shuffled order of the pool cycled
    to B entries -- indices that repeat, into the un-cycled pool."""
    x, y = decided_pool(key)
    if not gather:
        if B > len(x):
            return np.resize(x, (B, x.shape[1])), np.resize(y, (B, y.shape[1])), None
        return x[:B].copy(), y[:B].copy(), None
    perm = np.random.default_rng(1000 + B).permutation(len(x))
    rows = (np.resize(perm, B) if B > len(x) else perm[:B]).astype(np.int32)
    return x, y, rows


@functools.lru_cache(maxsize=None)
def references(key, B, gather=False):
    """(fp64 restatement, eager float32, eager float64) of student `key` on batch(key, B, gather): computed once."""
    x, y, rows = batch(key, B, gather)
    if rows is not None:
        x, y = x[rows], y[rows]
    pol = policy(key)
    return restated(params64(pol), x, y), eager(pol, x, y), eager(pol, x, y, double=True)


def exact_zeros(g32, g64):
    """Per gradient name the bool mask of the elements that are exactly 0 in eager float32 AND in eager float64 (a unit dead on
    the whole batch, a column fed by one): there the device's value must be exactly 0 too, whatever the tensor's bound."""
    return {k: (np.asarray(g32[k]) == 0) & (np.asarray(g64[k]) == 0) for k in NAMES}


def bounds(g32, g64):
    """Per name the distance from float64 the device may have: 4 max |g32 - g64| + 1e-6 max |g64| (section 28's factor and
    floor, the floor scaled by the tensor because a summed loss grows with B)."""
    return {k: 4 * float(np.abs(np.asarray(g32[k]) - np.asarray(g64[k])).max()) + 1e-6 * float(np.abs(np.asarray(g64[k])).max())
            for k in (*NAMES, *LOSSES)}


def zero_violations(got, g32, g64):
    """{name: count} of the elements exact_zeros() names at which `got` is not exactly 0 (-0 counts as 0); empty when none."""
    bad = {k: int((np.asarray(got[k])[m] != 0).sum()) for k, m in exact_zeros(g32, g64).items()}
    return {k: v for k, v in bad.items() if v}


def ratios(got, g64, bound):
    """Per name max |got - g64| / bound."""
    return {k: float(np.abs(np.asarray(got[k], np.float64) - np.asarray(g64[k])).max()) / max(bound[k], 1e-300) for k in bound}


# ------------------------------------------------------------------------------------------------------------ the loop of train_ch3
def eager_fit(policy, optimizer, x, y, perms, batch_size):
    """train_ch3 on `policy` IN PLACE with eager torch, in the dtype and on the device of the module: per epoch the orders
    perms[e], minibatches of batch_size (the last one short).  Returns [E, 3] float64: the sums of loss, ce, mse per epoch."""
    import torch
    p0 = next(policy.parameters())
    xt = torch.as_tensor(x).to(device=p0.device, dtype=p0.dtype)
    yt = torch.as_tensor(y).to(device=p0.device, dtype=p0.dtype)
    log = np.zeros((len(perms), 3))
    for e, perm in enumerate(perms):
        idx = torch.as_tensor(np.asarray(perm, np.int64)).to(p0.device)
        for a in range(0, len(perm), batch_size):
            rows = idx[a:a + batch_size]
            loss, ce, mse, _ = torch_loss(policy, xt[rows], yt[rows])
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            log[e] += (float(loss.detach()), float(ce.detach()), float(mse.detach()))
    return log
