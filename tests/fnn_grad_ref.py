"""Host side of the FNN-training tests (tests/test_fnn_grad_cpu.py, tests/test_gpu_fnn_grad.py): the statement of
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
POOL = 4101                     # rows of the shared data
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


# ------------------------------------------------------------------------------------------------------------ the ReLU condition
@functools.lru_cache(maxsize=None)
def undecided(seed, n=POOL):
    """bool [n]: rows of data(n) on which some hidden pre-activation of make_policy(seed) has |z64| <= 8 max |z32 - z64| of its
    layer: float32 and float64 may disagree about its ReLU mask, and a gradient compared across them says nothing there."""
    import torch
    x, _ = data(n)
    pol = R.make_policy(seed)
    P64 = params64(pol)
    z64, _ = pre_activations(P64, x.astype(np.float64))
    with torch.no_grad():
        h, z32 = torch.from_numpy(x), []
        for name, _, _ in R.LAYERS[:5]:
            z = getattr(pol, name)(h)
            z32.append(z.numpy().astype(np.float64))
            h = torch.relu(z)
    bad = np.zeros(n, bool)
    for a, b in zip(z32, z64):
        bad |= (np.abs(b) <= 8 * np.abs(a - b).max()).any(axis=1)
    return bad


@functools.lru_cache(maxsize=None)
def decided_pool(seed):
    """(x, y) of data() without the undecided rows of make_policy(seed): what every batch of that student is cut from."""
    x, y = data()
    keep = ~undecided(seed)
    return np.ascontiguousarray(x[keep]), np.ascontiguousarray(y[keep])


def batch(seed, B, gather=False):
    """(x, y, rows) for student `seed`: the first B decided rows (rows None), or the whole decided pool with rows = B distinct
    shuffled indices into it."""
    x, y = decided_pool(seed)
    assert B <= len(x)
    if not gather:
        return x[:B].copy(), y[:B].copy(), None
    rows = np.random.default_rng(1000 + B).permutation(len(x))[:B].astype(np.int32)
    return x, y, rows


@functools.lru_cache(maxsize=None)
def references(seed, B, gather=False):
    """(fp64 restatement, eager float32, eager float64) of student `seed` on batch(seed, B, gather): computed once."""
    x, y, rows = batch(seed, B, gather)
    if rows is not None:
        x, y = x[rows], y[rows]
    pol = R.make_policy(seed)
    return restated(params64(pol), x, y), eager(pol, x, y), eager(pol, x, y, double=True)


def bounds(g32, g64):
    """Per name the distance from float64 the device may have: 4 max |g32 - g64| + 1e-6 max |g64| (section 28's factor and
    floor, the floor scaled by the tensor because a summed loss grows with B)."""
    return {k: 4 * float(np.abs(np.asarray(g32[k]) - np.asarray(g64[k])).max()) + 1e-6 * float(np.abs(np.asarray(g64[k])).max())
            for k in (*NAMES, *LOSSES)}


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
