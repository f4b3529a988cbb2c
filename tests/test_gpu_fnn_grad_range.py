"""GPU: k_fnn_grad / k_fnn_grad_reduce (csrc/meshenv_fnn_grad.h) beyond the near-uniform students of tests/test_gpu_fnn_grad.py,
all against eager float64 within that file's bound (fnn_grad_ref.bounds: 4 eager-float32-against-float64 + 1e-6 max |g64| per
tensor, never made of the kernel):
  (1) confident students: logits with a spread of 63 and of 313, where the row maximum, an underflowing term of lse, the column
      of the one-hot and the argmax of the backward decide the result;
  (2) exact zeros: what eager torch gives as exactly 0 in float32 and float64 the device gives as exactly 0 -- in every
      comparison here, and by name for a student with crafted dead units;
  (3) a deep tile walk: 385 tiles on 128 workgroups, rows that repeat;
  (4) the sampler's rows: angles up to 4.5, targets up to 1.8;
  (5) ties in the backward's argmax on crafted heads, with gradients that are exact;
  (6) fit at batch sizes that leave ragged minibatches.
tests/fnn_grad_ref.py holds the students and tests/test_fnn_grad_cpu.py pins their conditions on the CPU."""
import copy

import numpy as np
import pytest

import fnn_grad_ref as G
import fnn_ref as R
from test_gpu_fnn import CRAFTED

pytestmark = pytest.mark.gpu


def _trainer(key, module=None):
    import torch
    from reinforcementlearning4meshgeneration_amd import FusedFNNTrain
    pol = copy.deepcopy(G.policy(key) if module is None else module).cuda()
    opt = torch.optim.Adam(pol.parameters(), lr=G.LR)
    return pol, opt, FusedFNNTrain(pol, opt)


def _dev(*arrays):
    import torch
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _got(pol, out):
    g = {k: p.grad.detach().cpu().numpy() for k, p in pol.named_parameters()}
    o = out.cpu().numpy()
    g.update(loss=o[0], classification_loss=o[1], regression_loss=o[2], hits=o[3])
    return g


def _fmt(w):
    top = max(w, key=w.get)
    return f"max {w[top]:.4f} ({top})"


def _compare(pol, tr, key, B, gather, worst=None):
    """One backward of student `key` on batch(key, B, gather) against its references: the bound, the exact zeros, hits, and the
    same bits from a second call.  Returns what the device gave."""
    import torch
    x, y, rows = G.batch(key, B, gather)
    want, e32, e64 = G.references(key, B, gather)
    bound = G.bounds(e32, e64)
    xd, yd, rd = _dev(x, y, rows)
    out = tr.backward(xd, yd, rows=rd)
    got = _got(pol, out)
    w = G.ratios(got, e64, bound)
    e32_dev = G.eager(G.policy(key), x if rows is None else x[rows], y if rows is None else y[rows], device="cuda")
    print(f"\nfnn grad student {key} B {B} gather {gather}: |device - fp64| / bound {_fmt(w)}; losses "
          + " ".join(f"{k}={w[k]:.3f}" for k in G.LOSSES) + f"; eager float32 on the device {_fmt(G.ratios(e32_dev, e64, bound))}; "
          f"hits {int(got['hits'])} of {B}")
    if worst is not None:
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), v)
    assert all(got[k].dtype == np.float32 and got[k].shape == np.shape(e64[k]) for k in G.NAMES)
    assert all(np.isfinite(got[k]).all() for k in (*G.NAMES, *G.LOSSES))
    assert max(w.values()) <= 1.0, (B, {k: v for k, v in w.items() if v > 1.0})
    assert not G.zero_violations(got, e32, e64), (B, G.zero_violations(got, e32, e64))
    assert got["hits"] == e64["hits"] == want["hits"]
    kept = [p.grad.clone() for p in pol.parameters()]
    out2 = tr.backward(xd, yd, rows=rd)
    assert torch.equal(out, out2) and all(torch.equal(p.grad, g) for p, g in zip(pol.parameters(), kept)), B
    return got


# --------------------------------------------------------------------------------------------------- (1) confident students
@pytest.mark.parametrize("gather", [False, True])
@pytest.mark.parametrize("key", G.CONFIDENT, ids=str)
def test_confident_students_against_float64(key, gather):
    """Softmax rows that are one-hot to float32 precision, on the predicted class or (for most rows) on a wrong one: ce is the
    logit spread, d_logits is (0, 1, -1)-like, and hits counts rows of two classes.  Measured on the MI355X: DESIGN.md
    section 29."""
    pol, _, tr = _trainer(key)
    worst = {}
    for B in (1, 17, 128, 2065):
        _compare(pol, tr, key, B, gather, worst)
    print(f"\nfnn grad student {key} gather {gather} over all B: worst |device - fp64| / bound {_fmt(worst)} "
          + " ".join(f"{k}={v:.3f}" for k, v in sorted(worst.items())))
    tr.close()


# --------------------------------------------------------------------------------------------------------- (2) exact zeros
@pytest.mark.parametrize("B", [33, 128])
def test_dead_units_give_exact_zeros_by_name(B):
    """Three crafted units in each of fc1 .. fc5 (pre-activations -1, -1 and exactly 0): their weight rows and bias entries and
    the columns they feed in the next layer's weight gradient are exactly 0, and the rest of each such tensor is not."""
    pol, _, tr = _trainer(G.DEAD)
    got = _compare(pol, tr, G.DEAD, B, False)
    for name, idx in G.dead_zero_blocks():
        assert got[name][idx].size and (got[name][idx] == 0).all(), (name, np.flatnonzero(got[name][idx]).tolist())
        assert (got[name] != 0).any(), name
    tr.close()


# ----------------------------------------------------------------------------------------------------------- (3) deep walk
@pytest.mark.parametrize("key", (G.STUDENTS[0], G.CONFIDENT[1]), ids=str)
def test_deep_tile_walk_with_repeating_rows(key):
    """B = 6145: workgroup 0 walks four tiles, every other workgroup three, the last tile has one row; the LDS buffers and the
    register accumulators are reused at depth.  rows holds every index once or twice."""
    import torch
    pol, _, tr = _trainer(key)
    worst = {}
    _compare(pol, tr, key, G.DEEP_B, False, worst)
    _compare(pol, tr, key, G.DEEP_B, True, worst)
    print(f"\nfnn grad student {key} deep walk: worst |device - fp64| / bound {_fmt(worst)}")
    # the gather is the same minibatch as the gathered rows handed over plainly
    x, y, rows = G.batch(key, G.DEEP_B, True)
    assert len(np.unique(rows)) < len(rows) == G.DEEP_B
    xd, yd, rd = _dev(x, y, rows)
    out_rows = tr.backward(xd, yd, rows=rd)
    kept = [p.grad.clone() for p in pol.parameters()]
    out_plain = tr.backward(*_dev(x[rows], y[rows]))
    assert torch.equal(out_rows, out_plain) and all(torch.equal(p.grad, g) for p, g in zip(pol.parameters(), kept))
    tr.close()


# --------------------------------------------------------------------------------------------------------- (4) sampler rows
@pytest.mark.parametrize("gather", [False, True])
@pytest.mark.parametrize("key", G.SAMPLER, ids=str)
def test_sampler_rows_against_float64(key, gather):
    """The data the trainer exists for: six tiles, the last of ten rows; 30 rows of each type, so the near-uniform student's
    one predicted class is hit 30 times."""
    pol, _, tr = _trainer(key)
    got = _compare(pol, tr, key, 90, gather)
    assert got["hits"] == 30
    tr.close()


# ------------------------------------------------------------------------------------------------------------------ (5) ties
TIED = [(bias, want) for bias, want in CRAFTED if np.isfinite(bias).all()]


@pytest.mark.parametrize("bias,want", TIED)
def test_the_backwards_argmax_breaks_ties_as_torch_does(bias, want):
    """Zero trunk and head weights: the logits are type_head.bias on every row, so hits counts the rows of torch.argmax(bias);
    every activation is 0, so the trunk and the head weights get exactly zero gradients; the action is action_head.bias, and
    with dyadic biases and targets its gradient 2 sum(bias - y) is exact in any order."""
    import torch
    assert len(TIED) == 6
    B = 17
    sd = {k: torch.zeros_like(v) for k, v in R.make_policy(0).state_dict().items()}
    sd["type_head.bias"] = torch.tensor(bias, dtype=torch.float32)
    sd["action_head.bias"] = torch.tensor([0.375, -1.25])
    module = R.make_policy(0)
    module.load_state_dict(sd)
    x = R.forward_observations(B)
    y = np.zeros((B, 3), np.float32)
    y[:, 0] = (np.arange(B) % 3) / 2.0
    y[:, 1] = (np.arange(B) % 4) * 0.25
    y[:, 2] = -(np.arange(B) % 5) * 0.5
    pol, _, tr = _trainer(None, module)
    got = _got(pol, tr.backward(*_dev(x, y)))
    assert int(torch.argmax(torch.tensor(bias, dtype=torch.float32))) == want
    assert got["hits"] == int((np.arange(B) % 3 == want).sum())
    for k in G.NAMES:
        if k not in ("action_head.bias", "type_head.bias"):
            assert (got[k] == 0).all(), k
    exact = 2.0 * (np.float64(sd["action_head.bias"].numpy())[None, :] - y[:, 1:].astype(np.float64)).sum(axis=0)
    assert np.array_equal(got["action_head.bias"].astype(np.float64), exact)
    mse = ((np.float64(sd["action_head.bias"].numpy())[None, :] - y[:, 1:].astype(np.float64)) ** 2).sum()
    assert got["regression_loss"] == mse                       # dyadic squares: exact as well
    # the softmax half against eager float64 within the bound (the tensors that are zero on both sides have a zero bound)
    e32, e64 = G.eager(module, x, y), G.eager(module, x, y, double=True)
    assert e32["hits"] == e64["hits"] == got["hits"]
    bound = G.bounds(e32, e64)
    w = {k: v for k, v in G.ratios(got, e64, bound).items() if bound[k] > 0}
    print(f"\nfnn grad crafted bias {bias}: hits {int(got['hits'])}, |device - fp64| / bound {_fmt(w)}")
    assert set(w) >= {"type_head.bias", "loss", "classification_loss"} and max(w.values()) <= 1.0
    assert not G.zero_violations(got, e32, e64)
    tr.close()


# ------------------------------------------------------------------------------------------------------------------- (6) fit
@pytest.mark.parametrize("batch_size,per_epoch", [(1, 37), (16, 3), (64, 1)])
def test_fit_at_ragged_batch_sizes(batch_size, per_epoch):
    """N = 37, two epochs: 37 minibatches of one row; 16 + 16 + 5; one minibatch shorter than batch_size."""
    import torch
    from reinforcementlearning4meshgeneration_amd.fnn_train import FNNTrainSpec
    seed, N, E = G.STUDENTS[0], 37, 2
    x, y = (a[:N] for a in G.decided_pool(seed))
    xd, yd = _dev(x, y)
    perms = FNNTrainSpec.permutations(N, E, seed=0)
    batches = FNNTrainSpec.minibatches(N, batch_size)
    assert len(batches) == per_epoch and batches[-1][1] == N
    pol_a, opt_a, tr_a = _trainer(seed)
    log_a = tr_a.fit(xd, yd, E, batch_size=batch_size, seed=0)
    pol_b, opt_b, tr_b = _trainer(seed)
    pd = _dev(perms)[0]
    log_b = torch.zeros((E, 4), device="cuda")
    for e in range(E):
        for a, b in batches:
            tr_b.backward(xd, yd, rows=pd[e, a:b], accum=log_b[e])
            tr_b.step()
    assert torch.equal(log_a.sums, log_b)
    for pa, pb in zip(pol_a.parameters(), pol_b.parameters()):
        assert torch.equal(pa, pb)
        sa, sb = opt_a.state[pa], opt_b.state[pb]
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"])
        assert float(sa["step"]) == float(sb["step"]) == float(E * per_epoch)
    logs = []
    for dt in (torch.float32, torch.float64):
        pe = copy.deepcopy(R.make_policy(seed)).to(dt)
        logs.append(G.eager_fit(pe, torch.optim.Adam(pe.parameters(), lr=G.LR), x, y, perms, batch_size))
    dev = log_a.read().astype(np.float64)
    worst = 0.0
    for col, name in enumerate(G.LOSSES):
        l32, l64 = logs[0][:, col], logs[1][:, col]
        d32 = float(np.abs(l32 - l64).max())
        tol = 4 * d32 + 1e-6 * float(np.abs(l64).max())
        off = float(np.abs(dev[:, col] - l64).max())
        worst = max(worst, off / tol)
        print(f"\nfnn fit batch_size {batch_size} {name}: device {dev[:, col].tolist()} fp64 {l64.tolist()}; d32 {d32:.3g}, "
              f"|device - fp64| {off:.3g} of {tol:.3g} allowed")
        assert name != "loss" or off <= tol      # the loss is held to it, as in tests/test_gpu_fnn_grad.py; its halves are shown
    print(f"fnn fit batch_size {batch_size}: worst |device - fp64| / allowed {worst:.4f}; hits {dev[:, 3].tolist()}")
    assert (dev[:, 3] <= N).all() and (dev[:, 3] >= 0).all()
    tr_a.close()
    tr_b.close()
