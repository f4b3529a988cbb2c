"""GPU: training the supervised FNN (include/meshenv_fnn_train.h; csrc/meshenv_fnn_grad.h: k_fnn_grad, k_fnn_grad_reduce;
k_optim_step; k_target_pack through meshenv_fnn_refresh):
  (a) the fourteen gradients and the three losses against float64, within a bound made of eager torch float32 against float64
      on the same rows (never of the kernel): 4 err_torch + 1e-6 max |g64| per tensor, and exactly 0 wherever eager float32 and
      float64 both give exactly 0; determinism, rows past B, accum, hits (tests/test_gpu_fnn_grad_range.py: confident and
      dead-unit students, a deep tile walk, the sampler's rows, ties, ragged fit);
  (b) one backward + step against eager float32 + a stock Adam step, within twice the one-step bound of tests/ppo_grad_ref.py;
  (c) refresh() against a freshly packed FusedFNN, bit for bit;
  (d) fit against the hand loop (bits), against eager float64 (the measured float32 distance), and mesh_with afterwards.
tests/fnn_grad_ref.py holds the data, the references and the ReLU condition tests/test_fnn_grad_cpu.py pinned on the CPU."""
import copy

import numpy as np
import pytest

import fnn_grad_ref as G
import fnn_ref as R
import ppo_grad_ref as P

pytestmark = pytest.mark.gpu

G_PARAMS = 20485      # floats of the fourteen gradients; the flat buffer is padded to 20 544


def _trainer(seed, with_fnn=False):
    import torch
    from reinforcementlearning4meshgeneration_amd import FusedFNN, FusedFNNTrain
    pol = copy.deepcopy(R.make_policy(seed)).cuda()
    opt = torch.optim.Adam(pol.parameters(), lr=G.LR)
    fnn = FusedFNN.from_module(pol) if with_fnn else None
    return pol, opt, FusedFNNTrain(pol, opt, fnn=fnn), fnn


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


# ----------------------------------------------------------------------------------------------------------- (a) the gradient
@pytest.mark.parametrize("gather", [False, True])
@pytest.mark.parametrize("seed", G.STUDENTS)
def test_gradients_and_losses_against_float64(seed, gather):
    """B: one row; both sides of the 16-row tile; a one-row second tile; three tiles; the reference's batch; 2065 = 130 tiles
    on 128 workgroups with a last tile of one row.  gather: the rows come shuffled out of the larger decided pool.
    Measured on the MI355X: DESIGN.md section 29."""
    import torch
    pol, _, tr, _ = _trainer(seed)
    worst = {}
    for B in G.GPU_BS:
        x, y, rows = G.batch(seed, B, gather)
        want, e32, e64 = G.references(seed, B, gather)
        bound = G.bounds(e32, e64)
        xd, yd, rd = _dev(x, y, rows)
        out = tr.backward(xd, yd, rows=rd)
        assert out.shape == (4,) and out.dtype == torch.float32 and out.is_cuda
        got = _got(pol, out)
        w = G.ratios(got, e64, bound)
        print(f"\nfnn grad student {seed} B {B} gather {gather}: |device - fp64| / bound {_fmt(w)}; "
              f"restatement against eager fp64 {_fmt(G.ratios(want, e64, bound))}")
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), v)
        assert all(got[k].dtype == np.float32 and got[k].shape == np.shape(e64[k]) for k in G.NAMES)
        assert max(w.values()) <= 1.0, (B, {k: v for k, v in w.items() if v > 1.0})
        assert not G.zero_violations(got, e32, e64), (B, G.zero_violations(got, e32, e64))   # exact zeros of eager stay exact zeros
        assert got["hits"] == e64["hits"] == want["hits"]
        kept = [p.grad.clone() for p in pol.parameters()]
        out2 = tr.backward(xd, yd, rows=rd)                                        # the same bits
        assert torch.equal(out, out2) and all(torch.equal(p.grad, g) for p, g in zip(pol.parameters(), kept)), B
    print(f"\nfnn grad student {seed} gather {gather} over all B: worst |device - fp64| / bound {_fmt(worst)} "
          + " ".join(f"{k}={v:.3f}" for k, v in sorted(worst.items())))
    tr.close()


def test_rows_past_the_batch_and_stale_gradients_contribute_nothing():
    import torch
    seed, B = G.STUDENTS[0], 17
    pol, _, tr, _ = _trainer(seed)
    x, y, _ = G.batch(seed, B)
    xd, yd = _dev(x, y)
    out = tr.backward(xd, yd)
    kept = [p.grad.clone() for p in pol.parameters()]
    assert all(p.grad.data_ptr() == tr.grad_buffer.data_ptr() + 4 * at for p, at in tr.spec.offsets())   # views of one buffer
    # the same 17 rows with garbage behind them in x and y (the second tile's rows 17..31 exist in memory but not in the batch)
    xg = torch.cat([xd, torch.full((30, 18), float("nan"), device="cuda")])
    yg = torch.cat([yd, torch.full((30, 3), 1e30, device="cuda")])
    tr.grad_buffer.fill_(float("nan"))                                            # and stale garbage in the buffer
    out_g = tr.backward(xg, yg, rows=torch.arange(B, dtype=torch.int32, device="cuda"), validate=False)
    assert torch.equal(out, out_g) and all(torch.equal(p.grad, g) for p, g in zip(pol.parameters(), kept))
    assert bool(torch.isnan(tr.grad_buffer[G_PARAMS:]).all())                      # the padding is not written
    tr.close()



def test_a_row_with_a_bad_label_adds_nothing_and_is_refused_when_validated():
    import torch
    seed, B = G.STUDENTS[1], 33
    pol, _, tr, _ = _trainer(seed)
    x, y, _ = G.batch(seed, B)
    keep = np.arange(B) != 20
    want = G.restated(G.params64(R.make_policy(seed)), x[keep], y[keep])
    e32, e64 = G.eager(R.make_policy(seed), x[keep], y[keep]), G.eager(R.make_policy(seed), x[keep], y[keep], double=True)
    yb = y.copy()
    yb[20, 0] = 0.25
    xd, yd = _dev(x, yb)
    with pytest.raises(ValueError, match=r"y\[20, 0\] = 0.25 is not a rule type"):
        tr.backward(xd, yd)
    with pytest.raises(ValueError, match="rows holds 33, outside"):
        tr.backward(*_dev(x, y), rows=torch.tensor([0, 33], device="cuda"))
    assert all(p.grad is None for p in pol.parameters())                           # refused before anything was enqueued
    got = _got(pol, tr.backward(xd, yd, validate=False))
    w = G.ratios(got, e64, G.bounds(e32, e64))
    print(f"\nfnn grad with a bad label at row 20 against fp64 without that row: {_fmt(w)}")
    assert max(w.values()) <= 1.0 and got["hits"] == want["hits"]
    assert not G.zero_violations(got, e32, e64), G.zero_violations(got, e32, e64)
    # a rows entry outside [0, N) likewise, when validate=False lets it through: the kernel reads nothing there
    rows = np.arange(B, dtype=np.int32)
    rows[20] = 10 ** 6
    got2 = _got(pol, tr.backward(*_dev(x, y, rows), validate=False))
    assert all(np.array_equal(got[k], got2[k]) for k in got)
    tr.close()


def test_accum_adds_the_outputs_in_the_reduce_kernels_order():
    import torch
    seed = G.STUDENTS[0]
    _, _, tr, _ = _trainer(seed)
    accum = torch.zeros(4, device="cuda")
    outs = []
    for B in (17, 128, 33):
        xd, yd = _dev(*G.batch(seed, B)[:2])
        outs.append(tr.backward(xd, yd, accum=accum).clone())
    want = torch.zeros(4, device="cuda")
    for o in outs:
        want = want + o
    assert torch.equal(accum, want) and float(accum[3]) == sum(float(o[3]) for o in outs)
    with pytest.raises(ValueError, match="accum must be"):
        tr.backward(xd, yd, accum=torch.zeros(3, device="cuda"))
    tr.close()


# ----------------------------------------------------------------------------------------------------------- (b), (c) step, refresh
@pytest.mark.parametrize("seed", G.STUDENTS)
def test_one_optimiser_step_and_refresh(seed):
    import torch
    from reinforcementlearning4meshgeneration_amd import FusedFNN
    B = 128
    pol, opt, tr, fnn = _trainer(seed, with_fnn=True)
    x, y, _ = G.batch(seed, B)
    _, e32, e64 = G.references(seed, B)
    bound = G.bounds(e32, e64)
    xd, yd = _dev(x, y)
    tr.backward(xd, yd)
    tr.step()
    # eager float32 on the device and a stock step
    pe = copy.deepcopy(R.make_policy(seed)).cuda()
    oe = torch.optim.Adam(pe.parameters(), lr=G.LR)
    G.torch_loss(pe, xd, yd)[0].backward()
    oe.step()
    p0 = dict(R.make_policy(seed).named_parameters())
    g = opt.param_groups[0]
    capped, worst = {}, 0.0
    for (k, a), b in zip(pol.named_parameters(), pe.parameters()):
        st = {}
        bd = P.adam_step_bound(p0[k].detach().numpy(), e64[k], np.full(np.shape(e64[k]), bound[k]), g["lr"], g["betas"], g["eps"], st)
        capped[k] = st["capped"]
        d = (a.detach() - b.detach()).abs().cpu().numpy().astype(np.float64)
        worst = max(worst, float((d / np.maximum(2.0 * bd.reshape(d.shape), 1e-300)).max()))
        assert (d <= 2.0 * bd.reshape(d.shape)).all(), (seed, k)
        assert not torch.equal(a.detach().cpu(), p0[k].detach())                    # and the step moved them
    print(f"\nfnn step student {seed}: |device - eager| / (2 bound) max {worst:.4f}; share of elements at the cap of 2 lr: "
          + " ".join(f"{k}={v:.3f}" for k, v in capped.items()))
    assert all(float(opt.state[p]["step"]) == 1.0 for p in pol.parameters())
    # (c) refresh: the live parameters into the packed buffer, exactly as the host packs them
    obs = _dev(R.forward_observations(33))[0]
    stale = [o.clone() for o in fnn.forward(obs, raw=True)]
    fnn.refresh()
    fresh = FusedFNN.from_module(pol)
    live, want = fnn.forward(obs, raw=True), fresh.forward(obs, raw=True)
    assert all(torch.equal(a, b) for a, b in zip(live, want)) and not torch.equal(stale[3], live[3])
    opt.step()                                                                     # a stock step in between (p.grad is still there)
    fnn.refresh()
    fresh2 = FusedFNN.from_module(pol)
    live2, want2 = fnn.forward(obs, raw=True), fresh2.forward(obs, raw=True)
    assert all(torch.equal(a, b) for a, b in zip(live2, want2)) and not torch.equal(live2[3], live[3])
    for h in (fresh, fresh2, fnn, tr):
        h.close()


# ----------------------------------------------------------------------------------------------------------- (d) fit
def test_fit_is_the_hand_loop_and_tracks_eager_float64():
    import torch
    from reinforcementlearning4meshgeneration_amd import MeshVecEnv
    from reinforcementlearning4meshgeneration_amd.fnn_train import FNNTrainSpec
    seed, N, E, BS = G.STUDENTS[0], 300, 3, 128
    x, y = (a[:N] for a in G.decided_pool(seed))
    xd, yd = _dev(x, y)
    perms = FNNTrainSpec.permutations(N, E, seed=0)
    obs = _dev(R.forward_observations(33))[0]
    # fit (its own permutations from the seed) and the hand loop with the same permutations
    pol_a, opt_a, tr_a, fnn_a = _trainer(seed, with_fnn=True)
    log_a = tr_a.fit(xd, yd, E, batch_size=BS, seed=0)
    pol_b, opt_b, tr_b, fnn_b = _trainer(seed, with_fnn=True)
    pd = _dev(perms)[0]
    log_b = torch.zeros((E, 4), device="cuda")
    for e in range(E):
        for a, b in ((0, 128), (128, 256), (256, 300)):
            tr_b.backward(xd, yd, rows=pd[e, a:b], accum=log_b[e])
            tr_b.step()
    fnn_b.refresh()
    assert torch.equal(log_a.sums, log_b) and log_a.read().shape == (E, 4)
    for pa, pb in zip(pol_a.parameters(), pol_b.parameters()):
        assert torch.equal(pa, pb)
        sa, sb = opt_a.state[pa], opt_b.state[pb]
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"])
        assert float(sa["step"]) == float(sb["step"]) == 9.0
    fa, fb = fnn_a.forward(obs, raw=True), fnn_b.forward(obs, raw=True)
    assert all(torch.equal(u, v) for u, v in zip(fa, fb))
    # given permutations are the same call
    pol_c, _, tr_c, _ = _trainer(seed)
    log_c = tr_c.fit(x, y, E, batch_size=BS, perms=perms)                        # host arrays: checked and uploaded by fit
    assert torch.equal(log_c.sums, log_b) and all(torch.equal(u, v) for u, v in zip(pol_c.parameters(), pol_a.parameters()))
    # eager float32 and float64 with the same permutations: the device's per-epoch sums within 4 d32 + 1e-6 max |loss64|
    logs = []
    for dt in (torch.float32, torch.float64):
        pe = copy.deepcopy(R.make_policy(seed)).to(dt)
        logs.append(G.eager_fit(pe, torch.optim.Adam(pe.parameters(), lr=G.LR), x, y, perms, BS))
    loss32, loss64 = logs[0][:, 0], logs[1][:, 0]
    dev = log_a.read().astype(np.float64)
    d32 = float(np.abs(loss32 - loss64).max())
    tol = 4 * d32 + 1e-6 * float(np.abs(loss64).max())
    print(f"\nfnn fit: loss per epoch device {dev[:, 0].tolist()} fp64 {loss64.tolist()}; d32 {d32:.3g}, "
          f"|device - fp64| {np.abs(dev[:, 0] - loss64).max():.3g} of {tol:.3g} allowed; hits {dev[:, 3].tolist()}")
    assert (np.abs(dev[:, 0] - loss64) <= tol).all()
    assert dev[-1, 0] < dev[0, 0]
    assert np.allclose(dev[:, 0], dev[:, 1] + dev[:, 2], rtol=1e-6) and (dev[:, 3] <= N).all() and (dev[:, 3] >= 0).all()
    # and the refreshed net meshes
    doms = R.closed_loop_domains()
    env = MeshVecEnv(doms, env_domain=(np.arange(16) % len(doms)).astype(np.int32), auto_reset=False, log_capacity=512)
    res = env.mesh_with(fnn_a, max_steps=8)
    assert 1 <= res.total_steps <= 8 and tuple(res.steps.shape) == (16,) and 1 <= int(res.steps.min()) <= int(res.steps.max()) <= 8
    env.close()
    for h in (tr_a, tr_b, tr_c, fnn_a, fnn_b):
        h.close()


def test_fit_refuses_bad_data_before_anything_is_enqueued(tmp_path):
    import torch
    seed = G.STUDENTS[0]
    pol, opt, tr, _ = _trainer(seed)
    x, y = (a[:40].copy() for a in G.decided_pool(seed))
    before = [p.detach().clone() for p in pol.parameters()]
    yb = y.copy()
    yb[3, 0] = 0.75
    with pytest.raises(ValueError, match=r"y\[3, 0\] = 0.75"):
        tr.fit(x, yb, 1)
    with pytest.raises(ValueError, match=r"perms must have shape \(2, 40\)"):
        tr.fit(x, y, 2, perms=np.zeros((1, 40), np.int32))
    with pytest.raises(ValueError, match="rows holds 40"):
        tr.fit(x, y, 1, perms=np.full((1, 40), 40, np.int32))
    with pytest.raises(ValueError, match=r"x must have shape \(N, 18\)"):
        tr.fit(x[:, :14], y, 1)
    assert all(torch.equal(p, b) for p, b in zip(pol.parameters(), before)) and len(opt.state) == 0
    tr.fit(x, y, 1, batch_size=16)
    path = tmp_path / "fnn.pt"
    tr.save(path)
    sd = torch.load(path)
    assert list(sd) == list(G.NAMES) and all(torch.equal(sd[k].cuda(), p) for k, p in pol.named_parameters())
    tr.close()
