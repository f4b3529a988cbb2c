"""CPU: the host half of the FNN training (reinforcementlearning4meshgeneration_amd/fnn_train.py, include/meshenv_fnn_train.h):
the fp64 restatement of tests/fnn_grad_ref.py against torch autograd, the packaging of the C-ABI, every Python refusal, and the
conditions tests/test_gpu_fnn_grad.py and tests/test_gpu_fnn_grad_range.py need of their students and data.  Nothing here needs
a GPU."""
import os
import re
import types

import numpy as np
import pytest

import fnn_grad_ref as G
import fnn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shared_data_has_the_three_classes_and_zero_rows():
    x, y = G.data()
    assert x.shape == (G.POOL, 18) and y.shape == (G.POOL, 3) and x.dtype == y.dtype == np.float32
    counts = np.bincount(np.rint(2 * y[:, 0]).astype(int), minlength=3)
    print("classes of the shared data:", counts.tolist(), "zero rows:", int((np.abs(x).sum(axis=1) == 0).sum()))
    assert set(np.unique(y[:, 0])) == {0.0, 0.5, 1.0} and (counts > 500).all()
    assert (np.abs(x).sum(axis=1) == 0).sum() > 100
    # the teacher alone gives classes 1 and 2 only: the rows off the every-fifth grid hold no class 0
    off = np.ones(G.POOL, bool)
    off[::5] = False
    assert not (y[off, 0] == 0).any()


@pytest.mark.parametrize("seed", G.STUDENTS)
@pytest.mark.parametrize("B", [1, 17, 128])
def test_restatement_matches_autograd_in_float64(B, seed):
    want, _, e64 = G.references(seed, B)
    worst = 0.0
    for k in (*G.NAMES, *G.LOSSES):
        a, b = np.asarray(want[k]), np.asarray(e64[k])
        assert a.shape == b.shape, k
        scale = max(float(np.abs(b).max()), 1e-30)
        worst = max(worst, float(np.abs(a - b).max()) / scale)
    print(f"student {seed} B {B}: restatement against autograd float64, worst relative difference {worst:.3g}")
    assert worst < 1e-12
    assert want["hits"] == e64["hits"]
    assert abs(want["loss"] - (want["classification_loss"] + want["regression_loss"])) <= 1e-12 * abs(want["loss"])
    assert all(float(np.abs(want[k]).max()) > 0 for k in G.NAMES)


@pytest.mark.parametrize("seed", G.STUDENTS)
def test_relu_condition_and_the_yardstick_on_the_chosen_inputs(seed):
    """The rows a float32 / float64 comparison cannot use stay under the cap, and eager float32 is off float64 by a few
    float32 roundings of the largest gradient: the figures the GPU test's bound is made of."""
    bad = G.undecided(seed)
    x, _ = G.decided_pool(seed)
    print(f"student {seed}: {int(bad.sum())} of {G.POOL} rows undecided, {int(bad[:128].sum())} among the first 128")
    assert bad.mean() <= G.UNDECIDED_CAP and len(x) == G.POOL - bad.sum() >= max(G.GPU_BS)
    for B in (17, 128, 2065):
        for gather in (False, True):
            _, e32, e64 = G.references(seed, B, gather)
            rel = {k: float(np.abs(e32[k] - e64[k]).max()) / float(np.abs(e64[k]).max()) for k in G.NAMES}
            print(f"  B {B} gather {gather}: eager float32 off float64 by {min(rel.values()):.2g} .. {max(rel.values()):.2g} of max |g64|")
            assert 0 < max(rel.values()) < 5e-6
            assert e32["hits"] == e64["hits"]


# ---- the students of tests/test_gpu_fnn_grad_range.py: what the references alone say of them, pinned as observed
RANGE_BATCHES = {    # key -> the (B, gather) its GPU tests run
    **{k: [(B, g) for B in (1, 17, 128, 2065) for g in (False, True)] for k in G.CONFIDENT},
    G.DEAD: [(33, False), (128, False)],
    **{k: [(90, False), (90, True)] for k in G.SAMPLER},
}
DEEP_STUDENTS = (G.STUDENTS[0], G.CONFIDENT[1])
# key -> ReLU-undecided rows, fp64 argmax counts over the rows, hits on the first 17 / 128 / 2065 decided rows (or on all 90).
# The ReLU condition compares |z64| with the float32 error of the host's own BLAS, so its count is a property of the host as
# well: the trunk of seed 6 has 9 such rows where these counts were taken and 12 on the MI355X host (another CPU, other float32
# kernels under torch); the trunk of seed 11 has 3 on both.  Every other figure is the same on both.
RELU_11, RELU_6 = (3,), (9, 12)
PINNED = {
    G.CONFIDENT[0]: dict(relu=RELU_11, argmax=[4101, 0, 0], hits=[4, 26, 414], loss_2065=6.84e4),
    G.CONFIDENT[1]: dict(relu=RELU_6, argmax=[0, 332, 3769], hits=[0, 0, 241], loss_2065=1.40e5),
    G.DEAD: dict(relu=RELU_11, argmax=[0, 4101, 0], hits=[10, 91, 1318]),
    G.SAMPLER[0]: dict(relu=(0,), argmax=[0, 90, 0], hits=[30]),
    G.SAMPLER[1]: dict(relu=(0,), argmax=[0, 90, 0], hits=[30]),
}


def test_keyed_helpers_give_the_plain_seeds_what_they_gave():
    """A bare seed is a student key: the same net, the same rows, no hits condition, no unit left out of the ReLU condition."""
    for seed in G.STUDENTS:
        assert np.array_equal(G.undecided(seed), G.relu_undecided(seed))
        for a, b in zip(G.policy(seed).parameters(), R.make_policy(seed).parameters()):
            assert np.array_equal(a.detach().numpy(), b.detach().numpy())
        x, y = G.data()
        xs, ys = G.decided_pool(seed)
        assert np.array_equal(xs, x[~G.undecided(seed)]) and np.array_equal(ys, y[~G.undecided(seed)])
        xb, yb, rows = G.batch(seed, 33)
        assert rows is None and np.array_equal(xb, xs[:33]) and np.array_equal(yb, ys[:33])
        _, _, rows = G.batch(seed, 2065, gather=True)
        assert rows.dtype == np.int32 and len(np.unique(rows)) == 2065 and rows.max() < len(xs)
    counts = [int(G.undecided(s).sum()) for s in G.STUDENTS]                # the trunks the confident students share
    assert counts[0] in RELU_11 and counts[1] in RELU_6, counts
    assert [int(G.relu_undecided(k).sum()) for k in G.CONFIDENT] == counts


def test_sampler_rows_are_the_recorded_accepted_candidates():
    x, y = G.sampler_rows()
    assert x.shape == (90, 18) and y.shape == (90, 3) and x.dtype == y.dtype == np.float32
    assert np.bincount(np.rint(2 * y[:, 0]).astype(int), minlength=3).tolist() == [30, 30, 30]
    assert set(np.unique(y[:, 0])) == {0.0, 0.5, 1.0}
    print("sampler rows: x in", [float(x.min()), float(x.max())], "targets in", [float(y[:, 1:].min()), float(y[:, 1:].max())])
    assert -1.58 < x.min() < -1.56 and 4.50 < x.max() < 4.52 and 0.03 < y[:, 1:].min() < 0.05 and 1.81 < y[:, 1:].max() < 1.83
    # 90 rows are six tiles, the last of ten rows
    assert -(-90 // 16) == 6 and 90 % 16 == 10


def test_dead_policy_is_the_seeded_net_with_three_crafted_units_a_layer():
    dead, plain = G.policy(G.DEAD), R.make_policy(G.DEAD[1])
    for name, out, _ in R.LAYERS[:5]:
        w, b = (getattr(getattr(dead, name), p).detach().numpy() for p in ("weight", "bias"))
        w0, b0 = (getattr(getattr(plain, name), p).detach().numpy() for p in ("weight", "bias"))
        minus, zero = G.crafted_units(out)
        crafted = [*minus, zero]
        assert minus == (0, out - 1) and zero == 1
        assert not w[crafted].any() and (b[list(minus)] == -1).all() and b[zero] == 0
        rest = np.setdiff1d(np.arange(out), crafted)
        assert np.array_equal(w[rest], w0[rest]) and np.array_equal(b[rest], b0[rest])
    for head in ("action_head", "type_head"):
        assert np.array_equal(getattr(dead, head).weight.detach().numpy(), getattr(plain, head).weight.detach().numpy())


@pytest.mark.parametrize("key", list(PINNED), ids=str)
def test_conditions_of_the_range_students(key):
    """The ReLU condition, the hits condition, the cap, the eager hits and the bounds of every student and batch of
    tests/test_gpu_fnn_grad_range.py, from the references alone; the counts as observed."""
    pin = PINNED[key]
    relu, margin = G.relu_undecided(key), G.margin_undecided(key)
    x, y = G.rows_of(key)
    pool = G.decided_pool(key)[0]
    l64 = R.eager(G.policy(key), x, double=True)[1]
    spread = float((l64.max(axis=1) - l64.min(axis=1)).max())
    counts = np.bincount(l64.argmax(axis=1), minlength=3).tolist()
    print(f"student {key}: {int(relu.sum())} ReLU-undecided and {int(margin.sum())} margin-undecided rows of {len(x)}; logits in "
          f"[{l64.min():.4g}, {l64.max():.4g}], spread up to {spread:.4g}; fp64 argmax counts {counts}")
    assert int(relu.sum()) in pin["relu"] and int(margin.sum()) == 0
    assert np.array_equal(G.undecided(key), relu | margin) and (relu | margin).mean() <= G.UNDECIDED_CAP
    assert len(pool) == len(x) - int((relu | margin).sum())
    assert counts == pin["argmax"]
    if key == G.CONFIDENT[0]:     # no overflow without the row maximum, every term of lse representable or flushed late
        assert 38 < l64.max() < 88 and 63 < spread < 64
    if key == G.CONFIDENT[1]:     # expf(121) overflows float32, expf(-313) underflows to 0
        assert l64.max() > 89 and spread > 104
    sizes = [90] if key in G.SAMPLER else [17, 128, 2065]
    assert [G.references(key, B)[2]["hits"] for B in sizes] == pin["hits"]
    if "loss_2065" in pin:
        assert abs(G.references(key, 2065)[2]["loss"] / pin["loss_2065"] - 1) < 5e-3
    batches = RANGE_BATCHES[key] + ([(G.DEEP_B, False), (G.DEEP_B, True)] if key in DEEP_STUDENTS else [])
    for B, gather in batches:
        want, e32, e64 = G.references(key, B, gather)
        bound = G.bounds(e32, e64)
        worst = max(G.ratios(want, e64, bound).values())
        print(f"  B {B} gather {gather}: hits {e64['hits']}, loss {e64['loss']:.6g}, smallest bound {min(bound.values()):.3g}, "
              f"restatement against autograd float64 {worst:.3g} of the bound")
        assert e32["hits"] == e64["hits"] == want["hits"]
        assert all(v > 0 for v in bound.values()), {k: v for k, v in bound.items() if not v > 0}
        assert worst < 1e-3
        assert all(np.isfinite(e32[k]).all() and np.isfinite(e64[k]).all() for k in (*G.NAMES, *G.LOSSES))


def test_deep_walk_batches_cycle_the_pool_and_repeat_rows():
    from reinforcementlearning4meshgeneration_amd import _capi
    tiles = -(-G.DEEP_B // 16)
    assert tiles == 385 == 3 * _capi.FNN_GRAD_MAX_GROUPS + 1 and G.DEEP_B % 16 == 1     # workgroup 0 four tiles, the others three
    for key in DEEP_STUDENTS:
        px, py = G.decided_pool(key)
        x, y, rows = G.batch(key, G.DEEP_B)
        assert rows is None and x.shape == (G.DEEP_B, 18) and len(px) < G.DEEP_B
        assert np.array_equal(x[:len(px)], px) and np.array_equal(x[len(px):], px[:G.DEEP_B - len(px)]) and np.array_equal(y[len(px):], py[:G.DEEP_B - len(py)])
        x, y, rows = G.batch(key, G.DEEP_B, gather=True)
        assert x is px and rows.shape == (G.DEEP_B,) and rows.dtype == np.int32
        assert np.array_equal(np.sort(rows[:len(px)]), np.arange(len(px))) and np.array_equal(rows[len(px):], rows[:G.DEEP_B - len(px)])
        assert not np.array_equal(rows[:len(px)], np.arange(len(px)))
        for gather in (False, True):
            want, e32, e64 = G.references(key, G.DEEP_B, gather)
            print(f"student {key} B {G.DEEP_B} gather {gather}: hits {e64['hits']}, loss {e64['loss']:.6g}")
            assert e32["hits"] == e64["hits"] == want["hits"] and all(v > 0 for v in G.bounds(e32, e64).values())


def test_gradients_that_are_exactly_zero_in_eager_torch():
    """What the exact-zero rule of the GPU tests rests on: units dead on a whole batch give exact zeros in eager float32 and
    float64 alike (student 11 on 33 rows: 8 of fc5's 16 bias gradients are non-zero), and the crafted units of the dead-unit
    student give the named zero rows and columns while the rest of each tensor is non-zero."""
    _, e32, e64 = G.references(G.STUDENTS[0], 33)
    zeros = G.exact_zeros(e32, e64)
    assert int((~zeros["fc5.bias"]).sum()) == 8 and np.array_equal(e32["fc5.bias"] == 0, e64["fc5.bias"] == 0)
    for B in (33, 128):
        _, e32, e64 = G.references(G.DEAD, B)
        zeros = G.exact_zeros(e32, e64)
        blocks = G.dead_zero_blocks()
        assert len(blocks) == 5 * 2 + 4 + 2
        for name, idx in blocks:
            assert zeros[name][idx].size and zeros[name][idx].all(), (B, name)
            assert (~zeros[name]).any(), (B, name)
        print(f"dead-unit student B {B}: exact zeros per tensor", {k: int(v.sum()) for k, v in zeros.items()})


def test_exports_and_header():
    import reinforcementlearning4meshgeneration_amd as pkg
    from reinforcementlearning4meshgeneration_amd import _capi, fnn, fnn_train
    assert len(_capi.EXPORTS_FNN_TRAIN) == 8
    header = open(os.path.join(ROOT, "include", "meshenv_fnn_train.h")).read()
    defines = dict(re.findall(r"#define\s+(MESHENV_[A-Z_]+)\s+(\d+)", header))
    n_params = sum(rows * cols + rows for _, rows, cols in fnn.LAYERS)
    assert n_params == 20485
    assert int(defines["MESHENV_FNN_GRAD_FLOATS"]) == _capi.FNN_GRAD_FLOATS == (n_params + 63) // 64 * 64
    assert int(defines["MESHENV_FNN_GRAD_OUTPUTS"]) == _capi.FNN_GRAD_OUTPUTS == len(fnn_train.OUTPUTS) == 4
    assert int(defines["MESHENV_FNN_GRAD_MAX_GROUPS"]) == _capi.FNN_GRAD_MAX_GROUPS == 128
    # the largest batch of the GPU test has more tiles than the header's rule gives workgroups, and a last tile of one row
    assert -(-max(G.GPU_BS) // 16) > _capi.FNN_GRAD_MAX_GROUPS >= -(-sorted(G.GPU_BS)[-2] // 16) and max(G.GPU_BS) % 16 == 1
    kernels = open(os.path.join(ROOT, "reinforcementlearning4meshgeneration_amd", "csrc", "meshenv_fnn_grad.h")).read()
    assert "k_fnn_grad" in kernels and "k_fnn_grad_reduce" in kernels and "__builtin_amdgcn_mfma_f32_16x16x4f32" in kernels
    assert "atomic" not in kernels.replace("No floating-point atomics", "")
    assert _capi.load().meshenv_abi_version() == 1      # a header of its own: meshenv.h is unchanged
    for k in ("FusedFNNTrain", "FNNTrainSpec", "FNNTrainLog"):
        assert k in pkg.__all__ and getattr(pkg, k) is getattr(fnn_train, k)
    assert hasattr(pkg.FusedFNN, "bind_live") and hasattr(pkg.FusedFNN, "refresh")


def test_null_handles_and_unbound_calls_are_refused_by_the_library():
    from reinforcementlearning4meshgeneration_amd import _capi
    L = _capi.load()
    assert L.meshenv_fnn_grad_bind(None, None, None, 0) == _capi.E_ARG
    assert L.meshenv_fnn_grad_backward(None, 1, 1, None, None, None, None, None) == _capi.E_ARG
    assert L.meshenv_fnn_bind(None, None) == _capi.E_ARG and L.meshenv_fnn_refresh(None) == _capi.E_ARG
    L.meshenv_fnn_grad_destroy(None)


def test_spec_refuses_other_architectures_and_optimisers():
    import torch
    from reinforcementlearning4meshgeneration_amd.fnn_train import FNNTrainSpec
    pol = R.make_policy(0)
    spec = FNNTrainSpec(pol, torch.optim.Adam(pol.parameters(), lr=1e-3))
    assert spec.n_grad == 20544 and [at for _, at in spec.offsets()][:3] == [0, 64 * 18, 64 * 18 + 64]
    assert [tuple(p.shape) for p in spec.params] == [s for _, r, c in R.LAYERS for s in ((r, c), (r,))]
    wide = torch.nn.Sequential()                                   # original_ann.py's 6 -> 500 -> 500 -> 3
    wide.fc1, wide.fc2 = torch.nn.Linear(6, 500), torch.nn.Linear(500, 500)
    with pytest.raises(ValueError, match=r"fc1.weight has shape \(500, 6\), expected \(64, 18\)"):
        FNNTrainSpec(wide, None)
    headless = types.SimpleNamespace(**{n: getattr(pol, n) for n, _, _ in R.LAYERS[:-1]})
    with pytest.raises(ValueError, match="type_head"):
        FNNTrainSpec(headless, None)
    with pytest.raises(ValueError, match="float64"):
        FNNTrainSpec(R.make_policy(0).double(), None)
    with pytest.raises(ValueError, match="torch.optim.Adam"):
        FNNTrainSpec(pol, torch.optim.SGD(pol.parameters(), lr=1e-3))
    with pytest.raises(ValueError, match="amsgrad"):
        FNNTrainSpec(pol, torch.optim.Adam(pol.parameters(), lr=1e-3, amsgrad=True))
    with pytest.raises(ValueError, match="not exactly the 14 parameters"):
        FNNTrainSpec(pol, torch.optim.Adam(list(pol.parameters())[:-1], lr=1e-3))
    with pytest.raises(ValueError, match="not exactly the 14 parameters"):
        FNNTrainSpec(pol, torch.optim.Adam(R.make_policy(1).parameters(), lr=1e-3))


def test_data_refusals_labels_rows_and_shapes():
    import torch
    from reinforcementlearning4meshgeneration_amd.fnn_train import FNNTrainSpec as S
    x, y = (a[:40].copy() for a in G.data())
    for conv in (np.asarray, torch.from_numpy):
        assert S.check_shapes(conv(x), conv(y)) == (40, 40)
        assert S.check_shapes(conv(x), conv(y), conv(np.arange(7, dtype=np.int32))) == (40, 7)
        S.check_labels(conv(y))
        S.check_rows(conv(np.array([0, 39, 5], np.int32)), 40)
        for bad in (0.25, 2.0, -0.5, float("nan"), 1.0000001):
            yb = y.copy()
            yb[17, 0] = bad
            with pytest.raises(ValueError, match=r"y\[17, 0\] = .* is not a rule type"):
                S.check_labels(conv(yb))
        for rows, what in (([0, 40], "40"), ([-1, 3], "-1"), ([2 ** 31 - 1], str(2 ** 31 - 1))):
            with pytest.raises(ValueError, match=f"rows holds {what}, outside"):
                S.check_rows(conv(np.array(rows, np.int64)), 40)
        with pytest.raises(ValueError, match=r"x must have shape \(N, 18\)"):
            S.check_shapes(conv(x[:, :14].copy()), conv(y))              # the reference's own (2, 3) samples: 14 columns
        with pytest.raises(ValueError, match=r"x must have shape"):
            S.check_shapes(conv(x[:0]), conv(y[:0]))
        with pytest.raises(ValueError, match=r"y must have shape \(40, 3\)"):
            S.check_shapes(conv(x), conv(y[:, :2].copy()))
        with pytest.raises(ValueError, match=r"y must have shape \(40, 3\)"):
            S.check_shapes(conv(x), conv(y[:39]))
        with pytest.raises(ValueError, match="rows must have shape"):
            S.check_shapes(conv(x), conv(y), conv(np.zeros((2, 2), np.int32)))
        with pytest.raises(ValueError, match="rows must have shape"):
            S.check_shapes(conv(x), conv(y), conv(np.zeros(0, np.int32)))
        with pytest.raises(ValueError, match="int32 or int64"):
            S.check_shapes(conv(x), conv(y), conv(np.zeros(3, np.float32)))


def test_permutations_and_minibatches_are_the_data_loaders():
    from reinforcementlearning4meshgeneration_amd.fnn_train import FNNTrainSpec as S
    assert S.minibatches(300, 128) == [(0, 128), (128, 256), (256, 300)]           # drop_last=False: the short one is last
    assert S.minibatches(256, 128) == [(0, 128), (128, 256)] and S.minibatches(5, 128) == [(0, 5)]
    with pytest.raises(ValueError, match="batch_size"):
        S.minibatches(10, 0)
    p = S.permutations(300, 3, seed=7)
    assert p.shape == (3, 300) and p.dtype == np.int32 and all(np.array_equal(np.sort(r), np.arange(300)) for r in p)
    assert np.array_equal(p, S.permutations(300, 3, seed=7)) and not np.array_equal(p[0], p[1])
    rng = np.random.default_rng(7)                                                   # a host loop can reproduce it
    assert np.array_equal(p, np.stack([rng.permutation(300) for _ in range(3)]))
    with pytest.raises(ValueError, match=r"perms must have shape \(3, 300\)"):
        S.check_perms(p[:2], 3, 300)


def test_eager_loop_learns_on_the_shared_data():
    """The yardstick of the fit test: three epochs of the eager loop in float32 and float64 agree and the loss falls."""
    import copy
    import torch
    from reinforcementlearning4meshgeneration_amd.fnn_train import FNNTrainSpec as S
    x, y = G.decided_pool(G.STUDENTS[0])
    x, y = x[:300], y[:300]
    perms = S.permutations(300, 3, seed=0)
    logs = []
    for dt in (torch.float32, torch.float64):
        pol = copy.deepcopy(R.make_policy(G.STUDENTS[0])).to(dt)
        logs.append(G.eager_fit(pol, torch.optim.Adam(pol.parameters(), lr=G.LR), x, y, perms, 128))
    d32 = np.abs(logs[0][:, 0] - logs[1][:, 0]).max()
    print("eager fit, loss per epoch float32:", logs[0][:, 0].tolist(), "float64:", logs[1][:, 0].tolist(), "d32", d32)
    assert logs[1][-1, 0] < logs[1][0, 0] and d32 < 1e-3 * logs[1][0, 0]
