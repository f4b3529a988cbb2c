"""Host side of the FNN-mesher tests (tests/test_fnn_cpu.py, tests/test_gpu_fnn.py): the network restated in eager torch, the
closed meshing loop of general/EBRD.py:525-548 on the CPU (eager torch + the oracle's move()), the seeded nets both files
use with the counts the CPU run gave, and the unpacking of the kernel's weight buffer.  Nothing here needs a GPU."""
import copy
import functools
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (name, out, in) of the seven torch.nn.Linear layers of the reference's Policy (general/EBRD.py:85-91)
LAYERS = (("fc1", 64, 18), ("fc2", 128, 64), ("fc3", 64, 128), ("fc4", 32, 64), ("fc5", 16, 32), ("action_head", 2, 16),
          ("type_head", 3, 16))
K_PAD = (32, 64, 128, 64, 32, 16)          # inputs of fc1 .. fc5 and the head tile, padded to a multiple of 16
PACKED_FLOATS = 21568

# ---- the closed-loop nets: torch.manual_seed(seed) default init, action_head.bias overwritten with ACTION_BIAS (a point
# inside the useful range of move(): radius fraction, angle).  Chosen by test_fnn_cpu.test_seed_hunt's loop; the counts are what
# the CPU reference (eager torch float32 + oracle) gave on the 48 envs of closed_loop_domains() within MAX_STEPS moves.
ACTION_BIAS = (0.25, 0.85)
N_ENVS = 48
MAX_STEPS = 104
CLOSED_LOOP_SEED = 6
CLOSED_LOOP_COUNTS = dict(envs_with_accepted_move=45, envs_through_smooth_pave=12, finished_early=6, unfinished=42)
CLOSED_LOOP_ACCEPTED_MOVES = 888        # elements extracted by the 48 envs together
# ---- the forward nets: (seed, type_head scale).  Scale 1 is the plain default init the tolerance is stated for; on these
# observations its rule type is the same on every row (the biases decide it), so a second net has its type_head weight scaled
# by 40 and its type_head bias zeroed: its fp64 argmax is 1 on 3047 and 2 on 1049 of forward_observations(4096).  No row of
# either net has a top-two margin under 8 err_torch (err_torch 1.9e-8 and 6.0e-7): nothing is excluded, under the 1 % cap.
FORWARD_NETS = ((11, 1.0), (12, 40.0))


def make_policy(seed, action_bias=None):
    """A Policy-shaped eager module: forward(x) -> (action [.., 2], type_values [.., 3])."""
    import torch
    import torch.nn as nn
    import torch.nn.functional as F

    class Policy(nn.Module):
        def __init__(self):
            super().__init__()
            self.fc1 = nn.Linear(18, 64)
            self.fc2 = nn.Linear(64, 128)
            self.fc3 = nn.Linear(128, 64)
            self.fc4 = nn.Linear(64, 32)
            self.fc5 = nn.Linear(32, 16)
            self.action_head = nn.Linear(16, 2)
            self.type_head = nn.Linear(16, 3)

        def forward(self, x):
            for fc in (self.fc1, self.fc2, self.fc3, self.fc4, self.fc5):
                x = F.relu(fc(x))
            return self.action_head(x), self.type_head(x)

    torch.manual_seed(seed)
    p = Policy()
    if action_bias is not None:
        with torch.no_grad():
            p.action_head.bias.copy_(torch.tensor(action_bias, dtype=torch.float32))
    return p.eval()


def forward_policy(seed, type_scale):
    import torch
    p = make_policy(seed)
    if type_scale != 1.0:
        with torch.no_grad():
            p.type_head.weight.mul_(type_scale)
            p.type_head.bias.zero_()
    return p


def eager(policy, obs, double=False):
    """(actions [n, 2], logits [n, 3]) of the eager module on obs [n, 18] float32, in float32 or (double=True) in float64."""
    import torch
    with torch.no_grad():
        x = torch.as_tensor(np.asarray(obs, np.float32))
        if double:
            a, l = copy.deepcopy(policy).double()(x.double())
        else:
            a, l = policy(x)
    return a.numpy(), l.numpy()


def forward_stats(policy, obs):
    """What the forward tolerance rests on: err_torch = max |eager fp32 - fp64| over actions and logits, the fp64 top-two logit
    margin per row, and the rows that margin > 8 err_torch keeps."""
    a32, l32 = eager(policy, obs)
    a64, l64 = eager(policy, obs, double=True)
    err = max(float(np.abs(a32 - a64).max()), float(np.abs(l32 - l64).max()))
    top = np.sort(l64, axis=1)
    margin = top[:, 2] - top[:, 1]
    return dict(a32=a32, l32=l32, a64=a64, l64=l64, err_torch=err, margin=margin, decided=margin > 8 * err)


def get_action(policy, obs):
    """EBRD.get_action (:174-177) for a batch: (points float64 [n, 2] -- the widening of tolist() --, types float64 [n])."""
    a, l = eager(policy, obs)
    import torch
    return a.astype(np.float64), torch.argmax(torch.from_numpy(l), dim=1).numpy().astype(np.float64) / 2.0


def closed_loop_domains():
    from reinforcementlearning4meshgeneration_amd.domains import boundary, random_domain
    d1 = [tuple(p) for p in np.load(os.path.join(GOLDEN_DIR, "boundary16_biased_s2.npz"))["domain_xy"]]
    return [boundary(0), boundary(-1), d1] + [random_domain(900 + k) for k in range(13)]


def make_refs(doms, n, cap_new=512):
    from oracle.ref_lib import RefEnv
    return [RefEnv.from_points(doms[k % len(doms)], cap_new=cap_new) for k in range(n)]


class OracleLoop:
    """n oracle envs driven one vector step at a time with the loop's bookkeeping: an env finishes at the move that returns
    done or code >= 2 and is not moved again."""

    def __init__(self, refs):
        self.refs = refs
        n = len(refs)
        self.obs = np.stack([r.reset(static=True)[0] for r in refs])
        self.finished = np.zeros(n, bool)
        self.steps = np.zeros(n, np.int32)
        self.code = np.zeros(n, np.uint8)
        self.done = np.zeros(n, np.uint8)
        self.complete = np.zeros(n, np.uint8)
        self.accepted = np.zeros(n, np.int64)
        self.smoothed = np.zeros(n, np.int64)
        self.first_smooth = np.full(n, -1)      # the move (counted from 1) that first went through smooth_pave

    def summary(self):
        """Copies of the bookkeeping and of every env's ring, element count and not_valid count, as they are now."""
        out = {k: getattr(self, k).copy() for k in ("obs", "finished", "steps", "code", "done", "complete", "accepted", "smoothed",
                                                    "first_smooth")}
        out["rings"] = [r.ring() for r in self.refs]
        out["n_elem"] = np.array([r.scalars()["n_elem"] for r in self.refs])
        out["n_not_valid"] = np.array([r.not_valid_count() for r in self.refs])
        return out

    def step(self, points, types):
        """Moves every unfinished env; returns (ran [n] bool, obs, done, complete, code) of this step (rows of envs that did not
        run are zero / 255)."""
        n = len(self.refs)
        ran = ~self.finished
        o = np.zeros((n, 18), np.float32)
        d = np.zeros(n, np.uint8)
        c = np.zeros(n, np.uint8)
        code = np.full(n, 255, np.uint8)
        for k in np.flatnonzero(ran):
            r = self.refs[k]
            ne0, nv0 = r.scalars()["n_elem"], r.not_valid_count()
            o_r, d_r, c_r, code_r = r.move(points[k], types[k])
            ne1 = r.scalars()["n_elem"]
            self.accepted[k] += ne1 > ne0
            # a rejected move that leaves not_valid_points empty went through smooth_pave (rl/boundary_env.py:405-426)
            self.smoothed[k] += int(code_r != 2 and ne1 == ne0 and r.not_valid_count() == 0 and nv0 > 0)
            if code_r == 2:
                d_r = c_r = False      # the reference raises: nothing is returned
            o[k], d[k], c[k], code[k] = o_r, d_r, c_r, code_r
            self.steps[k] += 1
            if self.smoothed[k] and self.first_smooth[k] < 0:
                self.first_smooth[k] = self.steps[k]
            self.code[k], self.done[k], self.complete[k] = code_r, d_r, c_r
            if code_r != 2:
                self.obs[k] = o_r
            if d_r or code_r >= 2:
                self.finished[k] = True
        return ran, o, d, c, code


@functools.lru_cache(maxsize=4)
def closed_loop_cpu(seed, max_steps=MAX_STEPS, n=N_ENVS):
    """The CPU reference of mesh_with: eager torch float32 + the oracle.  Returns the loop (counts per env) and the
    observations every forward read, [T, n, 18] with the rows of finished envs zero."""
    policy = make_policy(seed, ACTION_BIAS)
    loop = OracleLoop(make_refs(closed_loop_domains(), n))
    seen = []
    for _ in range(max_steps):
        if loop.finished.all():
            break
        seen.append(np.where(loop.finished[:, None], np.float32(0), loop.obs))
        pts, typ = get_action(policy, loop.obs)
        loop.step(pts, typ)
    return loop, np.stack(seen)


def closed_loop_counts(loop, max_steps=MAX_STEPS):
    """loop: an OracleLoop or its summary()."""
    g = loop.get if isinstance(loop, dict) else lambda k: getattr(loop, k)     # noqa: E731
    accepted, smoothed, finished, steps = g("accepted"), g("smoothed"), g("finished"), g("steps")
    return dict(envs_with_accepted_move=int((accepted > 0).sum()), envs_through_smooth_pave=int((smoothed > 0).sum()),
                finished_early=int((finished & (steps < max_steps)).sum()), unfinished=int((~finished).sum()))


# ---- the early-stop net: all weights zero, type_head.bias (1, 0, 0), action_head.bias EARLY_STOP_POINT.  The logits are the bias
# exactly, so every forward returns type 0 and that point, and the oracle alone says where each of EARLY_STOP_ENVS envs
# (two forward tiles, the second ragged) ends: every env with done = 1, complete = 0, code 0, after EARLY_STOP_STEPS moves,
# each through smooth_pave at least once.
EARLY_STOP_POINT = (0.375, -1.25)
EARLY_STOP_TYPE_BIAS = (1.0, 0.0, 0.0)
EARLY_STOP_ENVS = 21
EARLY_STOP_STEPS = (10, 8, 10, 162, 108, 26, 12, 179, 137, 10, 192, 151, 39, 185, 116, 68, 10, 8, 10, 162, 108)


def early_stop_state_dict():
    import torch
    sd = {k: torch.zeros_like(v) for k, v in make_policy(0).state_dict().items()}
    sd["type_head.bias"] = torch.tensor(EARLY_STOP_TYPE_BIAS, dtype=torch.float32)
    sd["action_head.bias"] = torch.tensor(EARLY_STOP_POINT, dtype=torch.float32)
    return sd


def early_stop_cpu(max_steps=500):
    """The oracle alone under the early-stop net's constant action: the OracleLoop after at most max_steps vector steps, and
    the number of vector steps made."""
    loop = OracleLoop(make_refs(closed_loop_domains(), EARLY_STOP_ENVS))
    points = np.tile(np.float64(np.float32(EARLY_STOP_POINT)), (EARLY_STOP_ENVS, 1))
    types = np.zeros(EARLY_STOP_ENVS)
    total = 0
    while total < max_steps and not loop.finished.all():
        loop.step(points, types)
        total += 1
    return loop, total


def forward_observations(n):
    """n observation rows for the forward tests: the static observations the closed loop of CLOSED_LOOP_SEED visited (its
    reset(static=True) rows first), cycled, with every 17th row zero (the reference's None)."""
    _, seen = closed_loop_cpu(CLOSED_LOOP_SEED)
    pool = seen.reshape(-1, 18)
    pool = pool[np.abs(pool).sum(axis=1) > 0]
    obs = np.resize(pool, (n, 18)).astype(np.float32)
    obs[16::17] = 0
    return np.ascontiguousarray(obs)


def unpack(packed):
    """The fourteen tensors back out of the kernel's buffer (include/meshenv_fnn.h states the layout): per layer the weight as
    [tile][K / 16][lane 64][4], element j of lane l in group g = W[16 tile + (l & 15)][4 (4 g + j) + (l >> 4)], then the bias;
    the two heads share the last tile, action_head in rows 0-1 and type_head in rows 2-4.  Also returns the floats that belong
    to no tensor (the padding), which must be zero."""
    packed = np.asarray(packed, np.float32)
    assert packed.shape == (PACKED_FLOATS,)
    used = np.zeros(PACKED_FLOATS, bool)
    out, at = {}, 0
    rows_of = [(("fc1", 0, 64),), (("fc2", 0, 128),), (("fc3", 0, 64),), (("fc4", 0, 32),), (("fc5", 0, 16),),
               (("action_head", 0, 2), ("type_head", 2, 3))]
    cols_of = (18, 64, 128, 64, 32, 16)
    for l, tensors in enumerate(rows_of):
        K, groups = K_PAD[l], K_PAD[l] // 16
        tiles = (max(r0 + rows for _, r0, rows in tensors) + 15) // 16
        w_at, b_at = at, at + tiles * K * 16
        for name, r0, rows in tensors:
            w = np.zeros((rows, cols_of[l]), np.float32)
            for n in range(rows):
                tile, col = divmod(r0 + n, 16)
                for k in range(cols_of[l]):
                    g, j, q = k // 16, (k // 4) % 4, k % 4
                    i = w_at + (((tile * groups + g) * 64) + 16 * q + col) * 4 + j
                    w[n, k] = packed[i]
                    used[i] = True
            out[name + ".weight"] = w
            out[name + ".bias"] = packed[b_at + r0:b_at + r0 + rows].copy()
            used[b_at + r0:b_at + r0 + rows] = True
        at = b_at + 16 * tiles
    assert at == PACKED_FLOATS
    return out, packed[~used]
