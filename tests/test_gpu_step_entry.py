"""GPU: the entry, the hand-over and the write-back of the CU-group step kernel, bit for bit against the one-wave kernel.

k_step_group reads what its entry needs from preloaded kernel arguments, hands an update to another wavefront through
flag words in LDS and writes a step's results back through pointers it re-reads from the kernel-argument segment
(csrc/meshenv_kernels.h: EntryArgs, spin_until_nonzero, late_state / late_outs / late_step0).  None of this may change a
result.  meshenv_create reads MESHENV_GROUP once, at creation, and the variable forces the CU-group kernel at any batch
size: every case builds one handle on k_step (MESHENV_GROUP=1, the yardstick) and one on k_step_group, drives both with
the same seeded action stream and compares every output after every step, and the work counters at the end.  Batches of
two or three workgroups whose last one is partly inactive; every instantiation of the kernel (ring stride <= 64, longer
rings, rings of mixed domains packed by their own lengths); and a five-vertex ring, whose every step ends the episode, so
that the reset path and terminal_obs run every step.

Seed, policy mix and step count were chosen on the CPU oracle (oracle.ref_lib.RefBatch): 200 steps of this stream end
19 / 12 / 4 / 16 episodes in cases a / b / c / d."""
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

T = 200
SEED = 7


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    return torch


def _golden_domain(name):
    tr = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    return [tuple(p) for p in tr["domain_xy"]]


def _actions(n):
    """Uniform over the action box, 60 % of the rows redrawn from the biased sub-box of the golden generators."""
    rng = np.random.default_rng(SEED)
    a = rng.uniform([-1, -1.5, 0], [1, 1.5, 1.5], size=(T, n, 3))
    pick = rng.random((T, n)) < 0.6
    b = np.stack([rng.uniform(-1, 1, (T, n)), rng.uniform(0.2, 1.0, (T, n)), rng.uniform(0.3, 1.2, (T, n))], axis=2)
    a[pick] = b[pick]
    return a.astype(np.float32)


def _make(group, doms, env_domain, auto_reset):
    from reinforcementlearning4meshgeneration_amd import MeshVecEnv
    before = os.environ.get("MESHENV_GROUP")
    os.environ["MESHENV_GROUP"] = str(group)      # read once, by meshenv_create
    try:
        return MeshVecEnv(doms, env_domain=env_domain, auto_reset=auto_reset)
    finally:
        if before is None:
            del os.environ["MESHENV_GROUP"]
        else:
            os.environ["MESHENV_GROUP"] = before


def _bits(torch, x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x.view(torch.int64) if x.dtype == torch.float64 else x


def _compare(torch, doms, n, group, want_kernel, auto_reset=True, need_work=True):
    env_domain = (np.arange(n) % len(doms)).astype(np.int32)
    ref = _make(1, doms, env_domain, auto_reset)
    got = _make(group, doms, env_domain, auto_reset)
    try:
        assert "k_step<" in ref.step_kernel, ref.step_kernel
        assert got.step_kernel != ref.step_kernel and "k_step_group" in got.step_kernel, got.step_kernel
        assert got.step_kernel == want_kernel, got.step_kernel
        msg_ref = torch.zeros((n, 21), dtype=torch.float32, device=ref.device)
        msg_got = torch.zeros((n, 21), dtype=torch.float32, device=ref.device)
        ref.set_packed_output(msg_ref)
        got.set_packed_output(msg_got)
        assert torch.equal(_bits(torch, ref.obs), _bits(torch, got.obs))     # the reset observation
        a = torch.from_numpy(_actions(n)).cuda()
        finished = 0
        for t in range(T):
            o0, r0, d0, c0 = ref.step(a[t])
            o1, r1, d1, c1 = got.step(a[t])
            for name, x, y in (("obs", o0, o1), ("reward", r0, r1), ("done", d0, d1), ("complete", c0, c1),
                               ("terminal_obs", ref.terminal_obs, got.terminal_obs), ("message", msg_ref, msg_got)):
                assert torch.equal(_bits(torch, x), _bits(torch, y)), (name, t)
            finished += int(d0.sum())
        k0, k1 = ref.counters(), got.counters()
        assert k0 == k1, (k0, k1)
        assert k0["steps"] == T * n
        print(want_kernel, "n", n, "extractions", k0["valid"], "finished episodes", finished)
        if need_work:      # on the yardstick leg: the stream extracted elements and ended episodes
            assert k0["valid"] >= 200 and finished >= 1, (k0, finished)
        return k0, finished
    finally:
        ref.close()
        got.close()


def test_a_small_rings_g16_partly_inactive_last_workgroup(torch_cuda):
    """boundary(), G = 16, 37 envs: three workgroups, eleven inactive waves in the last; the ring-stride <= 64 instantiation."""
    from reinforcementlearning4meshgeneration_amd.domains import boundary
    _compare(torch_cuda, [boundary(0)], 37, 16, "meshenv::k_step_group<16, true, false, true>")


def test_b_small_rings_g8_partly_inactive_last_workgroup(torch_cuda):
    """boundary(), G = 8, 19 envs: three workgroups of eight, five inactive waves in the last."""
    from reinforcementlearning4meshgeneration_amd.domains import boundary
    _compare(torch_cuda, [boundary(0)], 19, 8, "meshenv::k_step_group<8, true, false, true>")


def test_c_long_rings_g16(torch_cuda):
    """A 120-vertex ring (two 64-slot chunks at the entry), G = 16, 21 envs: the general instantiation."""
    d1 = _golden_domain("boundary16_biased_s2")
    assert len(d1) == 120
    _compare(torch_cuda, [d1], 21, 16, "meshenv::k_step_group<16, true, false, false>")


def test_d_mixed_domains_ragged_lds(torch_cuda):
    """120 / 196 / 272-vertex rings interleaved, G = 16, 35 envs: the LDS of a workgroup is packed by each ring's own length,
    and the entry reads the env's region from GroupArgs::env_lds."""
    doms = [_golden_domain(x) for x in ("boundary16_biased_s2", "boundary15_biased_s5", "test1_biased_s42")]
    assert [len(d) for d in doms] == [120, 196, 272]
    _compare(torch_cuda, doms, 35, 16, "meshenv::k_step_group<16, true, true, false>")


@pytest.mark.parametrize("auto_reset", [True, False])
def test_e_every_step_ends_the_episode(torch_cuda, auto_reset):
    """A five-vertex ring: every step ends the episode (B:141-143), so every step writes terminal_obs and, with
    auto-reset, copies the domain's reset state back -- on the waves that ran the checks, no update is ever dealt."""
    d = _golden_domain("basic_biased_s4")
    assert len(d) == 5
    k, finished = _compare(torch_cuda, [d], 20, 16, "meshenv::k_step_group<16, true, false, true>", auto_reset=auto_reset,
                           need_work=False)
    assert finished == T * 20 and k["valid"] == 0
