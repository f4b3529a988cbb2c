"""GPU: ``EpisodeStats`` (k_episode_stats, csrc/meshenv_learn.h) on synthetic histories against the Monitor restatement of
tests/offpolicy_learn_ref.py: the ring, the episode count and both carries are equal bit for bit, the means are ``np.mean`` of
the reference deque.  The kernel is one workgroup of 1024 threads: n = 1025 gives thread 0 a second env (the thread-stride seam
of phase 1) and T * n = 2050 a third trip of the ordered scan of phase 2; n = 33 ends inside a wavefront; window 4 with 7
episodes in one call drops the first three of that call."""
import numpy as np
import pytest

import offpolicy_learn_ref as LR

pytestmark = pytest.mark.gpu


def _up(reward, done, complete):
    import torch
    return dict(reward=torch.from_numpy(np.ascontiguousarray(reward)).cuda(), done=torch.from_numpy(np.ascontiguousarray(done)).cuda(),
                complete=torch.from_numpy(np.ascontiguousarray(complete)).cuda())


def _check(stats, ref):
    ring, count = stats.ring.cpu().numpy(), int(stats.count.cpu().numpy().view(np.uint64)[0])
    assert count == ref.count
    assert np.array_equal(ring.view(np.int64), ref.ring().view(np.int64))
    cr, cl = ref.carries()
    assert np.array_equal(stats.carry_return.cpu().numpy().view(np.int64), cr.view(np.int64))
    assert np.array_equal(stats.carry_len.cpu().numpy(), cl)
    got, want = stats.read(), ref.logs()
    assert got["episodes"] == want["episodes"]
    if ref.count:
        for k in ("rollout/ep_rew_mean", "rollout/ep_len_mean", "complete_rate"):
            assert got[k] == want[k], k
    else:
        assert "rollout/ep_rew_mean" not in got and "rollout/ep_len_mean" not in got and np.isnan(got["complete_rate"])


def _stats(n, window):
    from reinforcementlearning4meshgeneration_amd import EpisodeStats
    return EpisodeStats(n, window=window)


@pytest.mark.parametrize("T,n,window,p", [(5, 1, 100, 0.4), (3, 33, 100, 0.3), (2, 1025, 100, 0.3), (2, 1025, 4096, 0.5),
                                          (3, 33, 4, 0.3)])
def test_two_calls_equal_the_monitor(T, n, window, p):
    stats, ref = _stats(n, window), LR.MonitorRef(n, window)
    try:
        _check(stats, ref)                                               # nothing finished yet: no rollout keys
        for call in range(2):
            h = LR.synthetic_history(T, n, seed=100 * T + n + call, p_done=p)
            stats.update(_up(*h))
            ref.update(*h)
            _check(stats, ref)
        assert ref.count > 0
        if window == 4096:
            assert 1024 < ref.count <= window                            # more episodes than one scan trip, none dropped
        if n == 1025 and window == 100:
            assert ref.count > 2 * window                                # each call drops all but its last 100
    finally:
        stats.close()


def _history(T, n, done_at, seed):
    """done exactly at the (t, env) pairs of done_at; every other one complete."""
    reward, _, _ = LR.synthetic_history(T, n, seed)
    done = np.zeros((T, n), np.uint8)
    for t, e in done_at:
        done[t, e] = 1
    complete = done.copy()
    complete.reshape(-1)[::2] = 0
    return reward, done, complete


def test_window_4_with_7_episodes_in_one_call_and_over_three_calls():
    at = [(0, 1), (0, 2), (1, 0), (2, 1), (2, 2), (3, 0), (3, 2)]          # 7 episodes in flat order
    whole = _history(4, 3, at, 1)
    one, ref = _stats(3, 4), LR.MonitorRef(3, 4)
    three, ref3 = _stats(3, 4), LR.MonitorRef(3, 4)
    try:
        one.update(_up(*whole))
        ref.update(*whole)
        _check(one, ref)
        assert ref.count == 7 and len(ref.buffer) == 4
        wrong = LR.MonitorRef(3, 4, order="env_t")
        wrong.update(*whole)
        assert not np.array_equal(wrong.ring(), one.ring.cpu().numpy())   # the (env, t) order is told apart
        for a, b in ((0, 1), (1, 3), (3, 4)):                              # 2, 3 and 2 episodes; episodes span the seams
            part = tuple(x[a:b] for x in whole)
            three.update(_up(*part))
            ref3.update(*part)
            _check(three, ref3)
        assert np.array_equal(three.ring.cpu().numpy(), one.ring.cpu().numpy())
        assert one.read() == three.read()
    finally:
        one.close()
        three.close()


def test_no_done_then_every_entry_done():
    n, T = 33, 3
    stats, ref = _stats(n, 8), LR.MonitorRef(n, 8)
    try:
        quiet = _history(T, n, [], 2)
        stats.update(_up(*quiet))
        ref.update(*quiet)
        _check(stats, ref)                                                 # a call with no done: only the carries move
        assert ref.count == 0 and int(ref.carries()[1].min()) == T
        every = _history(T, n, [(t, e) for t in range(T) for e in range(n)], 3)
        stats.update(_up(*every))
        ref.update(*every)
        _check(stats, ref)                                                 # the first row closes the episodes carried in
        assert ref.count == T * n and int(ref.carries()[1].max()) == 0
        assert ref.buffer[-1][1] == 1.0 and stats.read()["rollout/ep_len_mean"] == 1.0
    finally:
        stats.close()


def test_update_refuses_other_shapes():
    import torch
    stats = _stats(4, 4)
    try:
        h = _up(*LR.synthetic_history(2, 4, 0))
        with pytest.raises(ValueError, match="reward must be a contiguous"):
            stats.update(dict(h, reward=h["reward"].float()))
        with pytest.raises(ValueError, match=r"done must be a \[T, 4\] tensor"):
            stats.update(dict(h, done=torch.zeros((2, 5), dtype=torch.uint8, device="cuda")))
    finally:
        stats.close()
