"""Episode statistics without a GPU: the numpy restatement of k_episode_stats's documented order
(tests/episode_stats_ref.py) against a plain per-replica Python loop, and flow_amd.utils.episode_stats on top of it.

Counts, lengths, min and max are exact.  The two sums may differ from the loop's by the order of their additions only: at
most R + K episodes' worth of rounded double additions per sum -- here the bound the issue sets, R * 2^-53 * sum |ret|
(for sum ret^2: with |ret|^2), the worst case of R rounded additions, derived and not measured."""
import numpy as np
import pytest

from episode_stats_ref import EMPTY, episode_stats_loop, episode_stats_ref
from flow_amd.utils.episode_stats import combine, summarize


def _inputs(K, R, p_done, seed, flag=1):
    rng = np.random.default_rng(seed)
    rew = rng.normal(0.3, 1.0, (K, R)).astype(np.float32)
    done = (rng.random((K, R)) < p_done).astype(np.uint8) * np.uint8(flag)
    return rew, done


def _check(stats, episodes, R):
    rets = np.array([e[0] for e in episodes], np.float64)
    lens = np.array([e[1] for e in episodes], np.float64)
    assert stats[0] == len(episodes)
    if not len(episodes):
        assert np.array_equal(stats, EMPTY)
        return
    assert stats[3] == rets.min() and stats[4] == rets.max()
    assert stats[5] == lens.sum() and stats[6] == lens.min() and stats[7] == lens.max()
    ref1, ref2 = sum(rets.tolist()), sum((rets * rets).tolist())
    print("sum ret %r vs %r; sum ret^2 %r vs %r" % (stats[1], ref1, stats[2], ref2))
    assert abs(stats[1] - ref1) <= R * 2.0 ** -53 * np.abs(rets).sum()
    assert abs(stats[2] - ref2) <= R * 2.0 ** -53 * (rets * rets).sum()


@pytest.mark.parametrize("K,R", [(1, 1), (8, 63), (8, 65), (8, 257), (3, 1025), (2, 256 * 512 + 77)])
def test_restatement_equals_the_loop(K, R):
    rew, done = _inputs(K, R, 0.3, 100 + R)
    stats, ret, ln = episode_stats_ref(rew, done)
    episodes, ret_l, ln_l = episode_stats_loop(rew, done)
    _check(stats, episodes, R)
    assert np.array_equal(ret, ret_l) and np.array_equal(ln, ln_l)


def test_no_episode_ends():
    rew, done = _inputs(8, 65, 0.0, 1)
    stats, ret, ln = episode_stats_ref(rew, done)
    assert np.array_equal(stats, EMPTY)
    assert np.all(ln == 8)
    assert np.array_equal(ret, episode_stats_loop(rew, done)[1])
    s = summarize(stats)
    assert s["episodes"] == 0 and s["episode_reward_mean"] is None and s["episode_len_mean"] is None
    assert s["episode_reward_min"] is None and s["episode_reward_max"] is None


def test_every_step_ends_one():
    rew, done = _inputs(8, 65, 1.1, 2)
    stats, ret, ln = episode_stats_ref(rew, done)
    assert stats[0] == 8 * 65 and stats[5] == 8 * 65 and stats[6] == 1 and stats[7] == 1
    assert stats[3] == rew.astype(np.float64).min() and stats[4] == rew.astype(np.float64).max()
    assert not ret.any() and not ln.any()
    _check(stats, episode_stats_loop(rew, done)[0], 65)


def test_any_done_bit_ends_an_episode():
    rew, done1 = _inputs(8, 257, 0.25, 3, flag=1)
    done2 = done1 * np.uint8(2)                                       # (a collision: bit 1 alone)
    a, b = episode_stats_ref(rew, done1), episode_stats_ref(rew, done2)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert a[0][0] == (done2 != 0).sum() > 0


@pytest.mark.parametrize("R", [65, 1025])
def test_two_fragments_with_carries_equal_one(R):
    K = 8
    rew, done = _inputs(2 * K, R, 0.15, 4)
    whole = episode_stats_ref(rew, done)
    s1, ret, ln = episode_stats_ref(rew[:K], done[:K])
    s2, ret, ln = episode_stats_ref(rew[K:], done[K:], ret, ln, s1, accumulate=True)
    # the carries and everything exact are identical; the sums see the same episodes in another grouping of additions
    assert np.array_equal(ret, whole[1]) and np.array_equal(ln, whole[2])
    assert np.array_equal(s2[[0, 3, 4, 5, 6, 7]], whole[0][[0, 3, 4, 5, 6, 7]])
    _check(s2, episode_stats_loop(rew, done)[0], R)
    # an episode that straddles the two fragments is counted once, where it ends
    straddle = np.zeros((2 * K, 1), np.uint8)
    straddle[K + 2, 0] = 1
    r1 = np.ones((2 * K, 1), np.float32)
    a, ret, ln = episode_stats_ref(r1[:K], straddle[:K])
    assert a[0] == 0 and ln[0] == K and ret[0] == K
    b, ret, ln = episode_stats_ref(r1[K:], straddle[K:], ret, ln, a, accumulate=True)
    assert b[0] == 1 and b[1] == K + 3 and b[5] == K + 3 and ln[0] == K - 3


def test_combine_of_two_shards_against_the_stacked_input():
    K, Ra, Rb = 8, 65, 257
    rew, done = _inputs(K, Ra + Rb, 0.2, 5)
    sa = episode_stats_ref(rew[:, :Ra], done[:, :Ra])[0]
    sb = episode_stats_ref(rew[:, Ra:], done[:, Ra:])[0]
    both = np.array(combine([sa, sb]))
    assert both[0] == sa[0] + sb[0] and both[1] == sa[1] + sb[1] and both[2] == sa[2] + sb[2] and both[5] == sa[5] + sb[5]
    assert both[3] == min(sa[3], sb[3]) and both[4] == max(sa[4], sb[4])
    assert both[6] == min(sa[6], sb[6]) and both[7] == max(sa[7], sb[7])
    _check(both, episode_stats_loop(rew, done)[0], Ra + Rb)
    assert combine([]) == list(EMPTY) and combine([sa]) == sa.tolist()
    assert sa.tolist() == [float(v) for v in sa]                      # (a pure function: its inputs are untouched)
    s = summarize(both)
    eps = episode_stats_loop(rew, done)[0]
    rets = np.array([e[0] for e in eps])
    assert s["episodes"] == len(eps)
    assert s["episode_reward_mean"] == pytest.approx(rets.mean(), rel=1e-12)
    assert s["episode_reward_std"] == pytest.approx(rets.std(), rel=1e-9)
    assert s["episode_reward_min"] == rets.min() and s["episode_reward_max"] == rets.max()
    assert s["episode_len_mean"] == pytest.approx(np.mean([e[1] for e in eps]), rel=1e-12)
