"""k_episode_stats (fs_episode_stats_dev, VecFlowEnv.episode_stats) against the numpy restatement of its documented order
(tests/episode_stats_ref.py), bit for bit: every shape at which the launch changes -- one lane, a wave short of / at / past
its end, more than one workgroup, lanes with more than one replica past 512 workgroups is the restatement's own case on the
CPU (R = 131149 there) --, carries over two calls, accumulate, the empty case, the same bits on a second call, a real
fused fragment, and a captured graph."""
import numpy as np
import pytest

from episode_stats_ref import EMPTY, episode_stats_loop, episode_stats_ref
from test_ringrl_gpu import make, rl_ring_spec

pytestmark = pytest.mark.gpu

SHAPES = [(K, R) for R in (1, 63, 64, 65, 257, 1025, 2049) for K in (1, 8)]


def _inputs(K, R, p_done, seed):
    rng = np.random.default_rng(seed)
    rew = rng.normal(0.3, 1.0, (K, R)).astype(np.float32)
    done = ((rng.random((K, R)) < p_done) * rng.integers(1, 4, (K, R))).astype(np.uint8)     # (any bit ends an episode)
    return rew, done


class Device(object):
    """One handle of R replicas and the buffers of fs_episode_stats_dev."""

    def __init__(self, R):
        import torch
        self.torch, self.dev = torch, torch.device("cuda", 0)
        self.sim = make(rl_ring_spec(R=R, N=22, seed=1), "f32")
        self.ret = torch.zeros(R, dtype=torch.float64, device=self.dev)
        self.len = torch.zeros(R, dtype=torch.int32, device=self.dev)
        self.stats = torch.full((8,), 7.0, dtype=torch.float64, device=self.dev)       # (garbage: accumulate=0 overwrites)
        torch.cuda.synchronize()

    def call(self, rew, done, accumulate):
        from flow_amd import _lib as L
        torch = self.torch
        r, d = torch.as_tensor(rew, device=self.dev), torch.as_tensor(done, device=self.dev)
        torch.cuda.synchronize()
        L.check(self.sim.lib.fs_episode_stats_dev(self.sim._h, int(rew.shape[0]), r.data_ptr(), d.data_ptr(), self.ret.data_ptr(),
                                                  self.len.data_ptr(), self.stats.data_ptr(), int(accumulate)), self.sim.lib)
        self.sim.sync()
        assert self.sim.last_kernel == "k_episode_stats"
        return self.stats.cpu().numpy().copy(), self.ret.cpu().numpy().copy(), self.len.cpu().numpy().copy()


def _same(got, want, msg):
    for name, g, w in zip(("stats", "run_ret", "run_len"), got, want):
        assert g.dtype == w.dtype, (msg, name, g.dtype, w.dtype)
        np.testing.assert_array_equal(g.view(np.uint64) if g.dtype == np.float64 else g,
                                      w.view(np.uint64) if w.dtype == np.float64 else w, err_msg="%s: %s" % (msg, name))


@pytest.mark.parametrize("K,R", SHAPES)
def test_kernel_equals_its_restatement_bit_for_bit(K, R):
    d = Device(R)
    rew, done = _inputs(K, R, 0.3, 10 * R + K)
    got = d.call(rew, done, 0)
    want = episode_stats_ref(rew, done)
    _same(got, want, "first call")
    # the carries over a second call, accumulated
    rew2, done2 = _inputs(K, R, 0.5, 10 * R + K + 1)
    got2 = d.call(rew2, done2, 1)
    want2 = episode_stats_ref(rew2, done2, want[1], want[2], want[0], accumulate=True)
    _same(got2, want2, "second call, accumulate")
    assert got2[0][0] == (done != 0).sum() + (done2 != 0).sum()
    # the same inputs from the same carries: the same bits (no float atomics, the ticket was reset)
    d.ret.copy_(d.torch.as_tensor(want[1])), d.len.copy_(d.torch.as_tensor(want[2]))
    d.stats.copy_(d.torch.as_tensor(want[0]))
    _same(d.call(rew2, done2, 1), got2, "repeat")
    # no episode ends: the empty statistics, the carries go on
    rew3, done3 = _inputs(K, R, 0.0, 3)
    got3 = d.call(rew3, done3, 0)
    np.testing.assert_array_equal(got3[0], EMPTY)
    _same(got3, episode_stats_ref(rew3, done3, got2[1], got2[2]), "empty")
    # ... and accumulating nothing leaves what was there
    d.stats.copy_(d.torch.as_tensor(got2[0]))
    np.testing.assert_array_equal(d.call(rew3, done3, 1)[0], got2[0])
    d.sim.close()


def test_arguments_are_checked():
    from flow_amd import _lib as L
    d = Device(4)
    with pytest.raises(Exception, match="fs_episode_stats_dev"):
        L.check(d.sim.lib.fs_episode_stats_dev(d.sim._h, 0, d.ret.data_ptr(), d.ret.data_ptr(), d.ret.data_ptr(),
                                               d.len.data_ptr(), d.stats.data_ptr(), 0), d.sim.lib)
    with pytest.raises(Exception, match="fs_episode_stats_dev"):
        L.check(d.sim.lib.fs_episode_stats_dev(d.sim._h, 1, None, d.ret.data_ptr(), d.ret.data_ptr(), d.len.data_ptr(),
                                               d.stats.data_ptr(), 0), d.sim.lib)
    d.sim.close()


def _ring_params(horizon):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_vec
    return train_vec.ring_flow_params(horizon)


def test_a_real_fused_fragment_and_the_python_layer():
    """VecFlowEnv.episode_stats after fused ring fragments (horizon 5, K = 8: resets fall inside): the episode count is the
    count of done flags, the carries straddle the two fragments, sum ret is the host loop's within R 2^-53 sum |ret|."""
    import torch
    from test_policy_gpu import make_policy
    from flow_amd.envs import VecFlowEnv
    from flow_amd.utils.episode_stats import summarize
    K, R = 8, 48
    vec = VecFlowEnv(_ring_params(5), num_replicas=R)
    pol = make_policy(2, True, seed=1)
    vec.reset()
    frags = []
    for f in range(2):
        _, _, _, rew, done = vec.policy_rollout(pol, K, reset_done=True)
        assert vec.sim.last_kernel == "k_ring_policy"
        stats = vec.episode_stats(rew, done, reset=f == 0)
        assert vec.sim.last_kernel == "k_episode_stats"
        frags.append((rew.cpu().numpy().copy(), done.cpu().numpy().copy(), stats.cpu().numpy().copy()))
    rew = np.concatenate([f[0] for f in frags])
    done = np.concatenate([f[1] for f in frags])
    stats = frags[1][2]
    episodes = episode_stats_loop(rew, done)[0]
    rets = np.array([e[0] for e in episodes])
    print("episodes %d, sum ret %r (host loop %r)" % (stats[0], stats[1], sum(rets.tolist())))
    assert stats[0] == (done != 0).sum() == len(episodes) == R * (2 * K // 5)
    assert abs(stats[1] - sum(rets.tolist())) <= R * 2.0 ** -53 * np.abs(rets).sum()
    assert stats[3] == rets.min() and stats[4] == rets.max()
    assert stats[5] == 5 * len(episodes) and stats[6] == 5 and stats[7] == 5           # (an episode straddles the fragments)
    # the first fragment alone, then the second through the restatement with the carries: the kernel's bits
    a = episode_stats_ref(frags[0][0], frags[0][1])
    np.testing.assert_array_equal(a[0].view(np.uint64), frags[0][2].view(np.uint64))
    b = episode_stats_ref(frags[1][0], frags[1][1], a[1], a[2], a[0], accumulate=True)
    np.testing.assert_array_equal(b[0].view(np.uint64), stats.view(np.uint64))
    s = summarize(stats)
    assert s["episodes"] == len(episodes) and s["episode_len_mean"] == 5.0
    assert s["episode_reward_mean"] == pytest.approx(rets.mean(), rel=1e-12)
    # accumulate=False: this fragment's episodes alone, the carries kept
    _, _, _, rew3, done3 = vec.policy_rollout(pol, K, reset_done=True)
    only = vec.episode_stats(rew3, done3, accumulate=False).cpu().numpy()
    c = episode_stats_ref(rew3.cpu().numpy(), done3.cpu().numpy(), b[1], b[2])
    np.testing.assert_array_equal(only.view(np.uint64), c[0].view(np.uint64))
    with pytest.raises(ValueError):
        vec.episode_stats(rew3[:, :5], done3[:, :5])
    vec.close()


def test_captured_in_a_graph_two_replays_equal_two_eager_calls():
    import torch
    K, R = 8, 257
    dev = torch.device("cuda", 0)
    rew, done = _inputs(K, R, 0.2, 77)
    eager = Device(R)
    e1 = eager.call(rew, done, 0)
    e2 = eager.call(rew, done, 1)
    d = Device(R)
    r, dn = torch.as_tensor(rew, device=dev), torch.as_tensor(done, device=dev)
    from flow_amd import _lib as L

    def launch(acc):
        L.check(d.sim.lib.fs_episode_stats_dev(d.sim._h, K, r.data_ptr(), dn.data_ptr(), d.ret.data_ptr(), d.len.data_ptr(),
                                               d.stats.data_ptr(), acc), d.sim.lib)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        d.sim.set_stream(stream.cuda_stream)
        launch(0)                                                     # (eager, on the capture stream: allocates the scratch)
        d.sim.sync()
        d.ret.zero_(), d.len.zero_()
        d.stats.copy_(torch.as_tensor(EMPTY, device=dev))
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        launch(1)
    out = []
    for _ in range(2):
        with torch.cuda.stream(stream):
            graph.replay()
        stream.synchronize()
        out.append((d.stats.cpu().numpy().copy(), d.ret.cpu().numpy().copy(), d.len.cpu().numpy().copy()))
    _same(out[0], e1, "first replay")
    _same(out[1], e2, "second replay")
    d.sim.close(), eager.sim.close()
