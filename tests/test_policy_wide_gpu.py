"""BottleneckDesiredVelocityEnv's ONE policy with an action vector, eager (flow_amd/csrc/flowsim_policy.h k_policy_act_wide,
policy_wide_act): the network maps the whole observation (4 cells + 1 values, 33 .. 513) to num_rl <= 64 action columns;
column c is sampled by lane c from Philox column 0x40000000 + c.  And that kernel inside a captured fragment
(VecFlowEnv.capture with a DevicePolicy).

* the network is the network: every column against a float64 numpy evaluation of the same weights, at every size at which
  the chunking of the first layer and the mapping of columns to lanes change;
* the log-probability is the float32 ascending sum over the columns;
* the bits do not depend on the launch: number of replicas, place of the replica, replica offset;
* a captured fragment equals eager stepping (fs_policy_act_dev, fs_step_dev, masked fs_reset_dev with warm-up steps) bit
  for bit, and its simulator is the oracle's;
* what is not built is refused by name, every message naming FS_ENV_BOTTLENECK_DV;
* a masked launch that selects nothing in a wave / workgroup skips its steps (FLOWSIM_NO_MASK_SKIP=1: the full launch)
  without changing a bit;
* singleagent_bottleneck.py through VecFlowEnv and train_on_device(fuse_action_vector=True)."""
import os
import sys

import numpy as np
import pytest

from helpers import bottleneck_spec, bottleneck_tables, merge_spec, segment_cells
from oracle import opennet as O
from test_open_gpu import make, quiet
from test_policy_merge_po_gpu import STATE_FIELDS, make_vec_policy

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "k_policy_act_wide"
SHIPPED_OBS = [("1", 1), ("2", 3), ("3", 3), ("4", 3), ("5", 1)]        # 35 lane-segments: 141 observations
SHIPPED_ACT = [("2", 2), ("3", 2), ("4", 2)]                            # 20 lane-segments
# edge "1" has four lanes, edge "5" one: n segments of edge "1" are 4 n cells
OBS = {33: [("1", 2)], 65: [("1", 4)], 141: SHIPPED_OBS, 257: [("1", 16)], 513: [("1", 32)]}
ACT = {1: [("5", 1)], 16: [("1", 4)], 17: [("1", 4), ("5", 1)], 20: SHIPPED_ACT, 40: [("1", 10)], 64: [("1", 16)]}


def wide_spec(R, in_dim=141, A=20, cap_human=40, cap_rl=8, **kw):
    tb = bottleneck_tables()
    oc, ac = segment_cells(tb, OBS[in_dim]), segment_cells(tb, ACT[A])
    assert 4 * len(oc) + 1 == in_dim and len(ac) == A
    return bottleneck_spec(R=R, cap_human=cap_human, cap_rl=cap_rl, obs_cells=oc, action_cells=ac, num_rl=A, **kw)


def make_wide_policy(in_dim, A, num_hidden=2, free=False, seed=0, log_std=-0.7, dev="cuda:0", ls_slope=0.05):
    """in_dim inputs -> 1..3 x 32 tanh -> A means [+ A log stds]; the weight scales of
    test_policy_merge_po_gpu.make_vec_policy.  free: column c's log std is log_std + ls_slope * c."""
    import torch
    from flow_amd.utils.device_policy import DevicePolicy
    g = torch.Generator().manual_seed(seed)
    dims = [in_dim] + [32] * num_hidden
    hidden = [torch.nn.Linear(dims[i], dims[i + 1]) for i in range(num_hidden)]
    head = torch.nn.Linear(32, A if free else 2 * A)
    for l in hidden + [head]:
        with torch.no_grad():
            l.weight.copy_(torch.randn(l.weight.shape, generator=g) * (0.4 if l is head else 0.25))
            l.bias.copy_(torch.randn(l.bias.shape, generator=g) * 0.2)
    with torch.no_grad():
        head.weight.mul_(0.3)
    for l in hidden + [head]:
        l.to(dev)
    ls = torch.nn.Parameter(torch.full((A,), float(log_std), device=dev) + ls_slope * torch.arange(A, device=dev)) if free else None
    return DevicePolicy(hidden, head, log_std=ls, seed=77 + seed, act_dim=A)


def pin_log_std(pol, value):
    """The policy's log std at `value` in every column, whatever the observation: the free parameter, or the log-std rows
    of the output layer (weights 0, bias `value`)."""
    import torch
    A = pol.act_dim
    with torch.no_grad():
        if pol.ls is not None:
            pol.log_std_param.fill_(value)
        else:
            pol.head.weight[A:].zero_()
            pol.head.bias[A:].fill_(value)
    pol.sync()
    return pol


def numpy_net(pol, obs):
    """(means [R, A], log stds [R, A]) of the policy's weights in float64."""
    h = np.asarray(obs, dtype=np.float64)
    for l in pol.hidden:
        h = np.tanh(h @ l.weight.detach().cpu().numpy().astype(np.float64).T + l.bias.detach().cpu().numpy().astype(np.float64))
    out = h @ pol.head.weight.detach().cpu().numpy().astype(np.float64).T + pol.head.bias.detach().cpu().numpy().astype(np.float64)
    A = pol.act_dim
    if pol.ls is not None:
        return out, np.broadcast_to(pol.log_std_param.detach().cpu().numpy().astype(np.float64), out.shape)
    return out[:, :A], out[:, A:]


def act(sim, pol, obs):
    """One fs_policy_act_dev call: (act [R, A], logp [R]) as numpy arrays."""
    import torch
    dev = torch.device("cuda", 0)
    o = torch.as_tensor(np.ascontiguousarray(obs, dtype=np.float32), device=dev)
    a, lp = torch.zeros((sim.R, sim.num_rl), device=dev), torch.zeros((sim.R,), device=dev)
    torch.cuda.synchronize()              # (the handles launch on streams of their own)
    sim.policy_act_dev(pol.struct, o, a, lp)
    sim.sync()
    assert sim.last_kernel == KERNEL
    return a.cpu().numpy(), lp.cpu().numpy()


def random_obs(R, in_dim, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (R, in_dim)).astype(np.float32)


# ---- 1. the net is the network ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_dim,A,num_hidden,free,cap_human", [
    (33, 1, 1, True, 40), (65, 16, 2, False, 40), (141, 20, 2, True, 40), (141, 17, 3, False, 40),
    (257, 40, 3, True, 40), (257, 64, 1, False, 40), (513, 64, 2, True, 72), (513, 20, 3, False, 72)])
def test_the_net_is_the_network(in_dim, A, num_hidden, free, cap_human):
    """Log std -30: the action is the kernel's mean, which must be the float64 network's in every column at atol 2e-5 (the
    bar of test_policy_merge_po_gpu.py::test_the_net_is_the_torch_net; a float32 evaluation of these weights stays within
    1.1e-5 of float64 before tanh whatever the order of its first-layer sum, a dropped input moves a mean by far more).
    Zeroing the last input, input 31 (the last of chunk 0) and input 32 (the first of chunk 1) must each change the
    means, and the changed means must be the network's again."""
    R = 256
    sim = make(wide_spec(R, in_dim, A, cap_human=cap_human), "f32")
    assert sim.obs_dim == in_dim and sim.policy_action_dim == A and sim.policy_agents == 1
    assert (sim.N > 64) == (in_dim == 513)
    pol = pin_log_std(make_wide_policy(in_dim, A, num_hidden, free, seed=num_hidden + A), -30.0)
    obs = random_obs(R, in_dim, in_dim + A)
    a, _ = act(sim, pol, obs)
    mu, _ = numpy_net(pol, obs)
    print("in_dim %d, A %d: max |kernel - float64| = %.3g" % (in_dim, A, np.abs(a - mu).max()))
    np.testing.assert_allclose(a, mu, atol=2e-5, rtol=0)
    if A > 1:
        assert np.abs(mu[:, 0] - mu[:, A - 1]).max() > 1e-2            # the columns are different functions
        assert np.abs(a[:, 0] - a[:, A - 1]).max() > 1e-2
    for i in (in_dim - 1, 31, 32):
        obs0 = obs.copy()
        obs0[:, i] = 0.0
        a0, _ = act(sim, pol, obs0)
        mu0, _ = numpy_net(pol, obs0)
        np.testing.assert_allclose(a0, mu0, atol=2e-5, rtol=0, err_msg="input %d zeroed" % i)
        assert np.abs(a0 - a).max() > 1e-3, "input %d does not reach the means" % i
        assert np.abs(mu0 - mu).max() > 1e-3
    sim.close()


# ---- 2. the log-probability ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,free", [(17, True), (20, False), (64, True)])
def test_log_probability_is_the_float32_ascending_sum_over_the_columns(A, free):
    """The method of test_policy_merge_po_gpu.py::test_log_probability_is_the_float32_sum_over_the_columns: g recovered
    from the kernel's own action, its mean (the same trunk and mean rows with the log std at -30, a second handle at the
    same counter) and the log std (the free parameter, or the float64 network's); atol 1e-5 per replica.
    The free log stds lie around -1.4, where a column's expected log-probability (-1/2 - log std - 0.919) is about zero:
    the sum over 64 columns then stays within +-16 or so, where float32 resolves 1e-6.  (With log stds that grow to +2.5
    over 64 columns the sums are around -150, where one unit in the last place is 1.5e-5 and the bar cannot be read.)"""
    import torch
    R, in_dim = 256, 141
    spec = wide_spec(R, in_dim, A)
    pol = make_wide_policy(in_dim, A, 2, free, seed=11, log_std=-1.4, ls_slope=0.002)
    obs = random_obs(R, in_dim, 5)
    sim = make(spec, "f32")
    a, lp = act(sim, pol, obs)
    sim.close()
    mean_pol = make_wide_policy(in_dim, A, 2, True, seed=11, log_std=-30.0)
    with torch.no_grad():
        mean_pol.log_std_param.fill_(-30.0)
        mean_pol.head.weight.copy_(pol.head.weight[:A])
        mean_pol.head.bias.copy_(pol.head.bias[:A])
        for l_dst, l_src in zip(mean_pol.hidden, pol.hidden):
            l_dst.weight.copy_(l_src.weight)
            l_dst.bias.copy_(l_src.bias)
    mean_pol.struct.seed = pol.struct.seed
    mean_pol.sync()
    sim = make(spec, "f32")
    mu, _ = act(sim, mean_pol, obs)
    sim.close()
    _, ls = numpy_net(pol, obs)
    g = (a.astype(np.float64) - mu.astype(np.float64)) / np.exp(ls)
    per_col = (-0.5 * g * g - ls - 0.9189385332046727).astype(np.float32)
    ref = per_col[:, 0].copy()
    for c in range(1, A):
        ref = (ref + per_col[:, c]).astype(np.float32)
    assert 2.0 < np.abs(g).max() < 6.0 and abs(g.mean()) < 0.1 and 0.9 < g.std() < 1.1        # standard normal draws
    assert np.abs(g[:, 0] - g[:, 1]).max() > 0.5                                              # column 1 is another stream
    print("A %d: max |logp - ref| = %.3g" % (A, np.abs(lp - ref).max()))
    np.testing.assert_allclose(lp, ref, atol=1e-5, rtol=0)


# ---- 3. launch-shape independence ----------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_the_launch():
    in_dim, A, big, lo = 141, 20, 130, 125
    row = random_obs(1, in_dim, 9)[0]
    # the same observation row in the first and the last replica of a small and a big launch; log std -60: the sample is
    # the mean bit for bit (the replicas draw different numbers)
    mean_pol = pin_log_std(make_wide_policy(in_dim, A, 2, False, seed=4), -60.0)
    got = []
    for R in (3, big):
        obs = random_obs(R, in_dim, R)
        obs[0], obs[R - 1] = row, row
        sim = make(wide_spec(R, in_dim, A), "f32")
        a, _ = act(sim, mean_pol, obs)
        a2, _ = act(sim, mean_pol, obs)                      # a second call: the means stay
        np.testing.assert_array_equal(a, a2)
        sim.close()
        got += [a[0], a[R - 1]]
    for x in got[1:]:
        np.testing.assert_array_equal(x, got[0])
    assert np.abs(got[0]).max() > 1e-3
    # sampling: a handle with replica_offset = lo reproduces rows lo .. of the big handle, first and second call
    pol = make_wide_policy(in_dim, A, 2, True, seed=5, log_std=-0.7)
    obs = random_obs(big, in_dim, 21)
    whole, part = make(wide_spec(big, in_dim, A), "f32"), make(wide_spec(big - lo, in_dim, A, replica_offset=lo), "f32")
    first = None
    for call in range(2):
        a, lp = act(whole, pol, obs)
        b, lq = act(part, pol, obs[lo:])
        np.testing.assert_array_equal(a[lo:], b, err_msg="call %d" % call)
        np.testing.assert_array_equal(lp[lo:], lq, err_msg="call %d" % call)
        if first is None:
            first = a
    assert (np.abs(a - first) > 1e-4).mean() > 0.99          # the counter advanced: other samples
    whole.close(), part.close()


# ---- 4. / 5. / 7. the captured fragment -----------------------------------------------------------------------------------
class SpecVec(object):
    """What StepGraph needs of a VecFlowEnv, around a handle made from a plain spec."""

    def __init__(self, spec):
        import torch
        from flow_amd.envs.vec import StepGraph
        self.torch, self.sim, self.device = torch, make(spec, "f32"), torch.device("cuda", 0)
        self.num_envs, self.obs_dim, self.act_dim = self.sim.R, self.sim.obs_dim, self.sim.act_dim
        self._obs = torch.zeros((self.num_envs, self.obs_dim), device=self.device)
        self._graph = StepGraph
        self._bound = None
        torch.cuda.synchronize()

    def use_current_stream(self):
        st = self.torch.cuda.current_stream(self.device).cuda_stream
        if st != self._bound:
            self.sim.set_stream(st)
            self._bound = st

    def reset(self):
        self.use_current_stream()
        self.sim.reset_dev(self._obs, None)
        return self._obs

    def capture(self, K, policy, reset_done):
        return self._graph(self, K, policy, reset_done)


def state_of(sim):
    from flow_amd import _lib as L
    return {name: sim.get_state(getattr(L, name)).copy() for name in STATE_FIELDS}


def graph_run(spec, pol, K, replays=2):
    """vec.reset(), capture (two eager warm-up steps), vec.reset(), `replays` replays: the fragments' (obs, act, logp, rew,
    done), the warm-up's (act, done), the final state."""
    vec = SpecVec(spec)
    vec.reset()
    g = vec.capture(K, pol, True)
    g.synchronize()
    warm = (g.actions[:2].cpu().numpy().copy(), g.done[:2].cpu().numpy().copy())
    g.begin(vec.reset())
    frags = []
    for _ in range(replays):
        o, a, r, d = g.replay()
        g.synchronize()
        assert g.logp is not None and tuple(g.logp.shape) == (K, vec.num_envs)
        frags.append(tuple(t.cpu().numpy().copy() for t in (o, a, g.logp, r, d)))
    vec.torch.cuda.synchronize()
    state = state_of(vec.sim)
    vec.sim.close()
    return frags, warm, state


def eager_run(spec, pol, K, replays=2, step_kernel="k_drop_queue", policy_kernel=KERNEL):
    """The same calls in the same order on a twin handle: reset, two x (policy, step, masked reset), reset, then
    replays * K x (fs_policy_act_dev, fs_step_dev, fs_reset_dev(done))."""
    import torch
    dev = torch.device("cuda", 0)
    sim = make(spec, "f32")
    R, D, A, T = sim.R, sim.obs_dim, sim.num_rl, replays * K
    o = torch.zeros((T + 1, R, D), device=dev)
    a, lp, r = torch.zeros((T, R, A), device=dev), torch.zeros((T, R), device=dev), torch.zeros((T, R), device=dev)
    d = torch.zeros((T, R), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    sim.reset_dev(o[0], None)
    for s in range(2):                                     # (the graph's warm-up; its outputs are overwritten below)
        sim.policy_act_dev(pol.struct, o[s], a[s], lp[s])
        sim.step_dev(o[s + 1], r[s], d[s], a[s])
        sim.reset_dev(o[s + 1], d[s])
    sim.reset_dev(o[0], None)
    for s in range(T):
        sim.policy_act_dev(pol.struct, o[s], a[s], lp[s])
        assert sim.last_kernel == policy_kernel
        sim.step_dev(o[s + 1], r[s], d[s], a[s])
        assert sim.last_kernel == step_kernel
        sim.reset_dev(o[s + 1], d[s])
    sim.sync()
    out = tuple(t.cpu().numpy() for t in (o, a, lp, r, d))
    state = state_of(sim)
    sim.close()
    return out, state


def fragment_spec(**kw):
    """(Every vehicle of this network drives on SUMO's model, which has no acceleration noise here: the noise of a
    fragment is the policy's sampling.)"""
    return quiet(wide_spec(6, 141, 20, horizon=30, warmup_steps=3, seed=4, **kw))


def fragment_policies(noise, n):
    """n policies with the same weights and seed; noise off: the log std pinned at -30 (the actions are the means)."""
    pols = [make_wide_policy(141, 20, 2, not noise, seed=3, log_std=-0.7) for _ in range(n)]
    return pols if noise else [pin_log_std(p, -30.0) for p in pols]


def assert_fragments_equal_eager(frags, eager, K):
    names = ("obs", "act", "logp", "rew", "done")
    for f, frag in enumerate(frags):
        for name, x, y in zip(names, frag, eager):
            ref = y[f * K:(f + 1) * K + 1] if name == "obs" else y[f * K:(f + 1) * K]
            np.testing.assert_array_equal(x, ref, err_msg="replay %d: %s" % (f, name))


@pytest.mark.parametrize("noise", [False, True])
def test_captured_fragment_equals_eager_stepping(noise):
    K = 80
    spec = fragment_spec()
    pol_g, pol_e = fragment_policies(noise, 2)
    frags, _, state_g = graph_run(spec, pol_g, K)
    eager, state_e = eager_run(spec, pol_e, K)
    assert_fragments_equal_eager(frags, eager, K)
    for name in STATE_FIELDS:
        np.testing.assert_array_equal(state_g[name], state_e[name], err_msg=name)
    np.testing.assert_array_equal(frags[1][0][0], frags[0][0][K])            # two replays continue each other
    done = frags[0][4]
    assert ((done != 0).sum(axis=0) >= 1).all(), "a replica went through the fragment without a reset"
    assert np.isfinite(frags[0][1]).all() and np.isfinite(frags[0][2]).all()
    assert (frags[0][0][:, :, :-1] > 0).any(), "no vehicle in any observed lane-segment"


@pytest.mark.parametrize("slots", [48, 80])
def test_fragment_simulator_is_the_oracles(slots):
    """The fragment's own actions replayed through oracle/opennet.py, built as tests/test_dropq_gpu.py builds its oracle
    (cell_sum = 'fixed'), with a masked reset -- warm-up steps included -- wherever the fragment's `done` byte is not zero:
    rewards, done flags and observations bit for bit.
    Which kernel writes an observation row decides how the mean speed of a lane-segment was added up.  obs[0] comes from
    the unmasked reset, whose warm-up steps run on k_drop_queue: 'fixed'.  Every later row is written last by the masked
    fs_reset_dev that follows the step (it reports every replica, reset or not): beyond 64 slots that is k_steps_wide,
    'fixed' again; up to 64 slots it is k_steps_open, whose mean speeds are float32 sums in slot order -- the oracle's
    cell_sum = 'slot', switched on for those rows (an ulp apart in some mean speeds; tests/test_open_cpu.py bounds both
    against the float64 sum).  The simulator's state does not depend on the switch."""
    K = 80
    spec = fragment_spec(cap_human=slots - 8)
    (frag,), (warm_a, warm_d), _ = graph_run(spec, fragment_policies(True, 1)[0], K, replays=1)
    on, an, _, rn, dn = frag
    ora = O.MergeOracle(dict(spec, cell_sum="fixed"), np.float32)
    ora.reset()
    for s in range(2):                                     # the graph's warm-up, then the reset the rollout starts from
        _, _, d_ref = ora.step(warm_a[s])
        np.testing.assert_array_equal(warm_d[s] != 0, d_ref)
        if d_ref.any():
            ora.reset(d_ref)
    o_ref = ora.reset()
    np.testing.assert_array_equal(on[0], o_ref.astype(np.float32))
    if slots <= 64:
        ora.spec["cell_sum"] = "slot"
    for k in range(K):
        o_ref, r_ref, d_ref = ora.step(an[k])
        np.testing.assert_array_equal(rn[k], r_ref.astype(np.float32), err_msg="reward, step %d" % k)
        np.testing.assert_array_equal(dn[k] != 0, d_ref, err_msg="done, step %d" % k)
        if d_ref.any():
            o_ref = ora.reset(d_ref)
        np.testing.assert_array_equal(on[k + 1], o_ref.astype(np.float32), err_msg="obs, step %d" % k)
    assert (dn != 0).sum() >= spec["num_replicas"]


def with_env(name, value, fn):
    os.environ[name] = value
    try:
        return fn()
    finally:
        os.environ.pop(name)


@pytest.mark.parametrize("slots", [48, 80])
def test_mask_skip_changes_no_bit_on_the_lane_drop(slots):
    """The fragment with its masked resets (three warm-up steps each) on k_steps_open (64 lanes per replica) and on
    k_steps_wide (80 slots: a workgroup per replica), with and without FLOWSIM_NO_MASK_SKIP=1 (read by fs_create)."""
    K = 80
    spec = fragment_spec(cap_human=slots - 8)
    pols = fragment_policies(True, 2)
    skip = graph_run(spec, pols[0], K)
    full = with_env("FLOWSIM_NO_MASK_SKIP", "1", lambda: graph_run(spec, pols[1], K))
    for f, (x, y) in enumerate(zip(skip[0], full[0])):
        for name, u, v in zip(("obs", "act", "logp", "rew", "done"), x, y):
            np.testing.assert_array_equal(u, v, err_msg="replay %d: %s" % (f, name))
    for name in STATE_FIELDS:
        np.testing.assert_array_equal(skip[2][name], full[2][name], err_msg=name)
    assert (skip[0][0][4] != 0).sum() >= 6


def test_mask_skip_changes_no_bit_on_the_merge():
    """The same on a merge with warm-up steps (k_steps_open with 16 / 32 lanes per replica: several replicas per wave, a
    wave skips only when none of them is reset); the policy in the fragment is k_policy_act_vec."""
    K, A = 80, 3
    spec = merge_spec(R=6, cap_human=24, cap_rl=5, num_rl=A, horizon=30, seed=6, sims_per_step=2, q_rl=900.0,
                      noise_math="exact", warmup_steps=3)
    pols = [make_vec_policy(A, 2, True, seed=8) for _ in range(3)]
    skip = graph_run(spec, pols[0], K)
    full = with_env("FLOWSIM_NO_MASK_SKIP", "1", lambda: graph_run(spec, pols[1], K))
    for f, (x, y) in enumerate(zip(skip[0], full[0])):
        for name, u, v in zip(("obs", "act", "logp", "rew", "done"), x, y):
            np.testing.assert_array_equal(u, v, err_msg="replay %d: %s" % (f, name))
    for name in STATE_FIELDS:
        np.testing.assert_array_equal(skip[2][name], full[2][name], err_msg=name)
    done = skip[0][0][4]
    assert (done != 0).sum() >= 6 and ((done != 0).sum(axis=1) < 6).any()     # resets of some replicas, not of all
    eager, state_e = eager_run(spec, pols[2], K, step_kernel="k_merge_queue", policy_kernel="k_policy_act_vec")
    assert_fragments_equal_eager(skip[0], eager, K)
    for name in STATE_FIELDS:
        np.testing.assert_array_equal(skip[2][name], state_e[name], err_msg=name)


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_are_named():
    import torch
    dev = torch.device("cuda", 0)
    R, in_dim, A = 4, 141, 20
    spec = wide_spec(R, in_dim, A)
    pol = make_wide_policy(in_dim, A, 2, False, seed=1)

    def bufs(sim, K=3):
        out = (torch.zeros((K + 1, R, sim.obs_dim), device=dev), torch.zeros((K, R, A), device=dev),
               torch.zeros((K, R), device=dev), torch.zeros((K, R), device=dev),
               torch.zeros((K, R), dtype=torch.uint8, device=dev))
        torch.cuda.synchronize()
        return out

    sim = make(spec, "f32")
    o, a, lp, r, d = bufs(sim)
    with pytest.raises(NotImplementedError, match="VecFlowEnv.capture") as err:
        sim.policy_rollout_dev(pol.struct, 3, o, a, lp, r, d, reset_done=True)
    assert "FS_ENV_BOTTLENECK_DV" in str(err.value) and "fs_policy_rollout_dev" in str(err.value), str(err.value)
    with pytest.raises(NotImplementedError, match="fs_policy.obs_dim") as err:
        sim.policy_act_dev(make_wide_policy(65, A, 2, False, seed=1).struct, o[0], a[0], lp[0])
    assert "FS_ENV_BOTTLENECK_DV" in str(err.value), str(err.value)
    deep = make_wide_policy(in_dim, A, 3, False, seed=1)
    deep.struct.num_hidden = 4                              # (the model class: 1..3 hidden layers)
    with pytest.raises(NotImplementedError, match="fs_policy model") as err:
        sim.policy_act_dev(deep.struct, o[0], a[0], lp[0])
    assert "FS_ENV_BOTTLENECK_DV" in str(err.value), str(err.value)
    sim.policy_act_dev(pol.struct, o[0], a[0], lp[0])       # (the handle itself is fine)
    sim.sync()
    assert sim.last_kernel == KERNEL
    sim.close()
    sim = make(spec, "f64")
    o, a, lp, r, d = bufs(sim)
    with pytest.raises(NotImplementedError, match="precision") as err:
        sim.policy_act_dev(pol.struct, o[0], a[0], lp[0])
    assert "FS_ENV_BOTTLENECK_DV" in str(err.value), str(err.value)
    sim.close()


# ---- 8. the experiment -------------------------------------------------------------------------------------------------------
def singleagent_bottleneck_params():
    import copy
    import importlib
    import flow_amd
    flow_amd.install_as_flow()                     # the experiment files import `flow.*` as the reference's do
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    fp = dict(importlib.import_module("exp_configs.rl.singleagent.singleagent_bottleneck").flow_params)
    fp["sim"] = copy.deepcopy(fp["sim"])
    return fp


def test_singleagent_bottleneck_fragment_equals_its_eager_twin():
    import torch
    from flow_amd.envs import VecFlowEnv
    K, R = 60, 128
    fp = singleagent_bottleneck_params()
    fp["sim"].seed = 11                            # (the experiment ships seed = None: a seed drawn per handle)
    a_vec, b_vec = VecFlowEnv(fp, num_replicas=R, device=0), VecFlowEnv(fp, num_replicas=R, device=0)
    assert a_vec.obs_dim == 141 and a_vec.act_dim == 20 and a_vec.sim.policy_action_dim == 20 and a_vec.sim.N == 64
    pol_a, pol_b = make_wide_policy(141, 20, 2, True, seed=5), make_wide_policy(141, 20, 2, True, seed=5)
    with pytest.raises(ValueError):
        a_vec.policy_act(make_wide_policy(141, 17, 2, True, seed=5))
    a_vec.reset()
    g = a_vec.capture(K, policy=pol_a, reset_done=True)
    g.begin(a_vec.reset())
    obs, act_, rew, done = g.replay()
    g.synchronize()
    assert tuple(g.logp.shape) == (K, R) and tuple(act_.shape) == (K, R, 20)
    b_vec.use_current_stream()
    eo = torch.zeros((K + 1, R, 141), device=b_vec.device)
    eo[0].copy_(b_vec.reset())
    for s in range(2):                             # (the graph's warm-up steps, through the public calls)
        ea, elp = b_vec.policy_act(pol_b)
        _, _, ed = b_vec.step(ea)
        b_vec.reset_done()
    eo[0].copy_(b_vec.reset())
    ea, elp = torch.zeros((K, R, 20), device=b_vec.device), torch.zeros((K, R), device=b_vec.device)
    er, ed = torch.zeros((K, R), device=b_vec.device), torch.zeros((K, R), dtype=torch.uint8, device=b_vec.device)
    for s in range(K):
        b_vec.policy_act(pol_b, obs=eo[s], out=(ea[s], elp[s]))
        assert b_vec.sim.last_kernel == KERNEL
        b_vec.sim.step_dev(eo[s + 1], er[s], ed[s], ea[s])
        assert b_vec.sim.last_kernel == "k_drop_queue"
        b_vec.sim.reset_dev(eo[s + 1], ed[s])
    b_vec.sim.sync()
    for name, x, y in zip(("obs", "act", "logp", "rew", "done"), (obs, act_, g.logp, rew, done), (eo, ea, elp, er, ed)):
        np.testing.assert_array_equal(x.cpu().numpy(), y.cpu().numpy(), err_msg=name)
    for name in STATE_FIELDS:
        from flow_amd import _lib as L
        np.testing.assert_array_equal(a_vec.sim.get_state(getattr(L, name)), b_vec.sim.get_state(getattr(L, name)), err_msg=name)
    assert np.isfinite(rew.cpu().numpy()).all() and (obs.cpu().numpy()[:, :, :-1] > 0).any()
    a_vec.close(), b_vec.close()


def test_train_on_device_puts_the_policy_kernel_into_the_graph_when_asked():
    import math
    fp = singleagent_bottleneck_params()
    import train_vec
    lines = []
    hist = train_vec.train_on_device(fp, replicas=48, fragment=12, iterations=2, fuse_action_vector=True, log=lines.append)
    assert lines[0] == "rollout: HIP graph of 12 single steps around the policy kernel (%s)" % KERNEL, lines
    assert len(hist) == 2 and all(math.isfinite(h) for h in hist)
