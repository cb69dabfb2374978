"""fs_policy.greedy: the mean action in every policy kernel, held to paths that exist without it.

* A greedy call with policy P against a SAMPLING call of the same network whose log std is exactly -1000 (the free
  parameter, or the log-std rows of the head with zero weights and bias -1000: the mean rows' arithmetic is untouched):
  exp2 of that log std underflows to 0 and fma(0, g, mu) == mu, so `act` must agree bit for bit -- eagerly on every head
  (k_policy_act, _vec, _wide, shared agents with an absent one, k_policy_pair_act with the flag on one policy) and fused
  (obs, rew and done too) at K = 8 with a horizon of 5, so that resets fall inside the fragment.
* A greedy fragment equals K x (greedy act, step, reset) bit for bit.
* logp is the float32 restatement of (-log_std) - 0.9189385332046727f, the columns of an action vector added in
  ascending order, 0 for an absent agent.
* The counters advance as they do when sampling: a sampling call after a greedy call draws what the second of two
  sampling calls draws.
* greedy = 0 written into the struct is the struct as it was built before the field existed."""
import ctypes

import numpy as np
import pytest

from helpers import merge_spec
from oracle import opennet as O
from oracle import refsim as S
from test_policy_gpu import eager_obs0, fig8_rl_spec, make_policy, make_policy_in
from test_policy_merge_po_gpu import make_vec_policy
from test_policy_wide_gpu import pin_log_std
from test_ringrl_gpu import rl_ring_spec

pytestmark = pytest.mark.gpu

LOG_SQRT_2PI = np.float32(0.9189385332046727)


def make(spec, precision="f32"):
    from flow_amd.sim import FlowSim
    return FlowSim(spec, precision=precision)


def greedy(pol):
    pol.greedy = True
    assert pol.struct.greedy == 1 and pol.greedy is True
    return pol


def zero_std(pol):
    """The sampling twin: the same trunk and mean rows, log std -1000 in every column."""
    assert pol.greedy is False
    return pin_log_std(pol, -1000.0)


def logp_at_mean(log_std):
    """float32: the columns' (-log_std) - c added in ascending order ([..., A] -> [...])."""
    ls = np.asarray(log_std, dtype=np.float32)
    cols = (-ls) - LOG_SQRT_2PI
    acc = cols[..., 0]
    for c in range(1, cols.shape[-1]):
        acc = (acc + cols[..., c]).astype(np.float32)
    return acc


def call(sim, pol, obs, act_shape, lp_shape, kernel):
    import torch
    dev = torch.device("cuda", 0)
    o = torch.as_tensor(np.ascontiguousarray(obs, dtype=np.float32), device=dev)
    a, lp = torch.full(act_shape, 7.0, device=dev), torch.full(lp_shape, 7.0, device=dev)
    torch.cuda.synchronize()
    sim.policy_act_dev(pol.struct, o, a, lp)
    sim.sync()
    assert sim.last_kernel == kernel
    return a.cpu().numpy(), lp.cpu().numpy()


def rand_obs(R, D, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (R, D)).astype(np.float32)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


# ------------------------------------------------------------------------------------------------------- eager heads
def eager_case(name):
    """(sim, policy factory, obs, act shape, logp shape, kernel, columns A of a joint logp or None)"""
    if name == "ring":                                    # R = 65: a replica count that fills no wave
        R = 65
        sim = make(rl_ring_spec(R=R, N=22, seed=5))
        sim.reset()
        return sim, lambda free: make_policy(3, free, seed=9), rand_obs(R, 3, 1), (R,), (R,), "k_policy_act", None
    if name == "vec5":
        R, A = 7, 5
        sim = make(merge_spec(R=R, cap_human=24, cap_rl=A + 3, num_rl=A, horizon=40, seed=3, q_rl=1200.0, q_highway=1500.0))
        sim.reset()
        return sim, lambda free: make_vec_policy(A, 2, free, seed=4), rand_obs(R, 5 * A, 2), (R, A), (R,), "k_policy_act_vec", A
    if name == "wide13":
        from test_policy_merge_wide_gpu import wide_spec
        R, A = 6, 13
        sim = make(wide_spec(A, R=R, seed=23))
        sim.reset()
        return sim, lambda free: make_vec_policy(A, 2, free, seed=5), rand_obs(R, 5 * A, 3), (R, A), (R,), "k_policy_act_wide", A
    if name == "bottleneck":
        from test_policy_wide_gpu import make_wide_policy, wide_spec
        R, A, D = 5, 20, 141
        sim = make(wide_spec(R, D, A))
        sim.reset()
        return sim, lambda free: make_wide_policy(D, A, 2, free, seed=6), rand_obs(R, D, 4), (R, A), (R,), "k_policy_act_wide", A
    if name == "ring_ma":
        from test_multiagent_ring_gpu import ma_ring_experiment_spec
        R, slots = 9, (4, 5, 13, 21)
        sim = make(ma_ring_experiment_spec(S.ENV_WAVE_ATTENUATION_PO_MA, R, slots, noise=0.2, N=22))
        sim.reset()
        n = len(slots)
        return sim, lambda free: make_policy_in(3, 2, free, seed=7), rand_obs(R, 3 * n, 5), (R, n), (R, n), "k_policy_act", None
    raise KeyError(name)


@pytest.mark.parametrize("free", [False, True])
@pytest.mark.parametrize("name", ["ring", "vec5", "wide13", "bottleneck", "ring_ma"])
def test_eager_greedy_is_the_zero_std_sample_and_the_density_at_the_mean(name, free):
    sim, factory, obs, ashape, lshape, kernel, A = eager_case(name)
    P, Z = greedy(factory(free)), zero_std(factory(free))
    a, lp = call(sim, P, obs, ashape, lshape, kernel)
    az, _ = call(sim, Z, obs, ashape, lshape, kernel)
    assert np.isfinite(a).all() and np.abs(a).max() > 0
    np.testing.assert_array_equal(bits(a), bits(az))
    # logp: the formula in float32 -- the free log stds, or log-std rows pinned to a bias (zero weights: ls == bias exactly)
    Q = greedy(factory(free))
    if not free:
        pin_log_std(Q, -0.7)
    n = A or 1
    ls = Q.log_std_param.detach().cpu().numpy().reshape(n) if free else np.full(n, -0.7, np.float32)
    aq, lq = call(sim, Q, obs, ashape, lshape, kernel)
    want = logp_at_mean(np.broadcast_to(ls, (1, n)))[0]
    print("%s: logp at the mean %r (restated %r)" % (name, lq.reshape(-1)[0], want))
    np.testing.assert_array_equal(bits(lq), bits(np.full(lshape, want, np.float32)))
    np.testing.assert_array_equal(bits(aq), bits(a))                 # (the log std never enters the mean action)
    # an overflowing std does not reach the action either: a select, not fma(sd, 0, mu)
    pin_log_std(Q, 200.0)
    ah, lh = call(sim, Q, obs, ashape, lshape, kernel)
    np.testing.assert_array_equal(bits(ah), bits(a))
    assert np.isfinite(lh).all()
    sim.close()


@pytest.mark.parametrize("name", ["ring", "vec5", "bottleneck"])
def test_the_counters_advance_as_they_do_when_sampling(name):
    """greedy then sampling == the second of sampling, sampling (two handles, the same policy seed and observations)."""
    sim_a, factory, obs, ashape, lshape, kernel, _ = eager_case(name)
    sim_b = eager_case(name)[0]
    pa, pb = factory(False), factory(False)
    pa.greedy = True
    call(sim_a, pa, obs, ashape, lshape, kernel)
    pa.greedy = False                                                    # (the property writes the struct: no repack)
    a2, l2 = call(sim_a, pa, obs, ashape, lshape, kernel)
    b1, _ = call(sim_b, pb, obs, ashape, lshape, kernel)
    b2, lb2 = call(sim_b, pb, obs, ashape, lshape, kernel)
    assert not np.array_equal(b1, b2)
    np.testing.assert_array_equal(bits(a2), bits(b2))
    np.testing.assert_array_equal(bits(l2), bits(lb2))
    sim_a.close(), sim_b.close()


def test_an_absent_agent_of_the_merge_still_gets_nan_and_zero():
    from test_policy_merge_gpu import ma_spec, stagger
    R, n_rl = 8, 6
    spec = ma_spec(R=R, cap_human=24, cap_rl=n_rl, num_rl=n_rl, horizon=400, seed=2, sims_per_step=2, q_rl=1500.0)
    out = []
    for pol in (greedy(make_policy_in(5, 2, False, seed=4)), zero_std(make_policy_in(5, 2, False, seed=4)),
                pin_log_std(greedy(make_policy_in(5, 2, False, seed=4)), -0.7)):
        sim = make(spec)
        stagger(sim, 2, steps=40)                                        # (RL vehicles in the network in odd replicas)
        out.append(call(sim, pol, eager_obs0(sim), (R, n_rl), (R, n_rl), "k_policy_act"))
        sim.close()
    (a, lp), (az, _), (_, lq) = out
    absent = np.isnan(a)
    assert absent.any() and (~absent).any()
    np.testing.assert_array_equal(np.isnan(az), absent)
    np.testing.assert_array_equal(bits(a[~absent]), bits(az[~absent]))
    assert (lp[absent] == 0).all() and (lq[absent] == 0).all()
    np.testing.assert_array_equal(bits(lq[~absent]), bits(np.full(int((~absent).sum()), logp_at_mean([[-0.7]])[0], np.float32)))


def test_pair_act_takes_the_flag_per_policy():
    import torch
    dev = torch.device("cuda", 0)
    R, D, w = 7, 28, 0.5
    obs = rand_obs(R, D, 8)

    def run(av, adv):
        sim = make(fig8_rl_spec(R, "accel", 0.2, horizon=35, seed=4))
        sim.reset()
        o = torch.as_tensor(obs, device=dev)
        a, lp, cmd = torch.zeros((2, R), device=dev), torch.zeros((2, R), device=dev), torch.zeros((R,), device=dev)
        torch.cuda.synchronize()
        sim.policy_pair_act_dev(av.struct, adv.struct, w, o, a, lp, cmd)
        sim.sync()
        assert sim.last_kernel == "k_policy_pair_act"
        sim.close()
        return a.cpu().numpy(), lp.cpu().numpy(), cmd.cpu().numpy()
    pols = lambda: (make_policy_in(D, 3, False, seed=3), make_policy_in(D, 1, True, seed=4))      # noqa: E731
    av, adv = pols()
    a_s, lp_s, _ = run(av, adv)                                          # both sample
    av, adv = pols()
    a_g, lp_g, cmd_g = run(greedy(av), adv)                              # the av alone applies its mean
    av, adv = pols()
    a_z, _, cmd_z = run(zero_std(av), adv)
    np.testing.assert_array_equal(bits(a_g), bits(a_z))
    np.testing.assert_array_equal(bits(cmd_g), bits(cmd_z))
    np.testing.assert_array_equal(bits(a_g[1]), bits(a_s[1]))            # the adversary still samples, the same draws
    np.testing.assert_array_equal(bits(lp_g[1]), bits(lp_s[1]))
    assert not np.array_equal(a_g[0], a_s[0])
    av, adv = pols()
    a_b, lp_b, _ = run(av, greedy(adv))                                  # ... and the other way round
    np.testing.assert_array_equal(bits(a_b[0]), bits(a_s[0]))
    np.testing.assert_array_equal(bits(lp_b[1]), bits(np.full(R, logp_at_mean([[-0.7]])[0], np.float32)))


# ------------------------------------------------------------------------------------------------------ fused kernels
K_FRAG, HORIZON = 8, 5


class Fused(object):
    """One fused head: how its handle is made and prepared, its policy, its buffers and how an action row is stepped."""

    def __init__(self, name):
        self.name, self.precision, self.prepare, self.joint = name, "f32", lambda sim: sim.reset(), None
        self.min_resets = None
        if name in ("ring", "ring_mixed"):
            self.R = 48
            self.spec = rl_ring_spec(R=self.R, N=22, noise=0.2, warmup=0, horizon=HORIZON, seed=21)
            self.precision = "mixed" if name == "ring_mixed" else "f32"
            self.policy = lambda free: make_policy(3, free, seed=3)
            self.cols, self.agents, self.kernel, self.eager = None, None, "k_ring_policy", "k_policy_act"
        elif name in ("loop_po", "loop_accel"):
            self.R = 7
            head = "po" if name == "loop_po" else "accel"
            self.spec = fig8_rl_spec(self.R, head, 0.2, horizon=HORIZON, seed=4)
            D = 3 if head == "po" else 28
            self.policy = lambda free: make_policy_in(D, 3, free, seed=3)
            self.cols, self.agents, self.kernel, self.eager = None, None, "k_loop_policy", "k_policy_act"
        elif name == "loop_ma":
            from test_policy_ma_gpu import fig8_ma_spec
            self.R = 7
            self.spec = fig8_ma_spec(self.R, horizon=HORIZON, seed=4)
            self.policy = lambda free: make_policy_in(6, 2, free, seed=3)
            n = self.spec["num_rl"]
            self.cols, self.agents, self.kernel, self.eager = n, n, "k_loop_policy<AccelMA>", "k_policy_act"
        elif name == "ring_ma":
            from test_multiagent_ring_gpu import ma_ring_experiment_spec
            self.R = 9
            self.spec = ma_ring_experiment_spec(S.ENV_WAVE_ATTENUATION_PO_MA, self.R, (4, 5, 13, 21), noise=0.2, N=22)
            self.spec["warmup_steps"], self.spec["horizon"] = 0, HORIZON
            self.policy = lambda free: make_policy_in(3, 2, free, seed=3)
            self.cols, self.agents, self.kernel, self.eager = 4, 4, "k_ring_policy<POMA>", "k_policy_act"
        elif name == "merge_ma":                               # (agents present and absent; no reset inside: horizon 400)
            from test_policy_merge_gpu import ma_spec, stagger
            self.R = 8
            self.spec = ma_spec(R=self.R, cap_human=24, cap_rl=6, num_rl=6, horizon=400, seed=2, sims_per_step=2, q_rl=1500.0)
            self.prepare = lambda sim: stagger(sim, 2, steps=40)
            self.policy = lambda free: make_policy_in(5, 2, free, seed=4)
            self.cols, self.agents, self.kernel, self.eager = 6, 6, "k_merge_policy", "k_policy_act"
            self.min_resets = 0
        elif name == "merge_po":
            from test_policy_merge_po_gpu import stagger
            self.R, A = 6, 5
            self.spec = merge_spec(R=self.R, cap_human=24, cap_rl=A + 3, num_rl=A, horizon=HORIZON, seed=15, sims_per_step=2,
                                   q_rl=1200.0, q_highway=1500.0)
            self.prepare = lambda sim: stagger(sim, 3, steps=3)
            self.policy = lambda free: make_vec_policy(A, 2, free, seed=3)
            self.cols, self.agents, self.kernel, self.eager, self.joint = A, None, "k_merge_policy<PO>", "k_policy_act_vec", A
        elif name == "merge_wide":
            from test_policy_merge_po_gpu import stagger
            from test_policy_merge_wide_gpu import wide_spec
            self.R, A = 6, 13
            self.spec = wide_spec(A, R=self.R, seed=23, sims_per_step=2, horizon=HORIZON)
            self.prepare = lambda sim: stagger(sim, 3, steps=3)
            self.policy = lambda free: make_vec_policy(A, 2, free, seed=3)
            self.cols, self.agents, self.kernel, self.eager, self.joint = A, None, "k_merge_policy<PO,WIDE>", "k_policy_act_wide", A
        else:
            raise KeyError(name)
        if self.min_resets is None:
            self.min_resets = self.R

    def sim(self):
        sim = make(self.spec, self.precision)
        self.prepare(sim)
        return sim

    def buffers(self, sim, K):
        import torch
        dev, R = torch.device("cuda", 0), self.R
        ashape = (K, R) if self.cols is None else (K, R, self.cols)
        lshape = (K, R) if self.agents is None else (K, R, self.agents)
        out = (torch.zeros((K + 1, R, sim.obs_dim), device=dev), torch.zeros(ashape, device=dev), torch.zeros(lshape, device=dev),
               torch.zeros((K, R), device=dev), torch.zeros((K, R), dtype=torch.uint8, device=dev))
        torch.cuda.synchronize()
        return out

    def fused(self, pol, K=K_FRAG):
        sim = self.sim()
        out = self.buffers(sim, K)
        sim.policy_rollout_dev(pol.struct, K, *out, reset_done=True)
        sim.sync()
        assert sim.last_kernel == self.kernel
        res = [t.cpu().numpy() for t in out] + [sim.pos.copy(), sim.vel.copy()]
        sim.close()
        return res

    def eager_steps(self, pol, K=K_FRAG):
        import torch
        dev = torch.device("cuda", 0)
        sim = self.sim()
        eo, ea, elp, er, ed = out = self.buffers(sim, K)
        eo[0].copy_(torch.as_tensor(eager_obs0(sim), device=dev))
        torch.cuda.synchronize()
        for k in range(K):
            sim.policy_act_dev(pol.struct, eo[k], ea[k], elp[k])
            assert sim.last_kernel == self.eager
            sim.step_dev(eo[k + 1], er[k], ed[k], ea[k].reshape(self.R, -1))
            sim.reset_dev(eo[k + 1], ed[k])
        sim.sync()
        res = [t.cpu().numpy() for t in out] + [sim.pos.copy(), sim.vel.copy()]
        sim.close()
        return res


NAMES = ("obs", "act", "logp", "rew", "done", "pos", "vel")
FUSED = [("ring", False), ("ring", True), ("ring_mixed", False), ("loop_po", False), ("loop_accel", True), ("loop_ma", False),
         ("ring_ma", True), ("merge_ma", False), ("merge_po", False), ("merge_po", True), ("merge_wide", False),
         ("merge_wide", True)]


@pytest.mark.parametrize("name,free", FUSED)
def test_fused_greedy_fragment(name, free):
    case = Fused(name)
    g = case.fused(greedy(case.policy(free)))
    z = case.fused(zero_std(case.policy(free)))
    e = case.eager_steps(greedy(case.policy(free)))
    done = g[4]
    print("%s: %d episodes ended inside the fragment" % (name, int((done != 0).sum())))
    assert (done != 0).sum() >= case.min_resets
    for k in (0, 1, 3, 4, 5, 6):                                         # everything but logp: the zero-std sampling fragment
        np.testing.assert_array_equal(g[k], z[k], err_msg="greedy vs zero-std sample: " + NAMES[k])
    for k in range(7):                                                   # K x (greedy act, step, reset)
        np.testing.assert_array_equal(g[k], e[k], err_msg="fused vs eager: " + NAMES[k])
    act = g[1]
    present = ~np.isnan(act)
    assert present.any() and np.abs(act[present]).max() > 0
    if free:                                                             # logp: the float32 formula of the free log stds
        pol = case.policy(True)
        ls = pol.log_std_param.detach().cpu().numpy().reshape(-1)
        want = logp_at_mean(ls[None, :])[0]
        lp = g[2]
        if case.agents is None:
            np.testing.assert_array_equal(bits(lp), bits(np.full(lp.shape, want, np.float32)))
        else:                                                            # shared agents: per agent, 0 where absent
            np.testing.assert_array_equal(bits(lp), bits(np.where(present, want, np.float32(0)).astype(np.float32)))
    if name == "merge_ma":
        assert (~present).any() and (g[2][~present] == 0).all()


def test_fused_pair_greedy_fragment():
    """k_loop_policy<Adversarial>: both policies greedy against the zero-std sampling pair and against eager stepping; the
    flag on the av alone leaves the adversary sampling."""
    import torch
    from test_policy_pair_gpu import bufs, eager_fragment
    dev = torch.device("cuda", 0)
    K, R, w, D = K_FRAG, 7, 0.5, 28
    spec = fig8_rl_spec(R, "accel", 0.2, horizon=HORIZON, seed=4)
    pols = lambda: (make_policy_in(D, 3, False, seed=3), make_policy_in(D, 1, True, seed=4))      # noqa: E731

    def fused(av, adv):
        sim = make(spec)
        sim.reset()
        out = bufs(K, R, dev)
        sim.policy_pair_rollout_dev(av.struct, adv.struct, w, K, *out, reset_done=True)
        sim.sync()
        assert sim.last_kernel == "k_loop_policy<Adversarial>"
        res = [t.cpu().numpy() for t in out] + [sim.pos.copy(), sim.vel.copy()]
        sim.close()
        return res
    g = fused(*[greedy(p) for p in pols()])
    z = fused(*[zero_std(p) for p in pols()])
    assert (g[4] != 0).sum() >= R
    for k in (0, 1, 3, 4, 5, 6):
        np.testing.assert_array_equal(g[k], z[k], err_msg="greedy vs zero-std sample: " + NAMES[k])
    sim = make(spec)
    sim.reset()
    e = [t.cpu().numpy() for t in eager_fragment(sim, *[greedy(p) for p in pols()], w, K)[:5]]
    sim.close()
    for k in range(5):
        np.testing.assert_array_equal(g[k], e[k], err_msg="fused vs eager: " + NAMES[k])
    np.testing.assert_array_equal(bits(g[2][1]), bits(np.full((K, R), logp_at_mean([[-0.7]])[0], np.float32)))
    # the flag on the av alone: the adversary's first draw is the sampling pair's (the same observation, its own stream)
    av, adv = pols()
    one = fused(greedy(av), adv)
    s = fused(*pols())
    np.testing.assert_array_equal(bits(one[1][1][0]), bits(s[1][1][0]))
    np.testing.assert_array_equal(bits(one[1][0][0]), bits(g[1][0][0]))
    assert not np.array_equal(one[1][1], g[1][1])


# ------------------------------------------------------------------------------------- greedy = 0 is the struct of before
class PolicyBefore(ctypes.Structure):
    """fs_policy as it was declared before the field: four bytes of padding after `activation`."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("obs_dim", ctypes.c_int32), ("num_hidden", ctypes.c_int32),
                ("hidden_width", ctypes.c_int32), ("activation", ctypes.c_int32), ("weights_dev", ctypes.c_void_p),
                ("log_std_dev", ctypes.c_void_p), ("seed", ctypes.c_uint64)]


@pytest.mark.parametrize("name", ["ring", "loop_accel"])
def test_greedy_zero_is_the_struct_as_it_was_built_before(name):
    from flow_amd import _lib as L
    assert ctypes.sizeof(PolicyBefore) == ctypes.sizeof(L.fs_policy) == 48
    case = Fused(name)
    pol = case.policy(False)
    new = case.fused(pol)

    class Old(object):
        pass
    old = Old()
    s = pol.struct
    before = PolicyBefore(struct_size=48, obs_dim=s.obs_dim, num_hidden=s.num_hidden, hidden_width=s.hidden_width,
                          activation=s.activation, weights_dev=s.weights_dev, log_std_dev=s.log_std_dev, seed=s.seed)
    old.struct = L.fs_policy.from_buffer_copy(bytes(before))
    assert old.struct.greedy == 0 and bytes(old.struct) == bytes(pol.struct)
    was = case.fused(old)
    for k in range(7):
        np.testing.assert_array_equal(new[k], was[k], err_msg=NAMES[k])
    assert not np.array_equal(new[1], case.fused(greedy(case.policy(False)))[1])     # (and the flag does something)
