"""MergePOEnv's ONE policy with an action vector on handles with 7 to 32 places (flow_amd/csrc/flowsim_queue.h
k_merge_wide_policy, fs_last_kernel "k_merge_policy<PO,WIDE>"; eagerly k_policy_act_wide): the observation is 35 .. 160
values wide, so the first layer is policy_wide_act's (chunks of 32 inputs), and lane c of the replica's wave samples
column c from Philox column 0x40000000 + c.

* the fused fragment equals K x (fs_policy_act_dev, fs_step_dev, fs_reset_dev(done != 0)) bit for bit at every size at
  which the first layer or the column mapping changes shape, with the LAST place of rl_veh occupied;
* horizon and collision resets inside one fragment;
* the simulator inside the fragment is the oracle's;
* the network is the float64 network; the log-probability is the ascending float32 sum; the bits do not depend on the launch;
* num_rl = 6 stays on the narrow head; what is not built is refused by name, every message naming FS_ENV_MERGE_PO;
* EXP_NUM 1 and 2 of singleagent_merge.py as shipped, train_on_device(fuse_action_vector=True), VecFlowEnv.capture.

The helpers are test_policy_merge_po_gpu.py's and test_policy_wide_gpu.py's.  eager_fragment and fused_and_eager are
written again here: theirs assert the narrow head's kernel names."""
import os
import sys

import numpy as np
import pytest

from helpers import merge_layout, merge_spec
from oracle import opennet as O
from oracle import refsim as S
from test_open_gpu import quiet
from test_policy_gpu import eager_obs0
from test_policy_merge_po_gpu import STATE_FIELDS, assert_same_state, buffers, make, make_vec_policy, stagger
from test_policy_wide_gpu import numpy_net, pin_log_std

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "k_merge_policy<PO,WIDE>"
EAGER = "k_policy_act_wide"


def wide_spec(num_rl, R=6, humans=6, spacing=13.0, speed=6.0, **kw):
    """A merge whose every place of rl_veh is taken from the first step on: num_rl RL vehicles stand on the highway at
    reset, `spacing` metres apart behind the merge point (the list fills in slot order with the first
    additional_command, and an initial vehicle that is placed again keeps its place: oracle/opennet.py reset), two humans
    ahead of them, and an all-RL highway inflow behind.  pre = 400: 500 m of highway before the merge point."""
    kw.setdefault("horizon", 25)
    kw.setdefault("q_highway", 300.0)
    kw.setdefault("q_rl", 1500.0)
    spec = merge_spec(R=R, cap_human=humans, cap_rl=num_rl + 2, num_rl=num_rl, pre=400.0, **kw)
    m = spec["merge_x"]
    lay = {0: (m + 60.0, 12.0, 0), 1: (m + 25.0, 10.0, 0)}
    lay.update({humans + k: (m - 15.0 - spacing * k, speed, 0) for k in range(num_rl)})
    spec.update(merge_layout(spec, lay))
    return spec


def eager_fragment(sim, pol, K, obs0):
    """K x (fs_policy_act_dev, fs_step_dev, fs_reset_dev(done != 0)) from the observation obs0."""
    import torch
    e = buffers(K, sim.R, sim.obs_dim, sim.num_rl)
    eo, ea, elp, er, ed = e
    eo[0].copy_(obs0)
    torch.cuda.synchronize()
    for s in range(K):
        sim.policy_act_dev(pol.struct, eo[s], ea[s], elp[s])
        assert sim.last_kernel == EAGER
        sim.step_dev(eo[s + 1], er[s], ed[s], ea[s])
        assert sim.last_kernel == "k_merge_queue"
        sim.reset_dev(eo[s + 1], ed[s])               # (the mask is the flag byte: horizon or collision)
    sim.sync()
    return e


def fused_and_eager(spec, num_hidden, free, K, precision="f32", seed=3, staggered=True):
    """The same fragment three times: one fs_policy_rollout_dev launch of K steps, two of K / 2, and eagerly."""
    import torch
    dev = torch.device("cuda", 0)
    R, A = spec["num_replicas"], spec["num_rl"]
    pols = [make_vec_policy(A, num_hidden, free, seed=seed) for _ in range(3)]
    sims = [make(spec, precision) for _ in range(3)]
    for sim in sims:
        if staggered:
            stagger(sim, seed)
        else:
            sim.reset()
    fused, halves, eager = sims
    D = fused.obs_dim
    assert D == 5 * A and fused.policy_action_dim == A and fused.policy_agents == 1
    f = buffers(K, R, D, A)
    fused.policy_rollout_dev(pols[0].struct, K, *f, reset_done=True)
    fused.sync()
    assert fused.last_kernel == KERNEL
    e = eager_fragment(eager, pols[2], K, torch.as_tensor(eager_obs0(eager), device=dev))
    for name, x, y in zip(("obs", "act", "logp", "rew", "done"), f, e):
        np.testing.assert_array_equal(x.cpu().numpy(), y.cpu().numpy(), err_msg=name)
    assert_same_state(fused, eager)
    K1 = K // 2                                       # stream continuation: two fragments of K / 2
    h1, h2 = buffers(K1, R, D, A), buffers(K - K1, R, D, A)
    halves.policy_rollout_dev(pols[1].struct, K1, *h1, reset_done=True)
    halves.policy_rollout_dev(pols[1].struct, K - K1, *h2, reset_done=True)
    halves.sync()
    assert halves.last_kernel == KERNEL
    for name, x, y1, y2 in zip(("obs", "act", "logp", "rew", "done"), f, h1, h2):
        x = x.cpu().numpy()
        lo = K1 + 1 if name == "obs" else K1
        np.testing.assert_array_equal(x[:lo], y1.cpu().numpy(), err_msg="first half: " + name)
        np.testing.assert_array_equal(x[K1:], y2.cpu().numpy(), err_msg="second half: " + name)
    assert_same_state(fused, halves, "halves: ")
    halves.close()
    return fused, eager, pols[0], f


def assert_last_place_is_live(o, a, A):
    """A vehicle that moves stands at place A - 1 of rl_veh somewhere in the fragment (its speed / max_speed is positive:
    an empty place reads 0, a ghost -1001 / max_speed), and the column that commands it is sampled there."""
    on, an = o.cpu().numpy(), a.cpu().numpy()
    live = on[:-1, :, 5 * (A - 1)] > 0
    print("place %d holds a moving vehicle in %d of %d (step, replica) pairs" % (A - 1, int(live.sum()), live.size))
    assert live.any(), "the last place of rl_veh is never occupied"
    assert np.isfinite(an[:, :, A - 1][live]).all() and (np.abs(an[:, :, A - 1][live]) > 0).all()
    assert (np.abs(on[:, :, 5 * (A - 1):]) > 0).any()


# 7: 35 inputs (two chunks, the second of 3); 13: 65 (a third chunk of 1); 17: the columns reach the second 16-lane row;
# 26: 130 inputs (five chunks: a second pass for row 0); 32: 160 inputs, full chunks, two full rows of columns -- the cap
@pytest.mark.parametrize("num_rl,num_hidden,free,precision,noise,sims", [
    (7, 1, True, "f32", True, 1), (13, 2, False, "f32", False, 5), (17, 3, True, "f32", True, 5),
    (26, 2, False, "f32", True, 1), (32, 3, False, "f32", False, 5), (32, 1, True, "f32", True, 1),
    (13, 2, True, "f16s", True, 5)])
def test_fused_fragment_equals_eager_stepping(num_rl, num_hidden, free, precision, noise, sims):
    K, R = 60, 6
    spec = wide_spec(num_rl, R=R, seed=10 + num_rl, sims_per_step=sims, noise_math="exact" if num_hidden == 2 else "hw")
    if not noise:
        spec = quiet(spec)
    fused, eager, pol, (o, a, lp, r, d) = fused_and_eager(spec, num_hidden, free, K, precision)
    dn = d.cpu().numpy()
    assert ((dn != 0).sum(axis=0) >= 1).all(), "a replica went through the fragment without a reset"
    assert np.isfinite(a.cpu().numpy()).all() and np.isfinite(lp.cpu().numpy()).all()
    assert_last_place_is_live(o, a, num_rl)
    fused.close(), eager.close()


def reset_spec():
    """13 places, the vehicles 12 m apart and free to run into each other (speed mode 0), a collision declared below a
    gap of 2 m, strong noise on the humans, and a horizon of 8 steps.  The first collision of an episode comes after 6
    to 9 steps (the numpy oracle driven by this test's network with numpy normal draws: 14 to 26 collision resets and
    32 to 43 horizon resets in 60 steps of 8 replicas), so some episodes end one way and some the other."""
    spec = wide_spec(13, R=8, spacing=12.0, speed=8.0, horizon=8, seed=4, sims_per_step=2, noise_math="exact",
                     crash_gap=2.0, q_merge=900.0)
    spec["vehicles"] = [dict(v, speed_mode=0, noise=1.5 if v["noise"] > 0 else 0.0) for v in spec["vehicles"]]
    return spec


def test_collisions_and_horizons_reset_inside_the_fragment():
    fused, eager, pol, (o, a, lp, r, d) = fused_and_eager(reset_spec(), 2, False, 60, staggered=False)
    dn, rn = d.cpu().numpy(), r.cpu().numpy()
    collisions, horizons = int(((dn & 2) != 0).sum()), int(((dn & 1) != 0).sum())
    print("collision resets %d, horizon resets %d" % (collisions, horizons))
    assert collisions >= 1 and horizons >= 1
    assert (rn[(dn & 2) != 0] == 0).all()                # (a collision: reward 0)
    assert_last_place_is_live(o, a, 13)
    fused.close(), eager.close()


@pytest.mark.parametrize("noise", [False, True])
def test_fragment_simulator_is_the_oracles(noise):
    """The fragment's own actions replayed through oracle/opennet.py as an action tape, with a masked reset wherever the
    fragment's `done` byte is not zero: the same observations, rewards and done flags, bit for bit."""
    K, R, A = 60, 4, 13
    spec = wide_spec(A, R=R, seed=6, sims_per_step=3, noise_math="exact")
    if not noise:
        spec = quiet(spec)
    sim, ora = make(spec), O.MergeOracle(spec, np.float32)
    sim.reset()
    o_ref = ora.reset()
    pol = make_vec_policy(A, 3, True, seed=8)
    o, a, lp, r, d = buffers(K, R, sim.obs_dim, A)
    sim.policy_rollout_dev(pol.struct, K, o, a, lp, r, d, reset_done=True)
    sim.sync()
    assert sim.last_kernel == KERNEL
    on, an, rn, dn = o.cpu().numpy(), a.cpu().numpy(), r.cpu().numpy(), d.cpu().numpy()
    np.testing.assert_array_equal(on[0], o_ref.astype(np.float32))
    for k in range(K):
        o_ref, r_ref, d_ref = ora.step(an[k])
        np.testing.assert_array_equal(rn[k], r_ref.astype(np.float32), err_msg="reward, step %d" % k)
        np.testing.assert_array_equal(dn[k] != 0, d_ref, err_msg="done, step %d" % k)
        if d_ref.any():
            o_ref = ora.reset(d_ref)
        np.testing.assert_array_equal(on[k + 1], o_ref.astype(np.float32), err_msg="obs, step %d" % k)
    assert (dn != 0).sum() >= R
    np.testing.assert_array_equal(sim.time_counter, ora.time_counter)
    assert_last_place_is_live(o, a, A)
    sim.close()


def act_once(spec, pol, obs):
    """One fs_policy_act_dev call on a fresh handle (the replicas' counters at zero): numpy (act [R, A], logp [R])."""
    import torch
    dev = torch.device("cuda", 0)
    sim = make(spec)
    sim.reset()
    o = torch.as_tensor(np.ascontiguousarray(obs, dtype=np.float32), device=dev)
    a, lp = torch.zeros((sim.R, sim.num_rl), device=dev), torch.zeros((sim.R,), device=dev)
    torch.cuda.synchronize()
    sim.policy_act_dev(pol.struct, o, a, lp)
    sim.sync()
    assert sim.last_kernel == EAGER
    sim.close()
    return a.cpu().numpy(), lp.cpu().numpy()


def random_obs(R, in_dim, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (R, in_dim)).astype(np.float32)


@pytest.mark.parametrize("A,num_hidden,free", [(7, 1, True), (17, 3, False), (32, 2, True)])
def test_the_net_is_the_network(A, num_hidden, free):
    """Log std -30: the action is the kernel's mean, which must be the float64 network's in every column at atol 2e-5 (the
    bar of test_policy_merge_po_gpu.py::test_the_net_is_the_torch_net and test_policy_wide_gpu.py::
    test_the_net_is_the_network, justified there).  Zeroing input 31 (the last of chunk 0), input 32 (the first of chunk
    1) and the last input must each move the means, and the moved means must be the network's again."""
    R, D = 64, 5 * A
    spec = merge_spec(R=R, cap_human=12, cap_rl=A, num_rl=A, horizon=100, seed=1)
    pol = pin_log_std(make_vec_policy(A, num_hidden, free, seed=num_hidden + A), -30.0)
    obs = random_obs(R, D, D + A)
    a, _ = act_once(spec, pol, obs)
    mu, _ = numpy_net(pol, obs)
    print("A %d: max |kernel - float64| = %.3g" % (A, np.abs(a - mu).max()))
    np.testing.assert_allclose(a, mu, atol=2e-5, rtol=0)
    assert np.abs(mu[:, 0] - mu[:, A - 1]).max() > 1e-2 and np.abs(a[:, 0] - a[:, A - 1]).max() > 1e-2
    for i in (31, 32, D - 1):
        obs0 = obs.copy()
        obs0[:, i] = 0.0
        a0, _ = act_once(spec, pol, obs0)
        mu0, _ = numpy_net(pol, obs0)
        np.testing.assert_allclose(a0, mu0, atol=2e-5, rtol=0, err_msg="input %d zeroed" % i)
        assert np.abs(a0 - a).max() > 1e-3, "input %d does not reach the means" % i
        assert np.abs(mu0 - mu).max() > 1e-3


@pytest.mark.parametrize("A,free", [(17, True), (32, False), (32, True)])
def test_log_probability_is_the_float32_ascending_sum_over_the_columns(A, free):
    """The method of test_policy_wide_gpu.py::test_log_probability_is_the_float32_ascending_sum_over_the_columns at its
    atol 1e-5: g recovered from the kernel's own action, its mean (the same trunk and mean rows with the log std at -30, a
    second handle at the same counter) and the log std (the free parameter, or the float64 network's).  The log stds lie
    near -1.4, where a column's expected log-probability is about zero and the sum stays where float32 resolves 1e-6."""
    import torch
    R, D = 256, 5 * A
    spec = merge_spec(R=R, cap_human=12, cap_rl=A, num_rl=A, horizon=100, seed=2)
    pol = make_vec_policy(A, 2, free, seed=11, log_std=-1.4)
    with torch.no_grad():
        if free:                                      # (make_vec_policy's slope of 0.05 per column: 0.002 here)
            pol.log_std_param.copy_(-1.4 + 0.002 * torch.arange(A, device=pol.log_std_param.device))
        else:                                         # the network's own log stds: small weights around a bias of -1.4
            pol.head.weight[A:].mul_(0.1)
            pol.head.bias[A:].fill_(-1.4)
    pol.sync()
    obs = random_obs(R, D, 5)
    a, lp = act_once(spec, pol, obs)
    mean_pol = make_vec_policy(A, 2, True, seed=11, log_std=-30.0)
    with torch.no_grad():
        mean_pol.log_std_param.fill_(-30.0)
        mean_pol.head.weight.copy_(pol.head.weight[:A])
        mean_pol.head.bias.copy_(pol.head.bias[:A])
        for l_dst, l_src in zip(mean_pol.hidden, pol.hidden):
            l_dst.weight.copy_(l_src.weight)
            l_dst.bias.copy_(l_src.bias)
    mean_pol.struct.seed = pol.struct.seed
    mean_pol.sync()
    mu, _ = act_once(spec, mean_pol, obs)
    _, ls = numpy_net(pol, obs)
    g = (a.astype(np.float64) - mu.astype(np.float64)) / np.exp(ls)
    per_col = (-0.5 * g * g - ls - 0.9189385332046727).astype(np.float32)
    ref = per_col[:, 0].copy()
    for c in range(1, A):
        ref = (ref + per_col[:, c]).astype(np.float32)
    assert 2.0 < np.abs(g).max() < 6.0 and abs(g.mean()) < 0.1 and 0.9 < g.std() < 1.1        # standard normal draws
    assert np.abs(g[:, 0] - g[:, A - 1]).max() > 0.5                                          # the columns' own streams
    print("A %d: max |logp - ref| = %.3g" % (A, np.abs(lp - ref).max()))
    np.testing.assert_allclose(lp, ref, atol=1e-5, rtol=0)


def test_bits_do_not_depend_on_the_launch():
    """The same observation row at replica 0 and at the last replica of R = 3 and of R = 130 (k_policy_act_wide puts four
    replicas into a workgroup: the last one of 3 and of 130 sit in different waves of theirs), log std -60: identical
    actions.  And a handle with a replica offset reproduces the rows of the big handle from that offset on."""
    A, big, lo = 17, 130, 125
    D = 5 * A
    row = random_obs(1, D, 9)[0]
    mean_pol = pin_log_std(make_vec_policy(A, 2, False, seed=4), -60.0)
    got = []
    for R in (3, big):
        obs = random_obs(R, D, R)
        obs[0], obs[R - 1] = row, row
        a, _ = act_once(merge_spec(R=R, cap_human=12, cap_rl=A, num_rl=A, horizon=100, seed=1), mean_pol, obs)
        got += [a[0], a[R - 1]]
    for x in got[1:]:
        np.testing.assert_array_equal(x, got[0])
    assert np.abs(got[0]).max() > 1e-3
    pol = make_vec_policy(A, 2, True, seed=5)
    obs = random_obs(big, D, 21)
    a, lp = act_once(merge_spec(R=big, cap_human=12, cap_rl=A, num_rl=A, horizon=100, seed=1), pol, obs)
    b, lq = act_once(merge_spec(R=big - lo, cap_human=12, cap_rl=A, num_rl=A, horizon=100, seed=1, replica_offset=lo), pol,
                     obs[lo:])
    np.testing.assert_array_equal(a[lo:], b)
    np.testing.assert_array_equal(lp[lo:], lq)
    assert np.abs(a[lo:] - a[:big - lo]).max() > 1e-2            # (other replicas: other draws)


def test_the_narrow_head_is_untouched():
    import torch
    dev = torch.device("cuda", 0)
    spec = merge_spec(R=4, cap_human=12, cap_rl=8, num_rl=6, horizon=100, seed=1)
    sim, pol = make(spec), make_vec_policy(6, 2, False, seed=1)
    sim.reset()
    o, a, lp, r, d = buffers(3, 4, sim.obs_dim, 6)
    sim.policy_act_dev(pol.struct, torch.as_tensor(eager_obs0(sim), device=dev), a[0], lp[0])
    sim.sync()
    assert sim.last_kernel == "k_policy_act_vec"
    sim.policy_rollout_dev(pol.struct, 3, o, a, lp, r, d, reset_done=True)
    sim.sync()
    assert sim.last_kernel == "k_merge_policy<PO>"
    sim.close()


def test_refusals_are_named():
    A = 13
    spec = merge_spec(R=4, cap_human=12, cap_rl=A + 1, num_rl=A, horizon=100, seed=1)
    pol = make_vec_policy(A, 2, False, seed=1)
    cases = [(make(dict(spec, warmup_steps=3)), pol, "warmup_steps = 0"),
             (make(spec, "f64"), pol, "FS_MIXED / FS_F64"),
             (make(dict(spec, inflows=[dict(f, probability=0.3) for f in spec["inflows"]])), pol, "queue_ok"),
             (make(dict(spec, vehicles=[dict(v, fail_safe=1) if v["controller"] == S.CTRL_IDM else v
                                        for v in spec["vehicles"]])), pol, "queue_ok"),
             (make(spec), make_vec_policy(12, 2, False, seed=1), "fs_policy.obs_dim"),
             (make(spec), make_vec_policy(6, 2, False, seed=1), "fs_policy.obs_dim")]
    os.environ["FLOWSIM_NO_QUEUE"] = "1"
    try:
        cases.append((make(spec), pol, "queue_ok"))
    finally:
        os.environ.pop("FLOWSIM_NO_QUEUE")
    for sim, p, msg in cases:
        sim.reset()
        o, a, lp, r, d = buffers(3, 4, sim.obs_dim, A)
        with pytest.raises(NotImplementedError, match=msg) as err:
            sim.policy_rollout_dev(p.struct, 3, o, a, lp, r, d, reset_done=True)
        assert "FS_ENV_MERGE_PO" in str(err.value), str(err.value)
        if msg != "warmup_steps = 0":              # (the eager policy has no resets to refuse)
            with pytest.raises(NotImplementedError, match=msg) as err:
                sim.policy_act_dev(p.struct, o[0], a[0], lp[0])
            assert "FS_ENV_MERGE_PO" in str(err.value), str(err.value)
        sim.close()


def singleagent_merge_params(exp):
    """flow_params of singleagent_merge.py with EXP_NUM = exp, the way test_singleagent_merge_config.py loads them."""
    import copy
    import flow_amd
    flow_amd.install_as_flow()                     # the experiment files import `flow.*` as the reference's do
    if os.path.join(ROOT, "examples") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "examples"))
    path = os.path.join(ROOT, "examples", "exp_configs", "rl", "singleagent", "singleagent_merge.py")
    with open(path) as f:
        text = f.read()
    assert text.count("EXP_NUM = 0\n") == 1
    scope = {"__name__": "singleagent_merge_exp%d" % exp}
    exec(compile(text.replace("EXP_NUM = 0\n", "EXP_NUM = %d\n" % exp), path, "exec"), scope)
    fp = dict(scope["flow_params"])
    fp["sim"] = copy.deepcopy(fp["sim"])
    return fp


@pytest.mark.parametrize("exp,A", [(1, 13), (2, 17)])
def test_shipped_experiment_fused_equals_eager(exp, A):
    """EXP_NUM 1 and 2 of singleagent_merge.py as shipped at 256 replicas: one fused fragment through
    VecFlowEnv.policy_rollout equals eager stepping on every replica."""
    from flow_amd.envs import VecFlowEnv
    K, R = 100, 256
    fp = singleagent_merge_params(exp)
    fp["sim"].seed = 11                            # (the experiment ships seed = None: a seed drawn per handle)
    a_vec, b_vec = VecFlowEnv(fp, num_replicas=R, device=0), VecFlowEnv(fp, num_replicas=R, device=0)
    assert a_vec.act_dim == A and a_vec.obs_dim == 5 * A and a_vec.sim.policy_action_dim == A
    obs0 = a_vec.reset().clone()
    b_vec.reset()
    pol_a, pol_b = make_vec_policy(A, 2, True, seed=5), make_vec_policy(A, 2, True, seed=5)
    obs, act, logp, rew, done = a_vec.policy_rollout(pol_a, K, reset_done=True)
    a_vec.sim.sync()
    assert a_vec.sim.last_kernel == KERNEL
    assert tuple(obs.shape) == (K + 1, R, 5 * A) and tuple(act.shape) == (K, R, A) and tuple(logp.shape) == (K, R)
    assert tuple(rew.shape) == (K, R) and tuple(done.shape) == (K, R)
    b_vec.use_current_stream()
    e = eager_fragment(b_vec.sim, pol_b, K, obs0)
    for name, x, y in zip(("obs", "act", "logp", "rew", "done"), (obs, act, logp, rew, done), e):
        np.testing.assert_array_equal(x.cpu().numpy(), y.cpu().numpy(), err_msg=name)
    assert_same_state(a_vec.sim, b_vec.sim)
    assert np.isfinite(rew.cpu().numpy()).all() and (rew.cpu().numpy() > 0).any()
    a_vec.close(), b_vec.close()


def test_train_on_device_fuses_the_wide_policy_when_asked():
    import math
    fp = singleagent_merge_params(1)
    import train_vec
    lines = []
    hist = train_vec.train_on_device(fp, replicas=48, fragment=12, iterations=2, fuse_action_vector=True, log=lines.append)
    assert lines[0] == "rollout: fused policy + step kernel (%s)" % KERNEL, lines
    assert len(hist) == 2 and all(math.isfinite(h) for h in hist)


def test_captured_fragment_with_the_device_policy_equals_eager_stepping():
    """VecFlowEnv.capture(K, policy=DevicePolicy, reset_done=True) at 13 places: K x (k_policy_act_wide, k_merge_queue,
    masked reset) in one graph equals the same calls made eagerly, and graph.logp holds the joint log-probabilities."""
    from test_policy_wide_gpu import assert_fragments_equal_eager, eager_run, graph_run
    K, A = 40, 13
    spec = wide_spec(A, R=6, seed=5, sims_per_step=2, noise_math="exact")
    pol_g, pol_e = make_vec_policy(A, 2, True, seed=8), make_vec_policy(A, 2, True, seed=8)
    frags, _, state_g = graph_run(spec, pol_g, K)
    eager, state_e = eager_run(spec, pol_e, K, step_kernel="k_merge_queue", policy_kernel=EAGER)
    assert_fragments_equal_eager(frags, eager, K)
    for name in STATE_FIELDS:
        np.testing.assert_array_equal(state_g[name], state_e[name], err_msg=name)
    logp = frags[0][2]
    assert logp.shape == (K, 6) and np.isfinite(logp).all() and np.abs(logp).max() > 1.0
    assert ((frags[0][4] != 0).sum(axis=0) >= 1).all()
    assert (frags[0][0][:-1, :, 5 * (A - 1)] > 0).any()
