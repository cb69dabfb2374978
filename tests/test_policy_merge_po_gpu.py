"""MergePOEnv's ONE policy with an action vector, in the loop (flow_amd/csrc/flowsim_queue.h k_merge_policy, fs_last_kernel
"k_merge_policy<PO>"; flow_amd/csrc/flowsim_policy.h policy_vec_act): the network maps the whole observation (5 num_rl
values) to num_rl accelerations once per step; column c draws from Philox column 0x40000000 + c.

* the fused fragment equals K x (fs_policy_act_dev, fs_step_dev, fs_reset_dev(done != 0)) bit for bit -- collisions, which
  end the episode on this head, included -- and two fragments of K / 2 steps equal one of K;
* the simulator inside the fragment is the oracle's (the fragment's actions replayed as an action tape, with its resets);
* the network is the torch network (DevicePolicy.reference), every input and every column;
* the log-probability is the float32 sum over the columns of the 1-d formula;
* what is not built is refused by name, every message naming FS_ENV_MERGE_PO;
* singleagent_merge.py as shipped at 1024 replicas, and train_on_device(fuse_action_vector=True)."""
import os
import sys

import numpy as np
import pytest

from helpers import merge_spec
from oracle import opennet as O
from oracle import refsim as S
from test_open_gpu import quiet
from test_policy_gpu import eager_obs0

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "k_merge_policy<PO>"


def make(spec, precision="f32"):
    from flow_amd.sim import FlowSim
    return FlowSim(spec, precision=precision)


def make_vec_policy(A, num_hidden=2, free=False, seed=0, log_std=-0.7, dev="cuda:0"):
    """5 A inputs -> 1..3 x 32 tanh -> A means [+ A log stds]; free: a log std parameter of A elements."""
    import torch
    from flow_amd.utils.device_policy import DevicePolicy
    g = torch.Generator().manual_seed(seed)
    dims = [5 * A] + [32] * num_hidden
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
    ls = torch.nn.Parameter(torch.full((A,), float(log_std), device=dev) + 0.05 * torch.arange(A, device=dev)) if free else None
    return DevicePolicy(hidden, head, log_std=ls, seed=77 + seed, act_dim=A)


def buffers(K, R, D, A):
    import torch
    dev = torch.device("cuda", 0)
    out = (torch.zeros((K + 1, R, D), device=dev), torch.zeros((K, R, A), device=dev), torch.zeros((K, R), device=dev),
           torch.zeros((K, R), device=dev), torch.zeros((K, R), dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()          # (the handles launch on streams of their own)
    return out


def stagger(sim, seed, steps=9):
    """A few open-loop steps, then a masked reset of every other replica: the replicas' episodes end at different steps."""
    import torch
    dev = torch.device("cuda", 0)
    R, A = sim.R, sim.num_rl
    rng = np.random.default_rng(seed)
    acts = torch.from_numpy(rng.uniform(-1.0, 1.0, (steps, R, A)).astype(np.float32)).to(dev)
    o, r, d = (torch.zeros((steps, R, sim.obs_dim), device=dev), torch.zeros((steps, R), device=dev),
               torch.zeros((steps, R), dtype=torch.uint8, device=dev))
    sim.reset()
    sim.rollout_dev(steps, o, r, d, actions=acts)
    m = torch.from_numpy((np.arange(R) % 2 == 0).astype(np.uint8)).to(dev)
    sim.reset_dev(o[0], m)
    sim.sync()


def eager_fragment(sim, pol, K, obs0):
    """K x (fs_policy_act_dev, fs_step_dev, fs_reset_dev(done != 0)) from the observation obs0."""
    import torch
    e = buffers(K, sim.R, sim.obs_dim, sim.num_rl)
    eo, ea, elp, er, ed = e
    eo[0].copy_(obs0)
    torch.cuda.synchronize()
    for s in range(K):
        sim.policy_act_dev(pol.struct, eo[s], ea[s], elp[s])
        assert sim.last_kernel == "k_policy_act_vec"
        sim.step_dev(eo[s + 1], er[s], ed[s], ea[s])
        sim.reset_dev(eo[s + 1], ed[s])               # (the mask is the flag byte: horizon or collision)
    sim.sync()
    return e


STATE_FIELDS = ("FS_FIELD_POS", "FS_FIELD_VEL", "FS_FIELD_ROUTE", "FS_FIELD_SEQ", "FS_FIELD_CTL_SEQ", "FS_FIELD_COUNTERS",
                "FS_FIELD_TIME")


def assert_same_state(a, b, msg=""):
    from flow_amd import _lib as L
    for name in STATE_FIELDS:
        np.testing.assert_array_equal(a.get_state(getattr(L, name)), b.get_state(getattr(L, name)), err_msg=msg + name)


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
    # stream continuation: two fragments of K / 2
    K1 = K // 2
    h1, h2 = buffers(K1, R, D, A), buffers(K - K1, R, D, A)
    halves.policy_rollout_dev(pols[1].struct, K1, *h1, reset_done=True)
    halves.policy_rollout_dev(pols[1].struct, K - K1, *h2, reset_done=True)
    halves.sync()
    assert halves.last_kernel == KERNEL
    np.testing.assert_array_equal(h2[0][0].cpu().numpy(), h1[0][K1].cpu().numpy())
    for name, x, y1, y2 in zip(("obs", "act", "logp", "rew", "done"), f, h1, h2):
        x = x.cpu().numpy()
        if name == "obs":
            np.testing.assert_array_equal(x[:K1 + 1], y1.cpu().numpy(), err_msg="first half: obs")
            np.testing.assert_array_equal(x[K1:], y2.cpu().numpy(), err_msg="second half: obs")
        else:
            np.testing.assert_array_equal(x[:K1], y1.cpu().numpy(), err_msg="first half: " + name)
            np.testing.assert_array_equal(x[K1:], y2.cpu().numpy(), err_msg="second half: " + name)
    assert_same_state(fused, halves, "halves: ")
    halves.close()
    return fused, eager, pols[0], f


@pytest.mark.parametrize("num_rl,num_hidden,free,precision,noise,sims", [
    (1, 1, True, "f32", True, 1), (2, 2, False, "f32", False, 5), (5, 3, False, "f32", True, 5),
    (6, 2, True, "f32", True, 2), (5, 2, True, "f16s", True, 5), (6, 3, False, "f16s", False, 1),
    (2, 1, False, "f16s", True, 2), (1, 3, True, "f32", False, 5)])
def test_fused_fragment_equals_eager_stepping(num_rl, num_hidden, free, precision, noise, sims):
    K, R = 90, 6
    spec = merge_spec(R=R, cap_human=24, cap_rl=num_rl + 3, num_rl=num_rl, horizon=40, seed=10 + num_rl, sims_per_step=sims,
                      q_rl=1200.0, q_highway=1500.0, noise_math="exact" if num_hidden == 2 else "hw")
    if not noise:
        spec = quiet(spec)
    fused, eager, pol, (o, a, lp, r, d) = fused_and_eager(spec, num_hidden, free, K, precision)
    dn, an = d.cpu().numpy(), a.cpu().numpy()
    assert ((dn != 0).sum(axis=0) >= 1).all(), "a replica went through the fragment without a reset"
    assert np.isfinite(an).all() and np.isfinite(lp.cpu().numpy()).all()       # (no absent / NaN logic on this head)
    assert (np.abs(o.cpu().numpy()[:, :, 0::5]) > 0).any(), "no controlled vehicle in any observation"
    fused.close(), eager.close()


def test_collisions_and_horizons_reset_inside_the_fragment():
    """The shape of test_queue_po_gpu.py::test_po_collisions_end_the_env_step (speed mode 0 everywhere: nothing keeps the
    vehicles apart) with a short horizon: collisions (bit 1 of `done`) and horizons (bit 0) both reset a replica in place,
    and the list of controlled vehicles outlives the resets (ghost rows: the accessors' error values).  The first
    collision of an episode is the ramp's first vehicle meeting the highway's in the junction, around step 76 whatever
    the actions; the humans' noise (sigma 1.5 here) spreads it over the replicas, so with the horizon at 80 some episodes
    end one way and some the other (the numpy oracle with random actions: 34 collisions and 16 horizons in 300 steps of
    16 replicas, and no fewer than 5 of either for horizons from 70 to 90)."""
    seed = 3
    spec = merge_spec(R=16, cap_human=18 + seed, cap_rl=4, num_rl=3, horizon=80, seed=seed, pre=150.0,
                      q_highway=1500 + 100 * seed, q_merge=200 + 80 * seed, q_rl=1500.0, sims_per_step=1 + seed % 3,
                      noise_math="exact")
    spec["vehicles"] = [dict(v, speed_mode=0, noise=1.5 if v["noise"] > 0 else 0.0) for v in spec["vehicles"]]
    fused, eager, pol, (o, a, lp, r, d) = fused_and_eager(spec, 2, False, 300, staggered=False)
    dn, on, rn = d.cpu().numpy(), o.cpu().numpy(), r.cpu().numpy()
    collisions, horizons = int(((dn & 2) != 0).sum()), int(((dn & 1) != 0).sum())
    ghosts = int((on[:, :, 0::5] < -30).sum())
    print("collision resets %d, horizon resets %d, ghost rows %d" % (collisions, horizons, ghosts))
    assert collisions >= 1 and horizons >= 1
    assert (rn[(dn & 2) != 0] == 0).all()                # (a collision: reward 0)
    assert ghosts >= 1
    fused.close(), eager.close()


@pytest.mark.parametrize("noise", [False, True])
def test_fragment_simulator_is_the_oracles(noise):
    """The fragment's own actions replayed through oracle/opennet.py, with a masked reset wherever the fragment's `done`
    byte is not zero, reproduce its observations, rewards and done flags bit for bit (noise: noise_math = 'exact' makes
    the draws fixed float32 sequences, the same in the numpy oracle)."""
    K, R, A = 80, 4, 3
    spec = merge_spec(R=R, cap_human=24, cap_rl=5, num_rl=A, horizon=35, seed=6, sims_per_step=3, q_rl=900.0,
                      noise_math="exact")
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
    sim.close()


def act_once(spec, pol, obs):
    """One fs_policy_act_dev call on a fresh handle (the replicas' counters at zero)."""
    import torch
    dev = torch.device("cuda", 0)
    sim = make(spec)
    sim.reset()
    a, lp = torch.zeros((sim.R, sim.num_rl), device=dev), torch.zeros((sim.R,), device=dev)
    torch.cuda.synchronize()
    sim.policy_act_dev(pol.struct, obs, a, lp)
    sim.sync()
    assert sim.last_kernel == "k_policy_act_vec"
    sim.close()
    return a, lp


@pytest.mark.parametrize("A,num_hidden", [(5, 1), (5, 3), (6, 2), (1, 2), (2, 3)])
def test_the_net_is_the_torch_net(A, num_hidden):
    """A free log std of -30: the action is the kernel's mean, which must be the torch module's in every column
    (atol 2e-5: the bar of test_policy_merge_gpu.py::test_five_input_network_matches_torch).  A = 5: zeroing input 24, the
    last one, must change the means -- a dropped input or a swapped column would pass unnoticed otherwise."""
    import torch
    R = 512
    dev = torch.device("cuda", 0)
    spec = merge_spec(R=R, cap_human=12, cap_rl=A, num_rl=A, horizon=100, seed=1)
    pol = make_vec_policy(A, num_hidden, True, seed=num_hidden + A, log_std=-30.0)
    with torch.no_grad():
        pol.log_std_param.fill_(-30.0)
    pol.sync()
    obs = torch.rand((R, 5 * A), device=dev) * 2 - 1
    a, _ = act_once(spec, pol, obs)
    with torch.no_grad():
        mu = pol.reference(obs)[0].reshape(R, A)         # (act_dim = 1: reference() has no column axis)
    np.testing.assert_allclose(a.cpu().numpy(), mu.cpu().numpy(), atol=2e-5, rtol=0)
    # the columns are different functions of the observation
    if A > 1:
        assert (mu[:, 0] - mu[:, A - 1]).abs().max() > 1e-2
    last = 5 * A - 1
    obs0 = obs.clone()
    obs0[:, last] = 0.0
    a0, _ = act_once(spec, pol, obs0)
    with torch.no_grad():
        mu0 = pol.reference(obs0)[0].reshape(R, A)
    np.testing.assert_allclose(a0.cpu().numpy(), mu0.cpu().numpy(), atol=2e-5, rtol=0)
    assert (a0 - a).abs().max() > 1e-3                  # (the last input matters to this network)
    assert (mu0 - mu).abs().max() > 1e-3


@pytest.mark.parametrize("A,free", [(5, True), (6, True), (3, False)])
def test_log_probability_is_the_float32_sum_over_the_columns(A, free):
    """logp = sum over the columns, ascending, in float32, of -g^2 / 2 - log std - log(2 pi) / 2, with g recovered from the
    kernel's own action, mean and log std: the mean is what the same weights give with the log std at -30 (a second
    handle, the same counter), the log std the free parameter -- or, with the network's own log std, torch's (its ~1e-6
    error enters the sum once per column).  atol 1e-5 is the multi-agent heads' bar (test_policy_ma_gpu.py) for one
    column; here up to six columns share it, so the comparison is per replica against the same bar."""
    import torch
    R = 256
    dev = torch.device("cuda", 0)
    spec = merge_spec(R=R, cap_human=12, cap_rl=A, num_rl=A, horizon=100, seed=2)
    pol = make_vec_policy(A, 2, free, seed=11, log_std=-0.6)
    obs = torch.rand((R, 5 * A), device=dev) * 2 - 1
    a, lp = act_once(spec, pol, obs)
    # the kernel's mean: the same trunk and mean rows, log std -30
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
    with torch.no_grad():
        _, ls = pol.reference(obs)
    an, mun, lsn = a.cpu().numpy().astype(np.float64), mu.cpu().numpy().astype(np.float64), ls.detach().cpu().numpy().astype(np.float64)
    g = (an - mun) / np.exp(lsn)
    per_col = (-0.5 * g * g - lsn - 0.9189385332046727).astype(np.float32)
    ref = per_col[:, 0].copy()
    for c in range(1, A):
        ref = (ref + per_col[:, c]).astype(np.float32)
    assert np.abs(g).max() > 2.0 and np.abs(g).max() < 6.0 and abs(g.mean()) < 0.1       # (standard normal draws)
    if A > 1:
        assert np.abs(g[:, 0] - g[:, 1]).max() > 0.5                                      # column 1 is another stream
    np.testing.assert_allclose(lp.cpu().numpy(), ref, atol=1e-5, rtol=0)


def test_refusals_are_named():
    spec = merge_spec(R=4, cap_human=12, cap_rl=3, num_rl=2, horizon=100, seed=1)
    pol = make_vec_policy(2, 2, False, seed=1)
    wide = merge_spec(R=4, cap_human=12, cap_rl=8, num_rl=7, horizon=100, seed=1)
    cases = [(make(wide), make_vec_policy(6, 2, False, seed=1), "num_rl <= 6", 7),
             (make(wide), make_vec_policy(6, 2, False, seed=1), "VecFlowEnv.capture", 7),
             (make(spec, "f64"), pol, "FS_MIXED / FS_F64", 2),
             (make(dict(spec, inflows=[dict(f, probability=0.3) for f in spec["inflows"]])), pol, "queue_ok", 2),
             (make(dict(spec, vehicles=[dict(v, fail_safe=1) if v["controller"] == S.CTRL_IDM else v
                                        for v in spec["vehicles"]])), pol, "queue_ok", 2),
             (make(dict(spec, warmup_steps=3)), pol, "warmup_steps = 0", 2),
             (make(spec), make_vec_policy(1, 2, False, seed=1), "fs_policy.obs_dim", 2)]
    try:
        cases.append((make(spec, "mixed"), pol, "FS_MIXED / FS_F64", 2))
    except Exception as e:                         # (fs_create may refuse the combination itself)
        assert "mixed" in str(e).lower() or "FS_MIXED" in str(e), e
    os.environ["FLOWSIM_NO_QUEUE"] = "1"
    try:
        cases.append((make(spec), pol, "queue_ok", 2))
    finally:
        os.environ.pop("FLOWSIM_NO_QUEUE")
    for sim, p, msg, A in cases:
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


def singleagent_merge_params():
    import copy
    import importlib
    import flow_amd
    flow_amd.install_as_flow()                     # the experiment files import `flow.*` as the reference's do
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    fp = dict(importlib.import_module("exp_configs.rl.singleagent.singleagent_merge").flow_params)
    fp["sim"] = copy.deepcopy(fp["sim"])
    return fp


def test_full_size_singleagent_merge_fused_equals_eager():
    """examples/exp_configs/rl/singleagent/singleagent_merge.py as shipped at 1024 replicas: one fused fragment through
    VecFlowEnv.policy_rollout equals eager stepping on every replica."""
    import torch
    from flow_amd.envs import VecFlowEnv
    K, R = 100, 1024                               # (the first controlled vehicle is listed after some 40 steps)
    fp = singleagent_merge_params()
    fp["sim"].seed = 11                            # (the experiment ships seed = None: a seed drawn per handle)
    a_vec, b_vec = VecFlowEnv(fp, num_replicas=R, device=0), VecFlowEnv(fp, num_replicas=R, device=0)
    A = a_vec.act_dim
    assert A == 5 and a_vec.obs_dim == 25 and a_vec.sim.policy_action_dim == A
    obs0 = a_vec.reset().clone()
    b_vec.reset()
    pol_a, pol_b = make_vec_policy(A, 2, True, seed=5), make_vec_policy(A, 2, True, seed=5)
    obs, act, logp, rew, done = a_vec.policy_rollout(pol_a, K, reset_done=True)
    a_vec.sim.sync()
    assert a_vec.sim.last_kernel == KERNEL
    assert tuple(obs.shape) == (K + 1, R, 25) and tuple(act.shape) == (K, R, A) and tuple(logp.shape) == (K, R)
    assert tuple(rew.shape) == (K, R) and tuple(done.shape) == (K, R)
    b_vec.use_current_stream()
    e = eager_fragment(b_vec.sim, pol_b, K, obs0)
    for name, x, y in zip(("obs", "act", "logp", "rew", "done"), (obs, act, logp, rew, done), e):
        np.testing.assert_array_equal(x.cpu().numpy(), y.cpu().numpy(), err_msg=name)
    assert_same_state(a_vec.sim, b_vec.sim)
    assert np.isfinite(rew.cpu().numpy()).all() and (rew.cpu().numpy() > 0).any()
    assert (np.abs(obs.cpu().numpy()[:, :, 0::5]) > 0).any(), "no controlled vehicle in any observation"
    a_vec.close(), b_vec.close()


def test_train_on_device_fuses_the_action_vector_policy_when_asked():
    import math
    fp = singleagent_merge_params()
    import train_vec
    lines = []
    hist = train_vec.train_on_device(fp, replicas=48, fragment=12, iterations=2, fuse_action_vector=True, log=lines.append)
    assert lines[0] == "rollout: fused policy + step kernel (%s)" % KERNEL, lines
    assert len(hist) == 2 and all(math.isfinite(h) for h in hist)
