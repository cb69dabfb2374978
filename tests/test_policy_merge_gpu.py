"""One policy shared by the agents of the multi-agent merge, in the loop (flow_amd/csrc/flowsim_queue.h
k_merge_queue<POLICY>, fs_last_kernel "k_merge_policy"): MultiAgentMergePOEnv with its actions applied
(ma_apply_actions = 1).  Agent c is the RL slot of column c; it is absent while that slot holds no vehicle.

* the fused fragment equals K x (fs_policy_act_dev, fs_step_dev, fs_reset_dev(done)) bit for bit, NaN positions included;
* absent agents get a NaN action and log-probability 0, exactly where the column's RL slot is empty;
* the simulator inside the fragment is the oracle's (the fragment's actions replayed as an action tape);
* five-input networks: the odd observation width reaches every input;
* the shipped environment (actions never applied), FS_F64 / FS_MIXED, non-queue handles and resets with warm-up steps
  are refused by name;
* VecFlowEnv.policy_rollout and examples/train_vec.py take the fused path."""
import os
import sys

import numpy as np
import pytest

from helpers import merge_spec
from oracle import opennet as O
from oracle import refsim as S
from test_open_gpu import compare_state, quiet
from test_policy_gpu import eager_obs0, make_policy_in

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make(spec, precision="f32"):
    from flow_amd.sim import FlowSim
    return FlowSim(spec, precision=precision)


def ma_spec(**kw):
    kw.setdefault("env", O.ENV_MERGE_MA)
    kw.setdefault("ma_apply_actions", True)
    return merge_spec(**kw)


def buffers(K, R, D, n_ag):
    import torch
    dev = torch.device("cuda", 0)
    out = (torch.zeros((K + 1, R, D), device=dev), torch.zeros((K, R, n_ag), device=dev),
           torch.zeros((K, R, n_ag), device=dev), torch.zeros((K, R), device=dev),
           torch.zeros((K, R), dtype=torch.uint8, device=dev))
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


def fused_and_eager(spec, num_hidden, free, K, precision="f32", seed=3):
    """The same fragment twice: one fs_policy_rollout_dev launch, and K x (act, step, masked reset) eagerly."""
    import torch
    from flow_amd import _lib as L
    dev = torch.device("cuda", 0)
    R, n_ag = spec["num_replicas"], spec["num_rl"]
    pol_a, pol_b = make_policy_in(5, num_hidden, free, seed=seed), make_policy_in(5, num_hidden, free, seed=seed)
    fused, eager = make(spec, precision), make(spec, precision)
    for sim in (fused, eager):
        stagger(sim, seed)
    D = fused.obs_dim
    assert D == 5 * n_ag and fused.policy_agents == n_ag
    f = buffers(K, R, D, n_ag)
    fused.policy_rollout_dev(pol_a.struct, K, *f, reset_done=True)
    fused.sync()
    assert fused.last_kernel == "k_merge_policy"
    e = buffers(K, R, D, n_ag)
    eo, ea, elp, er, ed = e
    eo[0].copy_(torch.as_tensor(eager_obs0(eager), device=dev))
    torch.cuda.synchronize()
    for s in range(K):
        eager.policy_act_dev(pol_b.struct, eo[s], ea[s], elp[s])
        eager.step_dev(eo[s + 1], er[s], ed[s], ea[s])
        eager.reset_dev(eo[s + 1], ed[s])
    eager.sync()
    for name, x, y in zip(("obs", "act", "logp", "rew", "done"), f, e):
        np.testing.assert_array_equal(x.cpu().numpy(), y.cpu().numpy(), err_msg=name)
    np.testing.assert_array_equal(fused.pos, eager.pos)
    np.testing.assert_array_equal(fused.vel, eager.vel)
    np.testing.assert_array_equal(fused.time_counter, eager.time_counter)
    for fld in (L.FS_FIELD_ROUTE, L.FS_FIELD_COUNTERS, L.FS_FIELD_SEQ, L.FS_FIELD_ORIGIN, L.FS_FIELD_ARRIVED_RL):
        np.testing.assert_array_equal(fused.get_state(fld), eager.get_state(fld), err_msg="field %d" % fld)
    # a second fragment starts where the first ended, and the state no field shows (policy and noise counters, follower
    # entries, inflow schedule) carries on alike
    K2 = 6
    f2, e2 = buffers(K2, R, D, n_ag), buffers(K2, R, D, n_ag)
    fused.policy_rollout_dev(pol_a.struct, K2, *f2, reset_done=True)
    fused.sync()
    np.testing.assert_array_equal(f2[0][0].cpu().numpy(), f[0][K].cpu().numpy())
    e2[0][0].copy_(eo[K])
    torch.cuda.synchronize()
    for s in range(K2):
        eager.policy_act_dev(pol_b.struct, e2[0][s], e2[1][s], e2[2][s])
        eager.step_dev(e2[0][s + 1], e2[3][s], e2[4][s], e2[1][s])
        eager.reset_dev(e2[0][s + 1], e2[4][s])
    eager.sync()
    for name, x, y in zip(("obs", "act", "logp", "rew", "done"), f2, e2):
        np.testing.assert_array_equal(x.cpu().numpy(), y.cpu().numpy(), err_msg="second fragment: " + name)
    return fused, eager, pol_a, f


@pytest.mark.parametrize("n_rl,noise_math,num_hidden,free", [(5, "hw", 3, False), (5, "exact", 1, True),
                                                             (9, "hw", 1, False), (9, "exact", 3, True)])
def test_fused_fragment_equals_eager_stepping(n_rl, noise_math, num_hidden, free):
    K, R = 90, 6
    spec = ma_spec(R=R, cap_human=24, cap_rl=n_rl, num_rl=n_rl, horizon=40, seed=n_rl, sims_per_step=2,
                   q_rl=2400.0 if n_rl > 5 else 400.0, q_highway=600.0 if n_rl > 5 else 1800.0, noise_math=noise_math)
    fused, eager, pol, (o, a, lp, r, d) = fused_and_eager(spec, num_hidden, free, K)
    dn, an = d.cpu().numpy(), a.cpu().numpy()
    assert ((dn != 0).sum(axis=0) >= 1).all(), "a replica went through the fragment without a reset"
    present = ~np.isnan(an)
    assert present.any() and (~present).any()
    if n_rl > 5:
        assert present.sum(axis=2).max() > 4, "no step with more than one pass of four agents"
    fused.close(), eager.close()


def test_half_precision_state_fused_equals_eager():
    spec = ma_spec(R=5, cap_human=24, cap_rl=5, num_rl=5, horizon=35, seed=9, sims_per_step=5)
    fused, eager, _, (o, a, lp, r, d) = fused_and_eager(spec, 2, False, 60, precision="f16s")
    assert (d.cpu().numpy() != 0).sum() >= 5
    fused.close(), eager.close()


def test_absent_agents_have_no_action_and_log_probability_zero():
    from flow_amd import _lib as L
    K, R, n_rl = 40, 8, 6
    spec = ma_spec(R=R, cap_human=24, cap_rl=n_rl, num_rl=n_rl, horizon=400, seed=2, sims_per_step=2, q_rl=1500.0)
    sim = make(spec)
    stagger(sim, 2, steps=40)                                      # (RL vehicles in the network in odd replicas)
    route = sim.get_state(L.FS_FIELD_ROUTE)                       # [R, N]: -1 = the slot holds no vehicle
    rl_slots = [i for i, v in enumerate(spec["vehicles"]) if v["controller"] == S.CTRL_RL]
    col = [spec["vehicles"][i]["rl_index"] for i in rl_slots]
    pol = make_policy_in(5, 2, False, seed=4)
    o, a, lp, r, d = buffers(K, R, sim.obs_dim, n_rl)
    sim.policy_rollout_dev(pol.struct, K, o, a, lp, r, d)
    sim.sync()
    on, an, lpn = o.cpu().numpy(), a.cpu().numpy(), lp.cpu().numpy()
    here0 = np.zeros((R, n_rl), dtype=bool)
    for i, c in zip(rl_slots, col):
        here0[:, c] = route[:, i] >= 0
    np.testing.assert_array_equal(~np.isnan(an[0]), here0)
    absent = np.isnan(an)
    assert absent.any() and (~absent).any()
    assert (lpn[absent] == 0).all() and np.isfinite(an[~absent]).all() and np.isfinite(lpn[~absent]).all()
    # an absent agent's observation block is zero
    blocks = on[:K].reshape(K, R, n_rl, 5)
    assert (blocks[absent] == 0).all()
    sim.close()


def test_fragment_simulator_is_the_oracles():
    """The fragment's own actions (NaN: no command) replayed through oracle/opennet.py reproduce its observations,
    rewards and final state bit for bit."""
    K, R, n_rl = 80, 4, 5
    spec = quiet(ma_spec(R=R, cap_human=24, cap_rl=n_rl, num_rl=n_rl, horizon=400, seed=6, sims_per_step=3, q_rl=600.0))
    sim, ora = make(spec), O.MergeOracle(spec, np.float32)
    sim.reset()
    o_ref = ora.reset()
    pol = make_policy_in(5, 3, True, seed=8)
    o, a, lp, r, d = buffers(K, R, sim.obs_dim, n_rl)
    sim.policy_rollout_dev(pol.struct, K, o, a, lp, r, d)
    sim.sync()
    on, an, rn = o.cpu().numpy(), a.cpu().numpy(), r.cpu().numpy()
    np.testing.assert_array_equal(on[0], o_ref.astype(np.float32))
    assert np.isnan(an).any() and (~np.isnan(an)).any()
    for k in range(K):
        o_ref, r_ref, d_ref = ora.step(an[k])
        np.testing.assert_array_equal(on[k + 1], o_ref.astype(np.float32), err_msg="obs, step %d" % k)
        np.testing.assert_array_equal(rn[k], r_ref.astype(np.float32), err_msg="reward, step %d" % k)
    compare_state(sim, ora)
    np.testing.assert_array_equal(sim.time_counter, ora.time_counter)
    sim.close()


def test_five_input_network_matches_torch():
    """in_dim = 5 (odd): the eager network sees all five inputs of the agent's block.  With the log std at -30 the action
    is the kernel's mean, which must be the torch module's (DevicePolicy.reference) to float tolerance -- a dropped
    fifth input moves it by ~0.1."""
    import torch
    R = 512
    dev = torch.device("cuda", 0)
    # one agent, present in every replica: the merge's RL slot placed at reset
    spec = ma_spec(R=R, cap_human=12, cap_rl=1, num_rl=1, horizon=100, seed=1, n_init=0)
    alive = np.zeros((R, 13), dtype=bool)
    alive[:, 12] = True
    X = np.zeros((R, 13))
    X[:, 12] = spec["routes"][0]["start"] + 50.0
    spec.update(init_alive=alive, init_pos=X)
    sim = make(spec)
    sim.reset()
    for num_hidden in (1, 3):
        pol = make_policy_in(5, num_hidden, True, seed=num_hidden)
        with torch.no_grad():
            pol.log_std_param.fill_(-30.0)
        pol.sync()
        obs = torch.rand((R, 5), device=dev) * 2 - 1
        a, lp = torch.zeros((R, 1), device=dev), torch.zeros((R, 1), device=dev)
        torch.cuda.synchronize()
        sim.policy_act_dev(pol.struct, obs, a, lp)
        sim.sync()
        with torch.no_grad():
            mu, _ = pol.reference(obs)
            mu4, _ = pol.reference(torch.cat([obs[:, :4], torch.zeros_like(obs[:, 4:])], 1))
        np.testing.assert_allclose(a.reshape(-1).cpu().numpy(), mu.cpu().numpy(), atol=2e-5, rtol=0)
        assert (mu4 - mu).abs().max() > 1e-3                  # (the fifth input matters to this network)
    sim.close()


def _experiment(name):
    import importlib
    import flow_amd
    flow_amd.install_as_flow()                     # the experiment files import `flow.*` as the reference's do
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    return importlib.import_module("exp_configs.rl.multiagent." + name).flow_params


def applied_merge_params():
    """multiagent_merge.py's flow_params with the actions applied (MultiAgentMergePOEnv's evident intent)."""
    from flow_amd.envs.multiagent.merge import MultiAgentMergePOEnv

    class MultiAgentMergeAppliedPOEnv(MultiAgentMergePOEnv):
        APPLY_ENUMERATE_QUIRK = False
    return dict(_experiment("multiagent_merge"), env_name=MultiAgentMergeAppliedPOEnv)


def test_refusals_are_named():
    from flow_amd.envs import VecFlowEnv
    spec = ma_spec(R=4, cap_human=12, cap_rl=2, num_rl=2, horizon=100, seed=1)
    pol = make_policy_in(5, 2, False, seed=1)
    cases = [(make(dict(spec, ma_apply_actions=False)), "FS_ENV_MERGE_MA"),
             (make(spec, "f64"), "FS_MIXED / FS_F64"),
             (make(dict(spec, inflows=[dict(f, probability=0.3) for f in spec["inflows"]])), "queue_ok"),
             (make(dict(spec, vehicles=[dict(v, fail_safe=1) if v["controller"] == S.CTRL_IDM else v
                                        for v in spec["vehicles"]])), "queue_ok"),
             (make(dict(spec, warmup_steps=3)), "warmup_steps = 0")]
    try:
        cases.append((make(spec, "mixed"), "FS_MIXED / FS_F64"))
    except Exception as e:                         # (fs_create may refuse the combination itself)
        assert "mixed" in str(e).lower() or "FS_MIXED" in str(e), e
    os.environ["FLOWSIM_NO_QUEUE"] = "1"
    try:
        cases.append((make(spec), "queue_ok"))
    finally:
        os.environ.pop("FLOWSIM_NO_QUEUE")
    for sim, msg in cases:
        sim.reset()
        o, a, lp, r, d = buffers(3, 4, sim.obs_dim, 2)
        with pytest.raises(NotImplementedError, match=msg):
            sim.policy_rollout_dev(pol.struct, 3, o, a, lp, r, d, reset_done=True)
        if msg != "warmup_steps = 0":              # (the eager policy has no resets to refuse)
            with pytest.raises(NotImplementedError, match=msg):
                sim.policy_act_dev(pol.struct, o[0], a[0], lp[0])
        sim.close()
    vec = VecFlowEnv(_experiment("multiagent_merge"), num_replicas=4, device=0)
    vec.reset()
    with pytest.raises(NotImplementedError, match="actions never reach the simulator"):
        vec.policy_rollout(make_policy_in(5, 2, False, seed=1), 3)
    vec.close()


def test_vec_env_policy_rollout_and_train_vec_take_the_fused_path():
    from flow_amd.envs import VecFlowEnv
    fp = applied_merge_params()
    vec = VecFlowEnv(fp, num_replicas=8, device=0)
    n_ag = vec.num_rl
    vec.reset()
    pol = make_policy_in(5, 2, True, seed=2)
    obs, act, logp, rew, done = vec.policy_rollout(pol, 30, reset_done=True)
    vec.sim.sync()
    assert tuple(obs.shape) == (31, 8, 5 * n_ag) and tuple(act.shape) == (30, 8, n_ag) and tuple(logp.shape) == (30, 8, n_ag)
    assert tuple(rew.shape) == (30, 8) and tuple(done.shape) == (30, 8) and vec.sim.last_kernel == "k_merge_policy"
    an = act.cpu().numpy()
    assert np.isnan(an).any() and np.isfinite(an[~np.isnan(an)]).all()
    vec.close()
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_vec
    lines = []
    hist = train_vec.train_on_device(fp, replicas=32, fragment=40, iterations=2, shared_agents=True, log=lines.append)
    assert any("fused policy + step kernel (k_merge_policy)" in l for l in lines), lines
    assert len(hist) == 2 and np.isfinite(hist).all()
