"""One policy shared by the agents of a replica, in the loop (flow_amd/csrc/flowsim_policy.h k_ring_policy<POMA>,
k_loop_policy<AccelMA>): the reference's multi-agent ring (MultiAgentWaveAttenuationPOEnv, multiagent_ring.py) and figure
eight (MultiAgentAccelPOEnv, multiagent_figure_eight.py) map every agent to the policy 'av'.

* the fused fragment equals K x (fs_policy_act_dev, fs_step_dev, masked fs_reset_dev) bit for bit: observation blocks,
  per-agent actions and log-probabilities, the shared reward, resets with warm-up steps and a pending ring length;
* agent c draws from its own Philox column (0x40000000 + c); agent 0's stream is the single-agent stream;
* the simulator inside the fragment is the oracle's;
* VecFlowEnv.policy_rollout and examples/train_vec.py take the fused path for shared agents."""
import os
import sys

import numpy as np
import pytest

from oracle import refsim as S
from test_multiagent_ring_gpu import ma_ring_experiment_spec
from test_policy_gpu import eager_obs0, make_policy_in

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make(spec, precision="f32"):
    from flow_amd.sim import FlowSim
    return FlowSim(spec, precision=precision)


def buffers(K, R, D, n_ag, dev):
    import torch
    out = (torch.zeros((K + 1, R, D), device=dev), torch.zeros((K, R, n_ag), device=dev),
           torch.zeros((K, R, n_ag), device=dev), torch.zeros((K, R), device=dev),
           torch.zeros((K, R), dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()          # (the handles launch on streams of their own)
    return out


def fused_and_eager(spec, k, num_hidden, free, K, pending=None):
    """The same fragment twice: one fs_policy_rollout_dev launch, and K x (act, step, masked reset) eagerly."""
    import torch
    from flow_amd import _lib as L
    dev = torch.device("cuda", 0)
    R, n_ag = spec["num_replicas"], spec["num_rl"]
    pol_a, pol_b = make_policy_in(k, num_hidden, free, seed=3), make_policy_in(k, num_hidden, free, seed=3)
    fused, eager = make(spec), make(spec)
    for sim in (fused, eager):
        sim.reset()
        if pending is not None:                    # a pending ring length: the in-fragment resets must take it
            sim.set_state(L.FS_FIELD_INIT_RING_LENGTH, sim.get_state(L.FS_FIELD_RING_LENGTH) + pending)
    D = fused.obs_dim
    assert D == k * n_ag and fused.policy_agents == n_ag
    f = buffers(K, R, D, n_ag, dev)
    fused.policy_rollout_dev(pol_a.struct, K, *f, reset_done=True)
    fused.sync()
    e = buffers(K, R, D, n_ag, dev)
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
    np.testing.assert_array_equal(fused.get_state(L.FS_FIELD_RING_LENGTH), eager.get_state(L.FS_FIELD_RING_LENGTH))
    return fused, eager, pol_a, f


@pytest.mark.parametrize("rl_slots,noise,num_hidden,free", [((0, 11), 0.2, 3, False), ((4, 5, 13, 21), 0.2, 2, True),
                                                             ((0, 11), 0.0, 1, True), ((4, 5, 13, 21), 0.0, 3, False)])
def test_ring_fused_fragment_equals_eager_stepping(rl_slots, noise, num_hidden, free):
    import torch
    K, R = 70, 9
    spec = ma_ring_experiment_spec(S.ENV_WAVE_ATTENUATION_PO_MA, R, rl_slots, noise=noise, N=22)
    spec["warmup_steps"], spec["horizon"] = 7, 40      # every replica ends an episode inside the fragment and is reset
    fused, eager, pol, (o, a, lp, r, d) = fused_and_eager(spec, 3, num_hidden, free, K, pending=3.0)
    assert fused.last_kernel == "k_ring_policy<POMA>"
    assert (d.cpu().numpy() != 0).sum() >= R and not np.isnan(o.cpu().numpy()).any()
    # a second fragment continues the streams
    dev = torch.device("cuda", 0)
    o2, a2, lp2, r2, d2 = buffers(5, R, fused.obs_dim, len(rl_slots), dev)
    fused.policy_rollout_dev(pol.struct, 5, o2, a2, lp2, r2, d2, reset_done=True)
    fused.sync()
    np.testing.assert_array_equal(o2[0].cpu().numpy(), o[K].cpu().numpy())
    assert not np.array_equal(a2[0].cpu().numpy(), a[0].cpu().numpy())
    fused.close(), eager.close()


def fig8_ma_spec(R, horizon, seed, hostile=False):
    """multiagent_figure_eight.py's population: 2 x (6 noisy IDM + 1 RL), obey_safe_speed, MultiAgentAccelPOEnv (columns
    not in slot order).  hostile: no safe-speed mode anywhere -- vehicles run into each other at the crossing."""
    from helpers import figure_eight_spec, idm_vehicle
    spec = figure_eight_spec(R=R, N=14, horizon=horizon, seed=seed, num_rl=2, env=S.ENV_ACCEL_PO_MA, action_low=-3.0,
                             action_high=3.0, track_aux=False)
    sm = 0 if hostile else 1
    veh = []
    for g in range(2):
        veh += [idm_vehicle(speed_mode=sm, max_decel=1.5, noise=0.2) for _ in range(6)]
        veh.append(idm_vehicle(controller=S.CTRL_RL, rl_index=1 - g, speed_mode=sm, max_accel=3.0, max_decel=3.0))
    spec["vehicles"] = veh
    spec["seed"] = 31 + seed
    return spec


@pytest.mark.parametrize("num_hidden,free", [(3, False), (1, True)])
def test_figure_eight_fused_fragment_equals_eager_stepping(num_hidden, free):
    K, R = 90, 7
    spec = fig8_ma_spec(R, horizon=35, seed=4)
    fused, eager, _, (o, a, lp, r, d) = fused_and_eager(spec, 6, num_hidden, free, K)
    assert fused.last_kernel == "k_loop_policy<AccelMA>"
    assert (d.cpu().numpy() != 0).sum() >= 2 * R and o.shape[2] == 12 and not np.isnan(o.cpu().numpy()).any()
    fused.close(), eager.close()


def test_figure_eight_crossing_collision_ends_nothing():
    """A policy that floors the accelerator without the safe-speed mode: vehicles collide at the crossing (the same
    actions under AccelEnv flag it), and the multi-agent head ends no episode and zeroes no reward."""
    import torch
    K, R = 260, 7
    spec = fig8_ma_spec(R, horizon=10 ** 6, seed=2, hostile=True)
    pol = make_policy_in(6, 2, True, seed=5)
    with torch.no_grad():
        pol.head.weight.zero_()
        pol.head.bias.fill_(3.0)                       # accelerate at ~3 m/s^2, whatever the observation
        pol.log_std_param.fill_(-3.0)
    pol.sync()
    sim = make(spec)
    sim.reset()
    dev = torch.device("cuda", 0)
    o, a, lp, r, d = buffers(K, R, sim.obs_dim, 2, dev)
    sim.policy_rollout_dev(pol.struct, K, o, a, lp, r, d, reset_done=True)
    sim.sync()
    assert sim.last_kernel == "k_loop_policy<AccelMA>"
    rn = r.cpu().numpy()
    assert not d.cpu().numpy().any() and np.isfinite(rn).all()
    # the same trajectory under AccelEnv (the fragment's own actions, no resets) reports the collisions and zeroes their
    # rewards; elsewhere the two heads' desired-velocity rewards agree
    acc_spec = dict(spec, env=S.ENV_ACCEL)
    from test_parity_gpu import _rollout
    b, ob, rb, db = _rollout(acc_spec, K, a.cpu().numpy())
    crash = (db & 2) != 0
    assert crash.any(), "no collision: the test lost its premise"
    np.testing.assert_array_equal(rn[~crash], rb[~crash])
    assert (rb[crash] == 0).all() and (rn[crash] > 0).any()
    b.close(), sim.close()


def test_agent_streams():
    """Agent 0 of a two-agent handle draws the single-agent stream, agent 1 a stream of its own; logp is the density of
    the sampled action."""
    import torch
    from test_ringrl_gpu import rl_ring_spec
    R = 1024
    dev = torch.device("cuda", 0)
    two = make(ma_ring_experiment_spec(S.ENV_WAVE_ATTENUATION_PO_MA, R, (0, 11), noise=0.0))
    one = make(rl_ring_spec(R=R, N=22, seed=5))
    pol = make_policy_in(3, 3, True, seed=9)
    with torch.no_grad():
        pol.log_std_param.fill_(0.0)
    pol.sync()
    obs = (torch.rand((R, 6), device=dev) * 2 - 1) * torch.tensor([1.0, 0.3, 0.5] * 2, device=dev)
    obs1 = obs[:, :3].contiguous()
    a2, lp2 = torch.zeros((R, 2), device=dev), torch.zeros((R, 2), device=dev)
    a1, lp1 = torch.zeros(R, device=dev), torch.zeros(R, device=dev)
    torch.cuda.synchronize()
    two.policy_act_dev(pol.struct, obs, a2, lp2)
    one.policy_act_dev(pol.struct, obs1, a1, lp1)
    two.sync(), one.sync()
    np.testing.assert_array_equal(a2[:, 0].cpu().numpy(), a1.cpu().numpy())
    np.testing.assert_array_equal(lp2[:, 0].cpu().numpy(), lp1.cpu().numpy())
    with torch.no_grad():
        mu, ls = pol.reference(obs.view(R * 2, 3))
        g = (a2.reshape(-1) - mu) / ls.exp()
        lp_ref = (-0.5 * g.double() ** 2 - ls.double() - 0.9189385332046727).float()
    g0 = g.view(R, 2)[:, 0]
    g1 = g.view(R, 2)[:, 1]
    assert (g0 - g1).abs().max() > 0.5                          # column 1 is another stream
    np.testing.assert_allclose(lp2.reshape(-1).cpu().numpy(), lp_ref.cpu().numpy(), atol=1e-5, rtol=0)
    gn = g1.cpu().numpy()
    assert abs(gn.mean()) < 0.1 and abs(gn.std() - 1.0) < 0.1
    two.close(), one.close()


def test_fragment_simulator_is_the_oracles():
    """Replaying a noise-free fragment's own actions [K, R, n_ag] through oracle/refsim.py reproduces its observations
    and rewards."""
    import torch
    K, R = 50, 6
    spec = ma_ring_experiment_spec(S.ENV_WAVE_ATTENUATION_PO_MA, R, (4, 5, 13, 21), noise=0.0)
    sim, ora = make(spec), S.RingOracle(spec, np.float32)
    sim.reset()
    o_ref = ora.reset()
    pol = make_policy_in(3, 3, False, seed=1)
    o, a, lp, r, d = buffers(K, R, sim.obs_dim, 4, torch.device("cuda", 0))
    sim.policy_rollout_dev(pol.struct, K, o, a, lp, r, d, reset_done=False)
    sim.sync()
    on, an, rn = o.cpu().numpy(), a.cpu().numpy(), r.cpu().numpy()
    np.testing.assert_array_equal(on[0], o_ref.astype(np.float32))
    for k in range(K):
        o_ref, r_ref, d_ref = ora.step(an[k])
        np.testing.assert_array_equal(on[k + 1], o_ref.astype(np.float32), err_msg="obs, step %d" % k)
        np.testing.assert_array_equal(rn[k], r_ref.astype(np.float32), err_msg="reward, step %d" % k)
    np.testing.assert_array_equal(sim.pos, ora.x)
    sim.close()


def _experiment(name):
    import importlib
    import flow_amd
    flow_amd.install_as_flow()                     # the experiment files import `flow.*` as the reference's do
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    return importlib.import_module("exp_configs.rl.multiagent." + name).flow_params


def test_vec_env_policy_rollout_and_train_vec_take_the_fused_path():
    from flow_amd.envs import VecFlowEnv
    fp = _experiment("multiagent_ring")
    vec = VecFlowEnv(fp, num_replicas=16, device=0)
    vec.reset()
    pol = make_policy_in(3, 2, True, seed=2)
    obs, act, logp, rew, done = vec.policy_rollout(pol, 8)
    vec.sim.sync()
    assert tuple(obs.shape) == (9, 16, 6) and tuple(act.shape) == (8, 16, 2) and tuple(logp.shape) == (8, 16, 2)
    assert tuple(rew.shape) == (8, 16) and vec.sim.last_kernel == "k_ring_policy<POMA>"
    assert np.isfinite(act.cpu().numpy()).all()
    vec.close()
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_vec
    lines = []
    hist = train_vec.train_on_device(fp, replicas=64, fragment=20, iterations=2, shared_agents=True, log=lines.append)
    assert any("fused policy + step kernel (k_ring_policy<POMA>)" in l for l in lines), lines
    assert len(hist) == 2 and np.isfinite(hist).all()


def test_unsupported_multi_agent_configurations_are_refused_by_name():
    import torch
    dev = torch.device("cuda", 0)
    spec = ma_ring_experiment_spec(S.ENV_WAVE_ATTENUATION_PO_MA, 4, (0, 11), noise=0.0)
    pol3, pol6 = make_policy_in(3, 2, False, seed=1), make_policy_in(6, 2, False, seed=1)
    # (fs_create itself refuses FS_MIXED with a multi-agent head; a float64 handle steps on the generic kernel)
    cases = [(make(spec, "f64"), pol3, "float32 only"),
             (make(dict(spec, env=S.ENV_ACCEL_PO_MA)), pol6, "FS_ENV_ACCEL_PO_MA on a ring"),
             (make(spec), pol6, "fs_policy.obs_dim")]
    for sim, pol, msg in cases:
        o, a, lp, r, d = buffers(3, 4, sim.obs_dim, 2, dev)
        with pytest.raises(NotImplementedError, match=msg):
            sim.policy_rollout_dev(pol.struct, 3, o, a, lp, r, d)
        sim.close()
    from flow_amd.envs import VecFlowEnv
    vec = VecFlowEnv(_experiment("multiagent_merge"), num_replicas=4, device=0)
    vec.reset()
    with pytest.raises(NotImplementedError, match="FS_ENV_MERGE_MA"):
        vec.policy_rollout(make_policy_in(vec.obs_dim // max(vec.num_rl, 1), 2, False, seed=1), 3)
    vec.close()
