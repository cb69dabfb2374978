"""flow_amd.envs.CompiledEnv on the GPU (head FS_ENV_USER in k_steps): AccelEnv restated as a CompiledEnv against the
built-in head, bit for bit (rings of 7 / 14 / 22 / 40 vehicles, the figure eight, a collision); the highway-style head
against its numpy restatement on the handle's own state (f32 bit for bit, f64 within 1e-6); the user's controller and the
user's head in one library against the oracle; the stock library's refusal; VecFlowEnv (rollout, capture with a
DevicePolicy, reset_done, snapshots, episode statistics); a short training run.

Two library copies serve every test (built once, then cached under flow_amd/_user/): (a) AccelStyleEnv's head alone, (b)
HighwayStyleEnv's head together with TimeGap's get_accel.  The bodies are examples/compiled_env.py's."""
import os
import sys

import numpy as np
import pytest

from helpers import figure_eight_spec, idm_vehicle, ring_spec
from oracle import refsim as S
from oracle.rewards import tree_sum

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
from compiled_controller import TimeGap, time_gap_numpy  # noqa: E402
import compiled_env as CE  # noqa: E402
from compiled_env import AccelStyleEnv, HighwayStyleEnv, head_source, highway_numpy, max_cost  # noqa: E402

ENV_USER = 12
K_ACCEL = 150


def test_the_example_restates_the_oracle_s_tree_sum():
    a = np.random.default_rng(0).normal(0, 3, (5, 22)).astype(np.float32)
    np.testing.assert_array_equal(CE.tree_sum(a), tree_sum(a))


# ------------------------------------------------------------------ 1. AccelEnv written as a CompiledEnv
def accel_ring_spec(N, collide=False, perm=False):
    """R = 5 replicas, N - 1 noisy IDM vehicles + 1 RL vehicle mid-ring; a ring length per replica.  collide: the RL vehicle
    has no speed-mode clamp and its tape (accel_tape) is full throttle in three replicas: it runs into its leader."""
    spec = ring_spec(R=5, N=N, length=230.0 if N < 40 else 420.0, junction_length=0.1, horizon=120, seed=5, noise_math="exact",
                     num_rl=1, action_low=-3.0, action_high=3.0, track_aux=False)
    spec["ring_length"] = np.asarray(spec["ring_length"]) + np.arange(5) * 2.5
    veh = [idm_vehicle(noise=0.2, speed_mode=25) for _ in range(N)]
    veh[N // 2] = idm_vehicle(controller=S.CTRL_RL, rl_index=0, speed_mode=0 if collide else 25)
    spec["vehicles"] = veh
    if perm:
        spec["obs_perm"] = np.random.default_rng(2).permutation(N).astype(np.int32)
    return spec


def accel_tape(spec, collide=False):
    rng = np.random.default_rng(9)
    tape = rng.uniform(-3.5, 3.5, (K_ACCEL, spec["num_replicas"], 1)).astype(np.float32)      # (beyond the bounds: clipped)
    if collide:
        tape[:, :3, 0] = 3.0
    return tape


def as_user_accel(spec):
    return dict(spec, env=ENV_USER, user_env_source=head_source(AccelStyleEnv),
                user_env_p=[max_cost(spec["target_velocity"], spec["num_vehicles"])])


ACCEL_CASES = {"ring7": lambda: accel_ring_spec(7), "ring14_perm": lambda: accel_ring_spec(14, perm=True),
               "ring22": lambda: accel_ring_spec(22), "ring40": lambda: accel_ring_spec(40),
               "ring7_collision": lambda: accel_ring_spec(7, collide=True),
               "figure_eight14": lambda: fig8_rl_spec()}


def fig8_rl_spec():
    spec = figure_eight_spec(R=5, N=14, horizon=120, seed=3, noise_math="exact", num_rl=1, track_aux=False)
    veh = [dict(v, noise=0.2) for v in spec["vehicles"]]
    veh[6] = idm_vehicle(controller=S.CTRL_RL, rl_index=0, speed_mode=1, max_decel=1.5)
    return dict(spec, vehicles=veh)


def test_the_collision_case_collides_in_the_oracle():
    """(CPU work: the placement and tape of ring7_collision were chosen with the oracle.)"""
    spec = accel_ring_spec(7, collide=True)
    ora = S.RingOracle(dict(spec, horizon=10 ** 6), np.float32)
    ora.reset()
    tape = accel_tape(spec, True)
    crashed = np.zeros(5, bool)
    for k in range(K_ACCEL):
        crashed |= ora.step(tape[k])[2]
    assert crashed[:3].all()


@pytest.mark.parametrize("case", sorted(ACCEL_CASES))
def test_accel_env_as_a_compiled_env_equals_the_built_in_head(case):
    from flow_amd.sim import FlowSim
    spec = ACCEL_CASES[case]()
    tape = accel_tape(spec, "collision" in case)
    user, stock = FlowSim(as_user_accel(spec), "f32"), FlowSim(spec, "f32")
    assert "_user" in user.lib._name and "_user" not in stock.lib._name
    assert user.obs_dim == stock.obs_dim == 2 * spec["num_vehicles"]
    np.testing.assert_array_equal(user.reset(), stock.reset())
    collided = np.zeros(spec["num_replicas"], bool)
    for k in range(K_ACCEL):
        o, r, _ = user.step(tape[k])
        o_ref, r_ref, _ = stock.step(tape[k])
        np.testing.assert_array_equal(o, o_ref, err_msg="obs, step %d" % k)
        np.testing.assert_array_equal(r, r_ref, err_msg="reward, step %d" % k)
        np.testing.assert_array_equal(user.last_done_flags, stock.last_done_flags, err_msg="done, step %d" % k)
        collided |= (stock.last_done_flags & 2) != 0
    assert user.last_kernel.startswith("k_steps"), user.last_kernel
    np.testing.assert_array_equal(user.pos, stock.pos)
    assert (stock.last_done_flags & 1).all()                                # the horizon bit travelled too
    if "collision" in case:
        assert collided.any(), "no collision: the fail path was not compared"
    assert r_ref.max() > 0 or "collision" in case
    user.close(), stock.close()


# ------------------------------------------------------------------ 2. / 3. the highway-style head (library (b))
def highway_spec(R=6, user_controllers=False):
    """22 vehicles, 2 RL vehicles whose action columns are NOT in slot order (slot 5: column 1, slot 16: column 0), noisy
    humans (IDM; with user_controllers two of three drive on TimeGap's law), a ring length per replica."""
    N = 22
    spec = ring_spec(R=R, N=N, junction_length=0.1, horizon=10 ** 6, seed=7, noise_math="exact", num_rl=2, action_low=-1.0,
                     action_high=1.0, track_aux=False)
    spec["ring_length"] = np.linspace(230.0, 270.0, R)
    rng = np.random.default_rng(1)
    spec["init_pos"] = np.asarray(spec["init_pos"]) + np.abs(rng.normal(0, 0.4, (R, N)))
    veh = []
    for i in range(N):
        d = idm_vehicle(noise=0.2, speed_mode=25)
        if user_controllers and i % 3 != 2:
            d.update(controller=S.CTRL_USER, p=[1.0 + 0.1 * (i % 4), 2.0, 0.3, 0.6, 0.05, 0.0, 0.0, 0.0])
        veh.append(d)
    veh[5] = idm_vehicle(controller=S.CTRL_RL, rl_index=1, speed_mode=25)
    veh[16] = idm_vehicle(controller=S.CTRL_RL, rl_index=0, speed_mode=25)
    spec["vehicles"] = veh
    spec["user_controller_source"] = TimeGap.SOURCE
    spec["user_controller_numpy"] = time_gap_numpy
    spec["user_env_source"] = head_source(HighwayStyleEnv)
    spec["user_env_p"] = [max_cost(spec["target_velocity"], N)]
    return spec


def restated(spec, pos, vel, fail, dtype):
    T = np.dtype(dtype).type
    L = np.asarray(spec["ring_length"], dtype=dtype) + T(4) * T(spec["junction_length"])
    veh = spec["vehicles"]
    return highway_numpy(pos, vel, [v["length"] for v in veh], L, np.array([v["controller"] == S.CTRL_RL for v in veh]),
                         [v["rl_index"] for v in veh], spec["max_speed"], spec["target_velocity"], spec["user_env_p"][0],
                         fail, dtype)


def highway_actions(k, R):
    return np.random.default_rng(100 + k).uniform(-1.2, 1.2, (R, 2)).astype(np.float32)


def test_highway_head_equals_its_numpy_restatement_bit_for_bit_in_float32():
    from flow_amd.sim import FlowSim
    spec = highway_spec()
    R = spec["num_replicas"]
    sim = FlowSim(dict(spec, env=ENV_USER), "f32")
    assert sim.obs_dim == 10
    o = sim.reset()                                                           # the zero-step form of the head
    np.testing.assert_array_equal(o, restated(spec, sim.pos, sim.vel, False, np.float32)[0])
    for k in range(100):
        o, r, _ = sim.step(None if k == 0 else highway_actions(k, R))          # (k = 0: a warm-up step, has_action false)
        fail = (sim.last_done_flags & 2) != 0
        o_ref, r_ref = restated(spec, sim.pos, sim.vel, fail, np.float32)
        np.testing.assert_array_equal(o, o_ref, err_msg="obs, step %d" % k)
        np.testing.assert_array_equal(r, r_ref, err_msg="reward, step %d" % k)
    assert sim.last_kernel.startswith("k_steps") and sim.vel.max() > 2.0 and 0 < r.min() and r.max() < 1
    assert np.abs(o[:, 3]).max() > 0 and np.abs(o[:, 8]).max() > 0            # the follower reads are not idle
    sim.close()


def test_highway_head_in_float64():
    from flow_amd.sim import FlowSim
    spec = highway_spec(R=3)
    sim = FlowSim(dict(spec, env=ENV_USER), "f64")
    o = sim.reset()
    np.testing.assert_allclose(o, restated(spec, sim.pos, sim.vel, False, np.float64)[0], rtol=0, atol=1e-6)
    for k in range(100):
        o, r, _ = sim.step(None if k == 0 else highway_actions(k, 3))
        o_ref, r_ref = restated(spec, sim.pos, sim.vel, (sim.last_done_flags & 2) != 0, np.float64)
        np.testing.assert_allclose(o, o_ref, rtol=0, atol=1e-6, err_msg="obs, step %d" % k)
        np.testing.assert_allclose(r, r_ref.astype(np.float32), rtol=0, atol=1e-6, err_msg="reward, step %d" % k)
    sim.close()


def test_user_controller_and_user_head_in_one_handle_equal_the_oracle():
    """Library (b): the state is the oracle's with TimeGap's numpy restatement (it runs the AccelEnv head, which does not
    touch the state), the observation and reward are the restated head on the ORACLE's state."""
    from flow_amd.sim import FlowSim
    spec = highway_spec(user_controllers=True)
    R = spec["num_replicas"]
    sim, ora = FlowSim(dict(spec, env=ENV_USER), "f32"), S.RingOracle(dict(spec, env=S.ENV_ACCEL), np.float32)
    o = sim.reset()
    ora.reset()
    np.testing.assert_array_equal(o, restated(spec, ora.x, ora.v, False, np.float32)[0])
    for k in range(100):
        a = highway_actions(k, R)
        o, r, d = sim.step(a)
        _, _, crashed = ora.step(a)                                           # (no horizon: done = a collision)
        np.testing.assert_array_equal(sim.pos, ora.x, err_msg="positions, step %d" % k)
        o_ref, r_ref = restated(spec, ora.x, ora.v, crashed, np.float32)
        np.testing.assert_array_equal(o, o_ref, err_msg="obs, step %d" % k)
        np.testing.assert_array_equal(r, r_ref, err_msg="reward, step %d" % k)
        np.testing.assert_array_equal(d, crashed)
    np.testing.assert_array_equal(sim.vel, ora.v)
    assert sim.last_kernel.startswith("k_steps")
    sim.close()


# ------------------------------------------------------------------ 4. the stock library
def test_the_stock_library_refuses_a_user_head_at_creation():
    from flow_amd.sim import FlowSim
    spec = accel_ring_spec(7)
    with pytest.raises(NotImplementedError, match=r"FS_ENV_USER[\s\S]*flow_amd\.envs\.CompiledEnv"):
        FlowSim(dict(spec, env=ENV_USER), "f32")


# ------------------------------------------------------------------ 5. VecFlowEnv
def vec_env(seed=3, **kw):
    """AccelStyleEnv (library (a)) on a ring of 14 vehicles, one of them an RL vehicle: R = 8, episodes of 30 steps after
    2 warm-up steps."""
    from flow_amd.envs import VecFlowEnv
    fp = CE.ring_flow_params(env_name=AccelStyleEnv, num_vehicles=14, num_rl=1, user_humans=False, horizon=30, warmup_steps=2)
    fp["sim"].noise_math = "exact"
    return VecFlowEnv(fp, num_replicas=8, device=0, seed=seed, **kw)


def device_policy(in_dim, seed=11):
    import torch
    from flow_amd.utils.device_policy import DevicePolicy
    gen = torch.Generator().manual_seed(5)
    layers = [torch.nn.Linear(in_dim, 32), torch.nn.Linear(32, 32), torch.nn.Linear(32, 1)]
    for lin in layers:
        with torch.no_grad():
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=gen) * 0.3)
            lin.bias.copy_(torch.randn(lin.bias.shape, generator=gen) * 0.1)
        lin.to("cuda:0")
    log_std = torch.nn.Parameter(torch.full((1,), -0.5, device="cuda:0"))
    pol = DevicePolicy(layers[:2], layers[2], log_std=log_std, seed=seed)
    pol.sync()
    return pol


def test_vec_rollout_equals_single_steps():
    import torch
    a, b = vec_env(), vec_env()
    assert (a.obs_dim, a.act_dim, a.num_rl) == (28, 1, 1) and a.sim.policy_agents == 1
    tape = torch.from_numpy(np.random.default_rng(4).uniform(-1.5, 1.5, (20, 8, 1)).astype(np.float32)).to(a.device)
    torch.testing.assert_close(a.reset(), b.reset(), rtol=0, atol=0)
    obs, rew, done = a.rollout(20, tape)
    assert a.sim.last_kernel.startswith("k_steps")
    for k in range(20):
        o, r, d = b.step(tape[k])
        assert torch.equal(o, obs[k]) and torch.equal(r, rew[k]) and torch.equal(d, done[k]), k
    a.close(), b.close()


def test_vec_capture_with_a_device_policy_equals_eager_policy_act_and_step():
    import torch
    K = 10
    g, e = vec_env(), vec_env()
    pol_g, pol_e = device_policy(28), device_policy(28)
    g.reset()
    graph = g.capture(K, pol_g)                                               # (two eager warm-up steps)
    graph.begin(g.reset())
    obs, act, rew, done = graph.replay()
    graph.synchronize()
    assert g.sim.last_kernel.startswith("k_steps")
    o = e.reset()
    for _ in range(2):
        a, _ = e.policy_act(pol_e, o)
        assert e.sim.last_kernel == "k_policy_act"
        o = e.step(a)[0]
    o = e.reset()
    assert torch.equal(obs[0], o)
    for k in range(K):
        a, lp = e.policy_act(pol_e, o)
        o, r, d = e.step(a)
        assert torch.equal(act[k], a) and torch.equal(graph.logp[k], lp), k
        assert torch.equal(obs[k + 1], o) and torch.equal(rew[k], r) and torch.equal(done[k], d), k
    assert torch.isfinite(act).all() and act.std() > 0
    g.close(), e.close()


def test_vec_reset_done_snapshot_statistics_and_the_refused_fused_rollout():
    import torch
    vec = vec_env()
    vec.reset()
    tape = torch.from_numpy(np.random.default_rng(6).uniform(-1, 1, (45, 8, 1)).astype(np.float32)).to(vec.device)
    # snapshot, 15 steps, restore, the same 15 steps
    snap = vec.snapshot()
    first = [tuple(t.clone() for t in vec.step(tape[k])) for k in range(15)]
    pos1 = vec.positions
    vec.restore(snap)
    again = [tuple(t.clone() for t in vec.step(tape[k])) for k in range(15)]
    for x, y in zip(first, again):
        assert all(torch.equal(u, v) for u, v in zip(x, y))
    np.testing.assert_array_equal(vec.positions, pos1)
    # on to the horizon (30 steps): every episode ends; reset_done re-places exactly the replicas whose flag is set
    for k in range(15, 30):
        obs, rew, done = vec.step(tape[k])
    assert (done.cpu().numpy() & 1).all() and (vec.sim.time_counter == 32).all()
    done[::2] = 0                                                             # (the env's own flag tensor)
    before = obs.clone()
    obs = vec.reset_done()
    t = vec.sim.time_counter
    assert (t[0::2] == 32).all() and (t[1::2] == 2).all()
    assert torch.equal(obs[0::2], before[0::2]) and not torch.equal(obs[1::2], before[1::2])
    # episode statistics of a fragment; the fused policy rollout is refused by name
    vec.reset()
    o, r, d = vec.rollout(45, tape)
    stats = vec.episode_stats(r, d, reset=True).cpu().numpy()
    assert stats[0] == float((d != 0).sum()) and stats[0] >= 8 and np.isfinite(stats[1])
    with pytest.raises(NotImplementedError, match="FS_ENV_USER"):
        vec.policy_rollout(device_policy(28), 4)
    vec.close()


def test_shared_agents_of_the_rl_layout_take_one_policy():
    """OBSERVE = "rl": fs_policy_act_dev runs the num_rl agents of a replica through ONE policy of OBS_PER_VEHICLE inputs;
    a policy of the whole observation is refused by name."""
    import torch
    from flow_amd.envs import VecFlowEnv
    fp = CE.ring_flow_params(horizon=30, warmup_steps=2)                      # HighwayStyleEnv + TimeGap: library (b)
    vec = VecFlowEnv(fp, num_replicas=8, device=0, seed=2)
    assert (vec.obs_dim, vec.act_dim, vec.sim.policy_agents, vec.sim.policy_action_dim) == (10, 2, 2, 1)
    obs = vec.reset()
    pol = device_policy(5)
    act, logp = vec.policy_act(pol, obs)
    assert vec.sim.last_kernel == "k_policy_act" and tuple(act.shape) == (8, 2) and tuple(logp.shape) == (8, 2)
    assert torch.isfinite(act).all() and torch.isfinite(logp).all()
    vec.step(act)
    assert vec.sim.last_kernel.startswith("k_steps")
    with pytest.raises(NotImplementedError, match="FS_ENV_USER"):
        vec.policy_act(device_policy(10), obs)
    vec.close()


# ------------------------------------------------------------------ 6. training
def test_train_compiled_highway_ring_through_the_graph_around_the_policy_kernel(monkeypatch, capsys):
    import math
    import re
    import flow_amd
    flow_amd.install_as_flow()
    train = __import__("train")
    train_vec = __import__("train_vec")
    seen = {}
    choose = train_vec.choose_rollout

    def recording(vec, pi, *a, **kw):
        seen["pi"], seen["before"] = pi, [p.detach().clone() for p in pi.mu.parameters()]
        return choose(vec, pi, *a, **kw)
    monkeypatch.setattr(train_vec, "choose_rollout", recording)
    train.main(["compiled_highway_ring", "--fuse_policy", "--device_adam", "--replicas", "64", "--rollout_size", "20",
                "--num_steps", "3"])
    lines = capsys.readouterr().out.splitlines()
    how = [ln for ln in lines if ln.startswith("rollout:")][0]
    assert "around the policy kernel (k_policy_act)" in how, how
    its = [ln for ln in lines if ln.startswith("iteration")]
    assert len(its) == 3
    for ln in its:
        assert math.isfinite(float(re.search(r"mean step reward\s+(\S+)", ln).group(1))), ln
    after = [p.detach() for p in seen["pi"].mu.parameters()]
    assert all(bool(np.isfinite(p.cpu().numpy()).all()) for p in after)
    assert any(not bool((p == q).all()) for p, q in zip(after, seen["before"])), "the policy's weights did not change"
