"""User-defined environments whose observation and reward run in the step kernel (the reference's extension point is an
Env subclass with Python get_state / compute_reward, flow/envs/base.py; here the three hooks are C++ statement bodies
compiled into a copy of the library: flow_amd.envs.CompiledEnv).

* ``HighwayStyleEnv``: the observation and reward of MultiAgentHighwayPOEnv (flow/envs/multiagent/highway.py) on a closed
  loop -- per RL vehicle its speed, the speed differences and headways to leader and follower; a desired-velocity term plus
  a penalty on time headways below one second.  An environment the project does not ship and a user can now write.
* ``AccelStyleEnv``: AccelEnv restated as a CompiledEnv (what tests/test_compiled_env_gpu.py compares with the built-in
  head, bit for bit).

Each head is written once as C++ (what the step kernel runs) and once as numpy (what a test checks it against).

    python examples/compiled_env.py          # 4096 replicas of a 22-vehicle ring with 2 RL vehicles, 1500 steps
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from flow_amd.envs import CompiledEnv  # noqa: E402


def max_cost(target_velocity, num_vehicles):
    """np.linalg.norm([target_velocity] * N) the way the built-in heads evaluate it: a float64 sum, then the root."""
    ss = 0.0
    for _ in range(int(num_vehicles)):
        ss += float(target_velocity) * float(target_velocity)
    return float(np.sqrt(ss))


class HighwayStyleEnv(CompiledEnv):
    OBSERVE = "rl"
    OBS_PER_VEHICLE = 5
    OBS_SOURCE = """
        o[0] = v / max_speed;
        o[1] = (v_lead - v) / max_speed;
        o[2] = h / L;
        o[3] = (v - v_follow) / max_speed;
        o[4] = h_follow / L;
    """
    REWARD_TERMS = 2
    TERM_SOURCE = """
        const T dv = v - target_velocity;
        t[0] = dv * dv;
        t[1] = (is_rl && v > T(0)) ? tmin((tmax(h / v, T(0)) - T(1)) / T(1), T(0)) : T(0);
    """
    REWARD_SOURCE = """
        if (fail) return T(0);
        const T cost1 = tmax(p[0] - tsqrt(sum[0]), T(0)) / p[0];
        return tmax(cost1 + T(0.1) * sum[1], T(0));
    """

    def __init__(self, env_params, sim_params, network, simulator='traci'):
        cost = max_cost(env_params.additional_params["target_velocity"], network.vehicles.num_vehicles)
        CompiledEnv.__init__(self, env_params, sim_params, network, simulator, params=[cost])


class AccelStyleEnv(CompiledEnv):
    OBSERVE = "all"
    OBS_PER_VEHICLE = 2
    OBS_SOURCE = """
        o[0] = v / max_speed;
        o[1] = x / L;
    """
    REWARD_TERMS = 1
    TERM_SOURCE = """
        const T dv = v - target_velocity;
        t[0] = dv * dv;
    """
    REWARD_SOURCE = """
        const T cost = tsqrt(sum[0]);
        const T reward = tmax(p[0] - cost, T(0)) / (p[0] + T(1.1920928955078125e-07));
        return fail ? T(0) : reward;
    """

    def __init__(self, env_params, sim_params, network, simulator='traci'):
        cost = max_cost(env_params.additional_params["target_velocity"], network.vehicles.num_vehicles)
        CompiledEnv.__init__(self, env_params, sim_params, network, simulator, params=[cost])


def head_source(cls):
    """The head of a CompiledEnv class as the dict a spec carries (spec['user_env_source'])."""
    head = CompiledEnv.check_head(cls)
    head.pop("params")
    return head


def tree_sum(a):
    """Sum over the last axis in the kernels' order: zero-pad to a power of two, add neighbours pairwise."""
    a = np.asarray(a)
    seg = 1
    while seg < a.shape[-1]:
        seg *= 2
    a = np.concatenate([a, np.zeros(a.shape[:-1] + (seg - a.shape[-1],), dtype=a.dtype)], axis=-1)
    while a.shape[-1] > 1:
        a = a[..., 0::2] + a[..., 1::2]
    return a[..., 0]


def ring_neighbours(pos, vel, lengths, L):
    """(v_lead, h, v_follow, h_follow) [R, N] of a single-lane ring in slot (= driving) order, in the arrays' type, the way
    the step kernel forms them: the gap to the leader wrapped by L, minus the LEADER's length; the follower's headway."""
    x_lead = np.roll(pos, -1, axis=1)
    d = x_lead - pos
    d = np.where(d < 0, d + L, d)
    h = d - np.roll(lengths, -1)[None, :].astype(pos.dtype)
    return np.roll(vel, -1, axis=1), h, np.roll(vel, 1, axis=1), np.roll(h, 1, axis=1)


def highway_numpy(pos, vel, lengths, L, is_rl, rl_index, max_speed, target_velocity, p0, fail, dtype=np.float32):
    """HighwayStyleEnv's head in numpy, operation by operation: (obs [R, 5 num_rl], reward [R]).  ``L`` [R] or a scalar."""
    T = np.dtype(dtype).type
    pos, vel = np.asarray(pos, dtype=dtype), np.asarray(vel, dtype=dtype)
    L = np.broadcast_to(np.asarray(L, dtype=dtype), (pos.shape[0],))[:, None]
    ms, tv, p0 = T(max_speed), T(target_velocity), T(p0)
    v_lead, h, v_follow, h_follow = ring_neighbours(pos, vel, np.asarray(lengths), L)
    blocks = np.stack([vel / ms, (v_lead - vel) / ms, h / L, (vel - v_follow) / ms, h_follow / L], axis=-1)   # [R, N, 5]
    rl = np.flatnonzero(is_rl)
    obs = np.zeros((pos.shape[0], 5 * rl.size), dtype=np.float32)
    for i in rl:
        obs[:, 5 * rl_index[i]:5 * rl_index[i] + 5] = blocks[:, i].astype(np.float32)
    dv = vel - tv
    with np.errstate(divide="ignore", invalid="ignore"):
        gap = np.minimum((np.maximum(h / vel, T(0)) - T(1)) / T(1), T(0))
    t1 = np.where(np.asarray(is_rl)[None, :] & (vel > 0), gap, T(0)).astype(dtype)
    s0, s1 = tree_sum(dv * dv), tree_sum(t1)
    cost1 = np.maximum(p0 - np.sqrt(s0), T(0)) / p0
    rew = np.maximum(cost1 + T(0.1) * s1, T(0))
    return obs, np.where(fail, T(0), rew).astype(dtype)


def ring_flow_params(env_name=HighwayStyleEnv, num_vehicles=22, num_rl=2, user_humans=True, horizon=1500, warmup_steps=0):
    """``num_vehicles`` on a 230 m ring, ``num_rl`` RL vehicles spread among noisy humans.  ``user_humans``: the humans
    drive on a user-written controller too (examples/compiled_controller.py TimeGap) -- the library copy then holds the
    user's get_accel AND the user's head --, else on the IDM."""
    from compiled_controller import TimeGap
    from flow_amd.controllers import ContinuousRouter, IDMController, RLController
    from flow_amd.core.params import EnvParams, InitialConfig, NetParams, SumoParams, VehicleParams
    from flow_amd.networks import RingNetwork
    human = (TimeGap, {"t_gap": 1.0, "noise": 0.1}) if user_humans else (IDMController, {"noise": 0.2})
    veh = VehicleParams()
    left = num_vehicles - num_rl
    for k in range(num_rl):
        share = round(left / (num_rl - k))
        left -= share
        veh.add("human_%d" % k, acceleration_controller=human, routing_controller=(ContinuousRouter, {}), num_vehicles=share)
        veh.add("rl_%d" % k, acceleration_controller=(RLController, {}), routing_controller=(ContinuousRouter, {}),
                num_vehicles=1)
    return dict(exp_tag="compiled_env_ring", env_name=env_name, network=RingNetwork, simulator="traci",
                sim=SumoParams(sim_step=0.1), initial=InitialConfig(bunching=20), veh=veh,
                env=EnvParams(horizon=horizon, warmup_steps=warmup_steps,
                              additional_params={"max_accel": 1, "max_decel": 1, "target_velocity": 10}),
                net=NetParams(additional_params={"length": 230, "lanes": 1, "speed_limit": 30, "resolution": 40}))


if __name__ == "__main__":
    import time
    import torch
    from flow_amd.envs import VecFlowEnv
    vec = VecFlowEnv(ring_flow_params(), num_replicas=4096, device=0)      # builds (once) and loads the library copy
    K = 1500
    tape = (0.5 * torch.randn((K, 4096, vec.act_dim), device=vec.device)).contiguous()
    vec.reset()
    vec.rollout(K, tape)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    obs, rew, done = vec.rollout(K, tape)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print("HighwayStyleEnv ring: %.2f G vehicle-steps/s on %s, obs_dim %d, mean reward %.3f"
          % (4096 * 22 * K / dt / 1e9, vec.sim.last_kernel, vec.obs_dim, float(rew.mean())))
    vec.close()
