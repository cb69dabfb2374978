"""examples/exp_configs/rl/singleagent/singleagent_bottleneck.py: `python examples/train.py singleagent_bottleneck` finds it,
and it is the reference's experiment (BottleneckDesiredVelocityEnv on the lane drop, 2070 / 230 veh/h, 141 observations, 20
speed offsets).  Host side only: the handle itself needs a device (tests/test_policy_wide_gpu.py runs the experiment)."""
import importlib
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def train(monkeypatch):
    monkeypatch.syspath_prepend(os.path.join(ROOT, "examples"))
    return importlib.import_module("train")               # (installs flow_amd as `flow`, as the experiment files need)


def test_train_finds_the_experiment_and_its_parameters_are_the_reference_s(train):
    from flow_amd.controllers import ContinuousRouter, RLController, SimCarFollowingController, SimLaneChangeController
    from flow_amd.envs import BottleneckDesiredVelocityEnv
    from flow_amd.networks import BottleneckNetwork
    module, multiagent = train.load_experiment("singleagent_bottleneck")
    assert not multiagent and module.__name__.endswith("singleagent.singleagent_bottleneck")
    assert (module.HORIZON, module.N_CPUS, module.N_ROLLOUTS, module.SCALING, module.AV_FRAC) == (1000, 2, 8, 1, 0.10)
    assert module.DISABLE_TB and module.DISABLE_RAMP_METER
    fp = module.flow_params
    assert fp["env_name"] is BottleneckDesiredVelocityEnv and fp["network"] is BottleneckNetwork
    assert fp["sim"].sim_step == 0.5 and fp["sim"].restart_instance is True
    env = fp["env"]
    assert (env.horizon, env.warmup_steps, env.sims_per_step) == (1000, 40, 1)
    assert env.additional_params == {
        "target_velocity": 40, "max_accel": 3, "max_decel": 3, "lane_change_duration": 5, "disable_tb": True,
        "disable_ramp_metering": True, "symmetric": False, "reset_inflow": False, "inflow_range": [1000, 2000],
        "controlled_segments": [("1", 1, False), ("2", 2, True), ("3", 2, True), ("4", 2, True), ("5", 1, False)],
        "observed_segments": [("1", 1), ("2", 3), ("3", 3), ("4", 3), ("5", 1)]}
    assert fp["net"].additional_params == {"scaling": 1, "speed_limit": 23}
    assert len(fp["tls"].get_properties()) == 0           # toll booth and ramp meter off: no traffic lights
    types = {t["veh_id"]: t for t in fp["veh"].initial}
    assert sorted(types) == ["followerstopper", "human"]
    human, rl = types["human"], types["followerstopper"]
    assert human["num_vehicles"] == 1 and rl["num_vehicles"] == 1                 # one of each type to start with
    assert human["acceleration_controller"][0] is SimCarFollowingController       # SUMO-driven
    assert rl["acceleration_controller"] == (RLController, {})
    assert human["car_following_params"].speed_mode == 31                         # all_checks
    assert rl["car_following_params"].speed_mode == 9
    for t in (human, rl):
        assert t["lane_change_params"].lane_change_mode == 0
        assert t["lane_change_controller"][0] is SimLaneChangeController and t["routing_controller"][0] is ContinuousRouter
    flows = fp["net"].inflows.get()
    assert [(f["vtype"], f["edge"], round(f["vehsPerHour"], 6), f["departLane"], f["departSpeed"]) for f in flows] == \
        [("human", "1", 2070.0, "random", 10), ("followerstopper", "1", 230.0, "random", 10)]
    ic = fp["initial"]
    assert (ic.spacing, ic.min_gap, ic.lanes_distribution) == ("uniform", 5, float("inf"))
    assert ic.edges_distribution == ["2", "3", "4", "5"]


def test_host_side_spec_64_slots_141_observations_20_actions(train):
    from flow_amd import _lib as L
    from flow_amd.core.kernel.kernel import Kernel
    from flow_amd.envs import BottleneckDesiredVelocityEnv
    from flow_amd.envs.spec import slot_capacities
    fp = train.load_experiment("singleagent_bottleneck")[0].flow_params
    network = fp["network"](name=fp["exp_tag"], vehicles=fp["veh"], net_params=fp["net"], initial_config=fp["initial"],
                            traffic_lights=fp["tls"])
    # the default pool: no max_vehicles, 64 slots -- the 62 spare ones shared out by inflow rate
    assert getattr(fp["sim"], "max_vehicles", None) in (None, 64)
    names, caps = slot_capacities(network.vehicles, fp["net"].inflows.get(), 64)
    assert names == ["human", "followerstopper"] and sum(caps) == 64 and caps[0] > caps[1] >= 1
    assert BottleneckDesiredVelocityEnv.FS_ENV == L.FS_ENV_BOTTLENECK_DV
    env = BottleneckDesiredVelocityEnv.__new__(BottleneckDesiredVelocityEnv)      # (the spaces need no handle)
    add = fp["env"].additional_params
    env.env_params, env.sim_step = fp["env"], fp["sim"].sim_step
    env.segments, env.obs_segments, env.symmetric = add["controlled_segments"], add["observed_segments"], add["symmetric"]
    env.k = Kernel(simulator="traci", sim_params=fp["sim"])
    env.k.generate_network(network)
    assert env.observation_space.shape == (141,) and env.action_space.shape == (20,)
    # max_accel / max_decel are 3 / 3; the space is the reference's: the speed offset of one step, +-3 * sim_step
    assert (add["max_accel"], add["max_decel"]) == (3, 3)
    assert (float(env.action_space.low[0]), float(env.action_space.high[0])) == (-3 * 0.5, 3 * 0.5)
