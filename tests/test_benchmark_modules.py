"""flow_amd/benchmarks: the figure-eight benchmark experiments (the reference's flow/benchmarks/figureeight{0,1,2}.py)
construct, have the reference's shapes and parameter values, resolve as flow.benchmarks.* after install_as_flow() and are
found by examples/train.py's look-up.  No GPU: the spaces are read off an environment that never touches the library."""
import importlib
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("k,n_rl,n_human", [(0, 1, 13), (1, 7, 7), (2, 14, 0)])
def test_flow_params_construct_with_the_reference_shapes(k, n_rl, n_human):
    from flow_amd.controllers import IDMController, RLController
    from flow_amd.envs import AccelEnv
    from flow_amd.networks import FigureEightNetwork
    fp = importlib.import_module("flow_amd.benchmarks.figureeight%d" % k).flow_params
    assert fp["exp_tag"] == "figure_eight_%d" % k and fp["env_name"] is AccelEnv and fp["network"] is FigureEightNetwork
    assert fp["env"].horizon == 1500 and fp["sim"].sim_step == 0.1
    assert fp["env"].additional_params == {"target_velocity": 20, "max_accel": 3, "max_decel": 3, "sort_vehicles": False}
    veh = fp["veh"]
    assert veh.num_vehicles == 14 and veh.num_rl_vehicles == n_rl
    kinds = [t["acceleration_controller"][0] for t in veh.initial for _ in range(t["num_vehicles"])]
    assert kinds.count(RLController) == n_rl and kinds.count(IDMController) == n_human
    if k == 1:                                           # every other vehicle is an RL vehicle, a human first
        assert kinds == [IDMController, RLController] * 7
    for t in veh.initial:
        if t["acceleration_controller"][0] is IDMController:
            assert t["acceleration_controller"][1] == {"noise": 0.2}
            assert t["car_following_params"].controller_params["decel"] == 1.5
    # the spaces, as the reference documents them: action (n_rl,), observation (28,)
    network = fp["network"](name=fp["exp_tag"], vehicles=veh, net_params=fp["net"], initial_config=fp["initial"])
    env = AccelEnv.__new__(AccelEnv)
    env.env_params, env.initial_vehicles = fp["env"], veh
    env.k = type("K", (), {"vehicle": veh})()
    assert env.action_space.shape == (n_rl,)
    assert env.observation_space.shape == (28,)
    assert network is not None


def test_the_modules_resolve_under_the_flow_alias_and_from_train_py():
    import flow_amd
    flow_amd.install_as_flow()
    for k in range(3):
        a = importlib.import_module("flow.benchmarks.figureeight%d" % k)
        b = importlib.import_module("flow_amd.benchmarks.figureeight%d" % k)
        assert a is b and a.flow_params is b.flow_params
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        train = importlib.import_module("train")
        for k in range(3):
            module, multiagent = train.load_experiment("figureeight%d" % k)
            assert module is importlib.import_module("flow_amd.benchmarks.figureeight%d" % k) and not multiagent
        module, multiagent = train.load_experiment("singleagent_figure_eight")       # (the exp_configs packages come first)
        assert module.__name__.startswith("exp_configs.rl.singleagent") and not multiagent
        with pytest.raises(ValueError, match="Unable to find experiment config"):
            train.load_experiment("figureeight9")
    finally:
        sys.path.remove(os.path.join(ROOT, "examples"))
