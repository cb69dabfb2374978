"""Open merge with a share of RL vehicles on the highway (the experiment of the reference's
examples/exp_configs/rl/singleagent/singleagent_merge.py, same parameter values): one policy commands the first
``num_rl`` RL vehicles of MergePOEnv's list, 5 observations and one acceleration per place.
python examples/train.py singleagent_merge --rl_trainer device"""
from flow.controllers import IDMController, RLController
from flow.core.params import (EnvParams, InFlows, InitialConfig, NetParams, SumoCarFollowingParams, SumoParams,
                              VehicleParams)
from flow.envs import MergePOEnv
from flow.networks import MergeNetwork
from flow.networks.merge import ADDITIONAL_NET_PARAMS

# 0: 10 % RL vehicles, 5 controlled places; 1: 25 %, 13 places; 2: 33 %, 17 places
EXP_NUM = 0

HORIZON = 600
N_ROLLOUTS = 20
N_CPUS = 2

FLOW_RATE = 2000
RL_PENETRATION = (0.1, 0.25, 0.33)[EXP_NUM]
NUM_RL = (5, 13, 17)[EXP_NUM]

additional_net_params = ADDITIONAL_NET_PARAMS.copy()
additional_net_params.update(merge_lanes=1, highway_lanes=1, pre_merge_length=500)

vehicles = VehicleParams()
vehicles.add(veh_id="human", acceleration_controller=(IDMController, {"noise": 0.2}),
             car_following_params=SumoCarFollowingParams(speed_mode="obey_safe_speed"), num_vehicles=5)
vehicles.add(veh_id="rl", acceleration_controller=(RLController, {}),
             car_following_params=SumoCarFollowingParams(speed_mode="obey_safe_speed"), num_vehicles=0)

inflow = InFlows()
inflow.add(veh_type="human", edge="inflow_highway", vehs_per_hour=(1 - RL_PENETRATION) * FLOW_RATE,
           departLane="free", departSpeed=10)
inflow.add(veh_type="rl", edge="inflow_highway", vehs_per_hour=RL_PENETRATION * FLOW_RATE,
           departLane="free", departSpeed=10)
inflow.add(veh_type="human", edge="inflow_merge", vehs_per_hour=100, departLane="free", departSpeed=7.5)

flow_params = dict(
    exp_tag="stabilizing_open_network_merges",
    env_name=MergePOEnv,
    network=MergeNetwork,
    simulator='traci',
    sim=SumoParams(sim_step=0.2, render=False, restart_instance=True),
    env=EnvParams(horizon=HORIZON, sims_per_step=5, warmup_steps=0,
                  additional_params={"max_accel": 1.5, "max_decel": 1.5, "target_velocity": 20, "num_rl": NUM_RL}),
    net=NetParams(inflows=inflow, additional_params=additional_net_params),
    veh=vehicles,
    initial=InitialConfig(),
)
