"""Desired speeds per lane-segment ahead of a lane drop (the experiment of the reference's
examples/exp_configs/rl/singleagent/singleagent_bottleneck.py, same parameter values): 2300 veh/h enter four lanes that
narrow to two and then to one, a tenth of them RL vehicles; one policy reads 141 observations (35 lane-segments x 4 and
the outflow) and sets 20 speed offsets, one per controlled lane-segment of edges 2-4.  Toll booth and ramp meter are off.
python examples/train.py singleagent_bottleneck --rl_trainer device"""
from flow.controllers import ContinuousRouter, RLController, SimLaneChangeController
from flow.core.params import (EnvParams, InFlows, InitialConfig, NetParams, SumoCarFollowingParams,
                              SumoLaneChangeParams, SumoParams, TrafficLightParams, VehicleParams)
from flow.envs import BottleneckDesiredVelocityEnv
from flow.networks import BottleneckNetwork

HORIZON = 1000
N_CPUS = 2
N_ROLLOUTS = N_CPUS * 4

SCALING = 1
DISABLE_TB = True
DISABLE_RAMP_METER = True
AV_FRAC = 0.10
FLOW_RATE = 2300 * SCALING

vehicles = VehicleParams()
vehicles.add(veh_id="human", lane_change_controller=(SimLaneChangeController, {}),
             routing_controller=(ContinuousRouter, {}),
             car_following_params=SumoCarFollowingParams(speed_mode="all_checks"),
             lane_change_params=SumoLaneChangeParams(lane_change_mode=0), num_vehicles=1 * SCALING)
vehicles.add(veh_id="followerstopper", acceleration_controller=(RLController, {}),
             lane_change_controller=(SimLaneChangeController, {}), routing_controller=(ContinuousRouter, {}),
             car_following_params=SumoCarFollowingParams(speed_mode=9),
             lane_change_params=SumoLaneChangeParams(lane_change_mode=0), num_vehicles=1 * SCALING)

# (edge, segments, controlled): 2 segments x (4 + 4 + 2) lanes = 20 actions; (edge, segments): 35 observed lane-segments
CONTROLLED_SEGMENTS = [("1", 1, False), ("2", 2, True), ("3", 2, True), ("4", 2, True), ("5", 1, False)]
OBSERVED_SEGMENTS = [("1", 1), ("2", 3), ("3", 3), ("4", 3), ("5", 1)]

inflow = InFlows()
inflow.add(veh_type="human", edge="1", vehs_per_hour=FLOW_RATE * (1 - AV_FRAC), departLane="random", departSpeed=10)
inflow.add(veh_type="followerstopper", edge="1", vehs_per_hour=FLOW_RATE * AV_FRAC, departLane="random", departSpeed=10)

traffic_lights = TrafficLightParams()

flow_params = dict(
    exp_tag="DesiredVelocity",
    env_name=BottleneckDesiredVelocityEnv,
    network=BottleneckNetwork,
    simulator='traci',
    sim=SumoParams(sim_step=0.5, render=False, print_warnings=False, restart_instance=True),
    env=EnvParams(horizon=HORIZON, warmup_steps=40, sims_per_step=1,
                  additional_params={"target_velocity": 40, "max_accel": 3, "max_decel": 3, "lane_change_duration": 5,
                                     "disable_tb": DISABLE_TB, "disable_ramp_metering": DISABLE_RAMP_METER,
                                     "controlled_segments": CONTROLLED_SEGMENTS, "symmetric": False,
                                     "observed_segments": OBSERVED_SEGMENTS, "reset_inflow": False,
                                     "inflow_range": [1000, 2000]}),
    net=NetParams(inflows=inflow, additional_params={"scaling": SCALING, "speed_limit": 23}),
    veh=vehicles,
    initial=InitialConfig(spacing="uniform", min_gap=5, lanes_distribution=float("inf"),
                          edges_distribution=["2", "3", "4", "5"]),
    tls=traffic_lights,
)
