"""What the three figure-eight benchmarks share (the reference's flow/benchmarks/figureeight{0,1,2}.py, same parameter
values): AccelEnv on FigureEightNetwork, 14 vehicles, horizon 1500, sim_step 0.1, accelerations in [-3, 3], target
velocity 20 m/s; humans are IDM vehicles with acceleration noise 0.2 and decel 1.5, every vehicle obeys the safe speed."""
from flow_amd.controllers import ContinuousRouter, IDMController, RLController
from flow_amd.core.params import (EnvParams, InitialConfig, NetParams, SumoCarFollowingParams, SumoParams,
                                  VehicleParams)
from flow_amd.envs import AccelEnv
from flow_amd.networks import FigureEightNetwork
from flow_amd.networks.figure_eight import ADDITIONAL_NET_PARAMS

HORIZON = 1500


def add_human(vehicles, veh_id, num_vehicles):
    vehicles.add(veh_id=veh_id, acceleration_controller=(IDMController, {"noise": 0.2}),
                 routing_controller=(ContinuousRouter, {}),
                 car_following_params=SumoCarFollowingParams(speed_mode="obey_safe_speed", decel=1.5),
                 num_vehicles=num_vehicles)


def add_rl(vehicles, veh_id, num_vehicles):
    vehicles.add(veh_id=veh_id, acceleration_controller=(RLController, {}), routing_controller=(ContinuousRouter, {}),
                 car_following_params=SumoCarFollowingParams(speed_mode="obey_safe_speed"), num_vehicles=num_vehicles)


def figure_eight_params(exp_tag, vehicles):
    return dict(
        exp_tag=exp_tag,
        env_name=AccelEnv,
        network=FigureEightNetwork,
        simulator='traci',
        sim=SumoParams(sim_step=0.1, render=False),
        env=EnvParams(horizon=HORIZON,
                      additional_params={"target_velocity": 20, "max_accel": 3, "max_decel": 3, "sort_vehicles": False}),
        net=NetParams(additional_params=dict(ADDITIONAL_NET_PARAMS)),
        veh=vehicles,
        initial=InitialConfig(),
    )
