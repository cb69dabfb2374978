"""A user-written environment on the device: HighwayStyleEnv (examples/compiled_env.py: the observation and reward of the
reference's MultiAgentHighwayPOEnv, flow/envs/multiagent/highway.py, written as a flow_amd.envs.CompiledEnv) on a ring of
22 vehicles whose length is redrawn from [230, 270] m at every reset.  NUM_AUTOMATED autonomous vehicles are spread evenly
among noisy humans that drive on a user-written controller as well (examples/compiled_controller.py TimeGap), so the
library copy of this experiment holds the user's get_accel AND the user's head; each autonomous vehicle is an agent with a
5-value observation and all share the policy 'av'.

    python examples/train.py compiled_highway_ring --fuse_policy --device_adam
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))

from compiled_controller import TimeGap  # noqa: E402
from compiled_env import HighwayStyleEnv  # noqa: E402
from flow.controllers import ContinuousRouter, RLController  # noqa: E402
from flow.core.params import EnvParams, InitialConfig, NetParams, SumoParams, VehicleParams  # noqa: E402
from flow.networks import RingNetwork  # noqa: E402

HORIZON = 1500
N_ROLLOUTS = 20
N_CPUS = 2
NUM_AUTOMATED = 2       # at most 22

# every autonomous vehicle is followed by its share of the humans
vehicles = VehicleParams()
humans_left = 22 - NUM_AUTOMATED
for i in range(NUM_AUTOMATED):
    vehicles.add(veh_id="rl_{}".format(i), acceleration_controller=(RLController, {}),
                 routing_controller=(ContinuousRouter, {}), num_vehicles=1)
    share = round(humans_left / (NUM_AUTOMATED - i))
    humans_left -= share
    vehicles.add(veh_id="human_{}".format(i), acceleration_controller=(TimeGap, {"t_gap": 1.0, "noise": 0.1}),
                 routing_controller=(ContinuousRouter, {}), num_vehicles=share)

flow_params = dict(
    exp_tag="compiled_highway_ring",
    env_name=HighwayStyleEnv,
    network=RingNetwork,
    simulator="traci",
    sim=SumoParams(sim_step=0.1, render=False, restart_instance=False),
    env=EnvParams(horizon=HORIZON, warmup_steps=100,
                  additional_params={"max_accel": 1, "max_decel": 1, "target_velocity": 10, "ring_length": [230, 270]}),
    net=NetParams(additional_params={"length": 260, "lanes": 1, "speed_limit": 30, "resolution": 40}),
    veh=vehicles,
    initial=InitialConfig(bunching=50, min_gap=0),
)
