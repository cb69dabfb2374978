"""NUM_RINGS separate rings (MultiRingNetwork) of 21 noisy IDM vehicles and one autonomous vehicle each; every autonomous
vehicle is an agent of MultiWaveAttenuationPOEnv, all agents share the policy 'av', and each is rewarded for the speeds on
its own ring (the flow_params of the reference's examples/exp_configs/rl/multiagent/lord_of_the_rings.py, same parameter
values, without the RLlib policy boilerplate).  NUM_RINGS selects the experiment: the file is loaded with another value
the way singleagent_merge.py is with another EXP_NUM."""
from flow.controllers import ContinuousRouter, IDMController, RLController
from flow.core.params import EnvParams, InitialConfig, NetParams, SumoParams, VehicleParams
from flow.envs.multiagent import MultiWaveAttenuationPOEnv
from flow.networks import MultiRingNetwork

# time horizon of a single rollout
HORIZON = 3000
# number of rings
NUM_RINGS = 1
# number of rollouts per training iteration
N_ROLLOUTS = 20
# number of parallel workers
N_CPUS = 2

# one autonomous vehicle and 21 human-driven vehicles on every ring
vehicles = VehicleParams()
for i in range(NUM_RINGS):
    vehicles.add(veh_id='human_{}'.format(i), acceleration_controller=(IDMController, {'noise': 0.2}),
                 routing_controller=(ContinuousRouter, {}), num_vehicles=21)
    vehicles.add(veh_id='rl_{}'.format(i), acceleration_controller=(RLController, {}),
                 routing_controller=(ContinuousRouter, {}), num_vehicles=1)

flow_params = dict(
    exp_tag='lord_of_numrings{}'.format(NUM_RINGS),
    env_name=MultiWaveAttenuationPOEnv,
    network=MultiRingNetwork,
    simulator='traci',
    sim=SumoParams(sim_step=0.1, render=False),
    env=EnvParams(horizon=HORIZON, warmup_steps=750,
                  additional_params={'max_accel': 1, 'max_decel': 1, 'ring_length': [230, 230], 'target_velocity': 4}),
    net=NetParams(additional_params={'length': 230, 'lanes': 1, 'speed_limit': 30, 'resolution': 40,
                                     'num_rings': NUM_RINGS}),
    veh=vehicles,
    initial=InitialConfig(bunching=20.0, spacing='custom'),
)

# the one policy every agent maps to (the reference's POLICY_GRAPHS / policy_mapping_fn)
POLICIES_TO_TRAIN = ['av']


def policy_mapping_fn(_):
    return 'av'
