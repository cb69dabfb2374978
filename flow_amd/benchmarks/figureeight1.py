"""figureeight1: every other vehicle of the figure eight is an RL vehicle -- 7 noisy IDM vehicles and 7 RL vehicles, ONE
network 28 -> 7 (the reference's flow/benchmarks/figureeight1.py).  Action (7,), observation (28,), horizon 1500.
python examples/train.py figureeight1 --fuse_policy --device_adam"""
from flow_amd.benchmarks._figure_eight import HORIZON, VehicleParams, add_human, add_rl, figure_eight_params  # noqa: F401

vehicles = VehicleParams()
for i in range(7):
    add_human(vehicles, "human{}".format(i), 1)
    add_rl(vehicles, "rl{}".format(i), 1)

flow_params = figure_eight_params("figure_eight_1", vehicles)
