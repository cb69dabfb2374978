"""figureeight2: all 14 vehicles of the figure eight are RL vehicles, ONE network 28 -> 14 (the reference's
flow/benchmarks/figureeight2.py).  Action (14,), observation (28,), horizon 1500.
python examples/train.py figureeight2 --fuse_policy --device_adam"""
from flow_amd.benchmarks._figure_eight import HORIZON, VehicleParams, add_rl, figure_eight_params  # noqa: F401

vehicles = VehicleParams()
add_rl(vehicles, "rl", 14)

flow_params = figure_eight_params("figure_eight_2", vehicles)
