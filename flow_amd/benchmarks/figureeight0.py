"""figureeight0: 13 noisy IDM vehicles and ONE RL vehicle on the figure eight (the reference's flow/benchmarks/figureeight0.py).
Action (1,), observation (28,), horizon 1500.  python examples/train.py figureeight0"""
from flow_amd.benchmarks._figure_eight import HORIZON, VehicleParams, add_human, add_rl, figure_eight_params  # noqa: F401

vehicles = VehicleParams()
add_human(vehicles, "human", 13)
add_rl(vehicles, "rl", 1)

flow_params = figure_eight_params("figure_eight_0", vehicles)
