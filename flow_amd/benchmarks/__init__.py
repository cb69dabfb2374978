"""The reference's benchmark experiments (flow/benchmarks/) written for this package: each module exposes ``flow_params``.
``python examples/train.py figureeight1 --fuse_policy --device_adam`` looks a name up here after the two exp_configs
packages; after ``flow_amd.install_as_flow()`` the modules are ``flow.benchmarks.<name>`` too.

Built so far: the figure-eight family (``figureeight0``, ``figureeight1``, ``figureeight2``: AccelEnv on FigureEightNetwork
with 1, 7 and 14 RL vehicles among 14)."""
