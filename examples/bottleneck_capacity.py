#!/usr/bin/env python3
"""The capacity diagram of the lane-drop bottleneck as ONE batched run (the reference's
examples/exp_scripts/bottleneck_density_sweep_capacity_diagram.py: 26 inflow rates x 10 trials x 2000 steps, one ray
worker and one SUMO process per rate): every (rate, trial) pair is a replica of one VecFlowEnv over
exp_configs/non_rl/bottleneck.py with its own inflow rate (VecFlowEnv.set_inflow_rates), stepped by one rollout launch.

    python examples/bottleneck_capacity.py --out data [--rates 400 500 ...] [--trials 10] [--steps 2000]

Writes, under --out:
    rets.csv              rate [veh/h], mean outflow over the rate's trials [veh/h]   (the reference's file also has the
                          mean speed and the bottleneck density: BottleneckEnv's head reports neither, so they are omitted)
    inflows_outflows.csv  one row per replica: rate, outflow                          (the reference's second file)
    replicas.csv          one row per replica: rate, trial, outflow, vehicles entered, vehicles dropped at insertion
"""
import argparse
import copy
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

DEFAULT_RATES = list(range(400, 3000, 100))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Outflow of the bottleneck against its inflow: rates x trials replicas, one launch.")
    ap.add_argument("--rates", type=float, nargs="+", default=DEFAULT_RATES, help="inflow rates [veh/h]")
    ap.add_argument("--trials", type=int, default=10, help="replicas per rate")
    ap.add_argument("--steps", type=int, default=2000, help="environment steps per replica")
    ap.add_argument("--out", type=str, required=True, help="directory of the CSV files")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max_vehicles", type=int, default=256, help="vehicle slots per replica (the queue upstream of the "
                    "lane drops outgrows the default 64 at the higher rates)")
    args = ap.parse_args(argv)
    if args.trials < 1 or args.steps < 1 or not args.rates or min(args.rates) <= 0:
        ap.error("need --trials >= 1, --steps >= 1 and rates > 0")
    return args


def replica_rates(rates, trials):
    """[len(rates) * trials]: replica ``k * trials + t`` is trial t of rate k."""
    return np.repeat(np.asarray(rates, dtype=np.float64), int(trials))


def summarise(rates, trials, steps, seconds_per_step, counters):
    """``counters``: FS_FIELD_COUNTERS [R, 8] after ``steps`` steps.  Per replica: outflow [veh/h] = vehicles arrived
    over the simulated time, vehicles entered, vehicles dropped at insertion; per rate: the mean outflow."""
    per_replica = replica_rates(rates, trials)
    counters = np.asarray(counters)
    if counters.shape != (per_replica.size, 8):
        raise ValueError("counters must be [len(rates) * trials, 8]")
    outflow = counters[:, 5] * 3600.0 / (float(steps) * float(seconds_per_step))
    return dict(rates=np.asarray(rates, dtype=np.float64), replica_rate=per_replica,
                replica_trial=np.tile(np.arange(int(trials)), len(rates)), outflow=outflow,
                entered=counters[:, 6].astype(np.int64), dropped=counters[:, 7].astype(np.int64),
                mean_outflow=outflow.reshape(len(rates), int(trials)).mean(axis=1))


def write_csv(out_dir, res):
    os.makedirs(out_dir, exist_ok=True)
    np.savetxt(os.path.join(out_dir, "rets.csv"), np.column_stack([res["rates"], res["mean_outflow"]]), delimiter=",")
    np.savetxt(os.path.join(out_dir, "inflows_outflows.csv"), np.column_stack([res["replica_rate"], res["outflow"]]),
               delimiter=",")
    np.savetxt(os.path.join(out_dir, "replicas.csv"),
               np.column_stack([res["replica_rate"], res["replica_trial"], res["outflow"], res["entered"], res["dropped"]]),
               delimiter=",", header="rate,trial,outflow,entered,dropped", comments="")


def run_sweep(rates, trials, steps, seed=0, max_vehicles=256, device=0):
    """One VecFlowEnv of ``len(rates) * trials`` replicas, one rate per replica, one rollout of ``steps`` steps.  The
    summary of ``summarise`` plus ``spec`` (the handle's configuration), ``periods`` [R, num_inflows] and ``rates_read_back``
    [R] (the periods and the total rate of every replica as the handle holds them) and ``kernel`` (the step kernel the
    rollout ran on)."""
    import flow_amd
    flow_amd.install_as_flow()                         # the experiment files import `flow.*` as the reference's do
    import importlib
    from flow_amd import _lib as L
    from flow_amd.envs import VecFlowEnv
    fp = dict(importlib.import_module("exp_configs.non_rl.bottleneck").flow_params)
    fp["sim"] = copy.deepcopy(fp["sim"])
    fp["sim"].max_vehicles = int(max_vehicles)
    fp["env"] = copy.deepcopy(fp["env"])
    fp["env"].horizon = max(int(fp["env"].horizon), int(steps))
    per_replica = replica_rates(rates, trials)
    import random
    random.seed(seed)                                  # InitialConfig(spacing="random") places the initial vehicle with
    np.random.seed(seed)                               # the global generators: the same seed, the same sweep
    vec = VecFlowEnv(fp, num_replicas=per_replica.size, device=device, seed=seed)
    try:
        vec.set_inflow_rates(per_replica)              # before the reset: every episode of this handle runs on these
        vec.reset()
        vec.rollout(int(steps), obs_every_step=False)
        vec.sim.sync()
        sp = vec.env._spec
        res = summarise(rates, trials, steps, float(sp["sim_step"]) * int(sp.get("sims_per_step", 1)),
                        vec.sim.get_state(L.FS_FIELD_COUNTERS))
        res.update(spec=sp, rates_read_back=vec.inflow_rates().sum(axis=1), kernel=vec.sim.last_kernel,
                   periods=vec.sim.get_state(L.FS_FIELD_INFLOW_PERIOD)[:, :len(sp["inflows"])])
    finally:
        vec.close()
    return res


def main(argv=None):
    args = parse_args(argv)
    res = run_sweep(args.rates, args.trials, args.steps, seed=args.seed, max_vehicles=args.max_vehicles)
    write_csv(args.out, res)
    print("%d replicas x %d steps on %s" % (res["replica_rate"].size, args.steps, res["kernel"]))
    for rate, out in zip(res["rates"], res["mean_outflow"]):
        print("inflow %7.1f veh/h  mean outflow %7.1f veh/h" % (rate, out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
