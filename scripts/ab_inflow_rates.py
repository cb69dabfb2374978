"""A/B of two builds of libflowsim.so on the open-network legs whose kernels read the inflow schedule, both libraries
loaded in ONE process, their launches alternating:
    python scripts/ab_inflow_rates.py --parent PARENT/libflowsim.so [--reps 7] [--out profiles/inflow_rates_ab.json]

Legs (bench.py's configurations): C4, the lane drop on k_drop_queue (128 replicas x 256 slots, one 1000-step episode with
an action tape), and C5, the merge on k_merge_queue (1024 replicas x 64 slots, 600 steps x 5 sub-steps).  Per leg one
handle per library, one warm-up launch each, then `reps` x (reset, timed launch) of the parent's handle and of this tree's,
in turn; env-steps/s (C5: sub-steps/s): median, min and max per library.  Boxes differ by up to 25 %, so only this
same-process comparison counts; `new_median_within_parent_range` is the bar."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch


def seconds(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def rates(ts, work):
    r = sorted(work / t for t in ts)
    return {"median": r[len(r) // 2], "min": r[0], "max": r[-1], "samples": [work / t for t in ts]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="libflowsim.so built from the parent commit")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench
    from flow_amd import _lib as L
    from flow_amd.envs import VecFlowEnv
    libs = (("parent", os.path.abspath(args.parent)), ("new", L.LIB_PATH))
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    res = {"what": "libflowsim.so of the parent commit against this tree's (per-replica inflow periods: one 8-byte load "
                   "per schedule-keeping lane and launch), both loaded in one process, %d timed launches each, alternating"
                   % args.reps,
           "bar": "each leg's `new` median inside the parent's min-max (new_median_within_parent_range)",
           "device": torch.cuda.get_device_name(0), "reps": args.reps, "legs": {}}
    legs = (("c4_bottleneck", bench.c4_flow_params(256), 128, 1000, 1, "k_drop_queue"),
            ("c5_merge", bench.c5_flow_params(), 1024, 600, 5, "k_merge_queue"))
    for leg, fp, R, K, sps, kernel in legs:
        runs = []
        for name, path in libs:
            L.LIB_PATH = path                              # (read when a handle is created)
            vec = VecFlowEnv(fp, num_replicas=R, device=0)
            assert vec.sim.lib is L.load(path)
            gen = torch.Generator(device=dev).manual_seed(3)
            tape = ((torch.rand((K, R, vec.act_dim), device=dev, generator=gen) * 2 - 1) * 1.5) if leg == "c4_bottleneck" else None
            out = (torch.empty((K, R, vec.obs_dim), device=dev), torch.empty((K, R), device=dev),
                   torch.empty((K, R), dtype=torch.uint8, device=dev))
            vec.reset()
            vec.sim.rollout_dev(K, *out, actions=tape)     # warm-up launch
            torch.cuda.synchronize()
            assert vec.sim.last_kernel == kernel, vec.sim.last_kernel
            runs.append((name, vec, tape, out, []))
        L.LIB_PATH = libs[1][1]
        for _ in range(args.reps):                         # alternately: drifts of the clock hit both libraries alike
            for name, vec, tape, out, ts in runs:
                vec.reset()
                torch.cuda.synchronize()
                ts.append(seconds(lambda: vec.sim.rollout_dev(K, *out, actions=tape)))
        row = {"kernel": kernel, "replicas": R, "steps": K, "sims_per_step": sps,
               "unit": "env-steps/s" if sps == 1 else "simulation sub-steps/s"}
        for name, vec, tape, out, ts in runs:
            row[name] = rates(ts, K * R * sps)
        row["outputs_identical"] = bool(all(torch.equal(x, y) for x, y in zip(runs[0][3], runs[1][3])))
        row["new_over_parent_median"] = row["new"]["median"] / row["parent"]["median"]
        row["new_median_within_parent_range"] = bool(row["parent"]["min"] <= row["new"]["median"] <= row["parent"]["max"])
        res["legs"][leg] = row
        for name, vec, tape, out, ts in runs:
            vec.close()
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    import warnings
    warnings.simplefilter("ignore")
    main()
