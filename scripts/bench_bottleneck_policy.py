"""The closed loop of `train.py singleagent_bottleneck --rl_trainer device` (BottleneckDesiredVelocityEnv, 141 -> 20), as
captured HIP graphs of single steps, and where its time goes:
python scripts/bench_bottleneck_policy.py [--replicas 128 1024] [--steps 100] [--reps 7]
                                          [--out profiles/bottleneck_policy_graph_bench.json]

Per replica count, in ONE process, every leg a VecFlowEnv of its own with a graph of `steps` steps (resets in the graph):
  torch_graph          the graph around the torch GaussianPolicy(141, 20).act: the trainer's default path;
  kernel_graph         the graph around the policy kernel (k_policy_act_wide: the same weights as a DevicePolicy);
  *_noskip             both again on handles created under FLOWSIM_NO_MASK_SKIP=1: the masked warm-up launch of every
                       reset (40 steps of k_steps_open) runs in full for every replica;
  step_only            the step alone on an action tape (k_drop_queue), no reset;
  step_reset[_noskip]  step + masked reset on the tape: with torch_graph / kernel_graph, the policy's share.
The legs are replayed alternately, `reps` fragments each after one warm-up fragment (drifts of the clock hit all legs
alike); median, min and max of the env-steps/s, and the episodes that ended inside the timed fragments (a reset that
selects nobody is the cheapest the skip can make it).  One JSON object on stdout (and in --out)."""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

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
    return {"median": r[len(r) // 2], "min": r[0], "max": r[-1]}


def bench(fp, R, K, reps):
    from flow_amd.envs import VecFlowEnv
    from flow_amd.utils.device_policy import DevicePolicy
    from train_vec import GaussianPolicy
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    pi = None
    legs = {}

    def leg(name, kind, noskip):
        nonlocal pi
        if noskip:
            os.environ["FLOWSIM_NO_MASK_SKIP"] = "1"          # (read when a handle is created)
        try:
            vec = VecFlowEnv(fp, num_replicas=R, device=0)
        finally:
            os.environ.pop("FLOWSIM_NO_MASK_SKIP", None)
        if pi is None:
            pi = GaussianPolicy(vec.obs_dim, vec.act_dim).to(dev)
        vec.reset()
        if kind == "torch":
            graph = vec.capture(K, policy=pi.act, reset_done=True)
        elif kind == "kernel":
            pol = DevicePolicy([pi.mu[0], pi.mu[2]], pi.mu[4], log_std=pi.log_std, seed=0, act_dim=vec.act_dim)
            graph = vec.capture(K, policy=pol, reset_done=True)
        else:
            graph = vec.capture(K, policy=None, reset_done=kind == "step_reset")
            graph.actions.copy_((torch.rand((K, R, vec.act_dim), device=dev) * 2 - 1) * 1.5)
        graph.begin(vec.reset())
        graph.replay()                                       # warm-up fragment
        graph.synchronize()
        legs[name] = (vec, graph, [], [])

    leg("torch_graph", "torch", False)
    leg("kernel_graph", "kernel", False)
    leg("torch_graph_noskip", "torch", True)
    leg("kernel_graph_noskip", "kernel", True)
    leg("step_only", "step", False)
    leg("step_reset", "step_reset", False)
    leg("step_reset_noskip", "step_reset", True)
    torch.cuda.synchronize()
    for _ in range(reps):
        for vec, graph, ts, ended in legs.values():
            ts.append(seconds(graph.replay))
            ended.append(int((graph.done != 0).sum()))
    res = {"replicas": R, "steps": K, "reps": reps, "obs_dim": legs["torch_graph"][0].obs_dim,
           "act_dim": legs["torch_graph"][0].act_dim, "slots": legs["torch_graph"][0].sim.N}
    for name, (vec, graph, ts, ended) in legs.items():
        t = sorted(ts)
        res[name] = {"env_steps_per_s": rates(ts, K * R), "ms_per_fragment": {"median": t[len(t) // 2] * 1e3, "min": t[0] * 1e3,
                                                                            "max": t[-1] * 1e3},
                     "us_per_step": t[len(t) // 2] / K * 1e6, "episodes_ended": sum(ended)}
        vec.close()
    e = {k: res[k]["env_steps_per_s"] for k in legs}
    res["kernel_over_torch_median"] = e["kernel_graph"]["median"] / e["torch_graph"]["median"]
    res["kernel_min_above_torch_max"] = e["kernel_graph"]["min"] > e["torch_graph"]["max"]
    for a in ("torch_graph", "kernel_graph", "step_reset"):
        res[a + "_skip_over_noskip_median"] = e[a]["median"] / e[a + "_noskip"]["median"]
        res[a + "_skip_not_below_noskip_range"] = e[a]["median"] >= e[a + "_noskip"]["min"]
    us = {k: res[k]["us_per_step"] for k in legs}
    res["us_per_step_shares"] = {"step": us["step_only"], "reset": us["step_reset"] - us["step_only"],
                                 "reset_noskip": us["step_reset_noskip"] - us["step_only"],
                                 "torch_policy": us["torch_graph"] - us["step_reset"],
                                 "policy_kernel": us["kernel_graph"] - us["step_reset"]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, nargs="+", default=[128, 1024])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import importlib
    import flow_amd
    flow_amd.install_as_flow()
    fp = dict(importlib.import_module("exp_configs.rl.singleagent.singleagent_bottleneck").flow_params)
    fp["sim"] = copy.deepcopy(fp["sim"])
    fp["sim"].seed = 11                                    # (the experiment ships seed = None: a seed drawn per handle)
    torch.cuda.set_device(0)
    res = {"experiment": "singleagent_bottleneck", "device": torch.cuda.get_device_name(0),
           "runs": [bench(fp, R, args.steps, max(args.reps, 7)) for R in args.replicas]}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    import warnings
    warnings.simplefilter("ignore")
    main()
