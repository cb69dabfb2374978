"""MergePOEnv with more than six places -- EXP_NUM 1 and 2 of examples/exp_configs/rl/singleagent/singleagent_merge.py, 13 and
17 controlled places -- in the closed loop, three ways, next to the open loop of the same run:
python scripts/bench_merge_po_wide.py [--replicas 1024] [--steps 600] [--reps 7] [--out profiles/merge_po_wide_policy_bench.json]

In ONE process, per experiment one handle per route, one fragment of `steps` steps per launch:
  (tape)         open-loop rollout_dev with an action tape on k_merge_queue, from a reset: what the simulator alone costs;
  (torch_graph)  VecFlowEnv.capture around the torch GaussianPolicy(5 num_rl, num_rl), resets in the graph: the only closed
                 loop these experiments had before the wide head, and the baseline;
  (kernel_graph) VecFlowEnv.capture around the eager policy kernel (a DevicePolicy with act_dim = num_rl: k_policy_act_wide);
  (fused)        VecFlowEnv.policy_rollout: one k_merge_policy<PO,WIDE> launch per fragment, resets in the kernel.
The routes of both experiments are timed alternately, `reps` fragments each after one warm-up fragment; median, min and max
of each in env-steps/s.  `fused_min_above_torch_graph_max` is the bar: the fused route's slowest fragment against the torch
graph's fastest.  One JSON object on stdout (and in --out)."""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

import torch

from bench_merge_po import rates, seconds


def experiment_params(exp):
    """flow_params of singleagent_merge.py with EXP_NUM = exp (the file selects its experiment by that constant)."""
    path = os.path.join(ROOT, "examples", "exp_configs", "rl", "singleagent", "singleagent_merge.py")
    with open(path) as f:
        text = f.read()
    assert text.count("EXP_NUM = 0\n") == 1
    scope = {"__name__": "singleagent_merge_exp%d" % exp}
    exec(compile(text.replace("EXP_NUM = 0\n", "EXP_NUM = %d\n" % exp), path, "exec"), scope)
    fp = dict(scope["flow_params"])
    fp["sim"] = copy.deepcopy(fp["sim"])
    fp["sim"].seed = 11                                    # (the experiment ships seed = None: a seed drawn per handle)
    return fp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import flow_amd
    from flow_amd.envs import VecFlowEnv
    from flow_amd.utils.device_policy import DevicePolicy
    from train_vec import GaussianPolicy
    flow_amd.install_as_flow()
    R, K = args.replicas, args.steps
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    res = {"experiment": "singleagent_merge", "replicas": R, "steps": K, "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "experiments": {}}
    legs = []                                              # (exp, route, timed call, times)
    keep = []
    for exp in (1, 2):
        fp = experiment_params(exp)
        vecs = [VecFlowEnv(fp, num_replicas=R, device=0) for _ in range(4)]
        tape_v, torch_v, kern_v, fused_v = vecs
        A, D = tape_v.act_dim, tape_v.obs_dim
        pi = GaussianPolicy(D, A).to(dev)
        entry = {"num_rl": A, "obs_dim": D, "sims_per_step": int(tape_v.sim.spec.get("sims_per_step", 1)), "kernels": {}}
        res["experiments"]["EXP_NUM=%d" % exp] = entry
        # the tape: one episode from a reset
        tape = ((torch.rand((K, R, A), device=dev) * 2 - 1) * 1.5).contiguous()
        out = (torch.empty((K, R, D), device=dev), torch.empty((K, R), device=dev),
               torch.empty((K, R), dtype=torch.uint8, device=dev))

        def run_tape(v=tape_v, out=out, tape=tape):
            v.reset()
            torch.cuda.synchronize()
            return seconds(lambda: v.sim.rollout_dev(K, *out, actions=tape))
        run_tape()
        entry["kernels"]["tape"] = tape_v.sim.last_kernel
        # the captured graph around the torch policy
        torch_v.reset()
        g_torch = torch_v.capture(K, policy=pi.act, reset_done=True)
        g_torch.begin(torch_v.reset())
        g_torch.replay()
        entry["kernels"]["torch_graph"] = "torch modules + k_merge_queue"
        # the captured graph around the eager policy kernel
        pol_g = DevicePolicy([pi.mu[0], pi.mu[2]], pi.mu[4], log_std=pi.log_std, seed=0, act_dim=A)
        kern_v.reset()
        kern_v.policy_act(pol_g)
        entry["kernels"]["kernel_graph"] = kern_v.sim.last_kernel + " + k_merge_queue"
        g_kern = kern_v.capture(K, policy=pol_g, reset_done=True)
        g_kern.begin(kern_v.reset())
        g_kern.replay()
        # the fused kernel
        pol_f = DevicePolicy([pi.mu[0], pi.mu[2]], pi.mu[4], log_std=pi.log_std, seed=0, act_dim=A)
        fused_v.reset()
        fout = fused_v.policy_rollout(pol_f, K, reset_done=True)
        torch.cuda.synchronize()
        entry["kernels"]["fused"] = fused_v.sim.last_kernel
        legs += [(exp, "tape", run_tape, []),
                 (exp, "torch_graph", lambda g=g_torch: seconds(g.replay), []),
                 (exp, "kernel_graph", lambda g=g_kern: seconds(g.replay), []),
                 (exp, "fused", lambda v=fused_v, p=pol_f, o=fout: seconds(lambda: v.policy_rollout(p, K, reset_done=True, out=o)), [])]
        keep.append((vecs, pi, pol_g, pol_f, g_torch, g_kern))
    for _ in range(args.reps):                             # alternately: drifts of the clock hit every route alike
        for _, _, fn, ts in legs:
            ts.append(fn())
    for exp, route, _, ts in legs:
        res["experiments"]["EXP_NUM=%d" % exp][route] = {"env_steps_per_s": rates(ts, K * R)}
    for entry in res["experiments"].values():
        f, t, g, k = (entry[r]["env_steps_per_s"] for r in ("fused", "tape", "torch_graph", "kernel_graph"))
        entry["fused_over_tape_median"] = f["median"] / t["median"]
        entry["fused_over_torch_graph_median"] = f["median"] / g["median"]
        entry["fused_over_kernel_graph_median"] = f["median"] / k["median"]
        entry["kernel_graph_over_torch_graph_median"] = k["median"] / g["median"]
        entry["fused_min_above_torch_graph_max"] = f["min"] > g["max"]
        entry["fused_min_above_kernel_graph_max"] = f["min"] > k["max"]
    for vecs, *_ in keep:
        for v in vecs:
            v.close()
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    import warnings
    warnings.simplefilter("ignore")
    main()
