"""MergePOEnv (examples/exp_configs/rl/singleagent/singleagent_merge.py) on the queue-order kernel against the slot-order
kernel, and the closed loop the device trainer runs:
python scripts/bench_merge_po.py [--replicas 1024] [--steps 600] [--reps 5] [--out profiles/merge_po_policy_bench.json]
python scripts/bench_merge_po.py --fused_only      # one reset and two fused fragments, nothing else: the run to profile

In ONE process, one `steps`-step episode per launch:
  (a) open-loop rollout_dev with an action tape on k_merge_queue;
  (b) the same tape on k_steps_open -- a second handle created under FLOWSIM_NO_QUEUE=1.  (a) and (b) are timed
      alternately, `reps` times each after one warm-up launch; median, min and max of each;
  (c) the captured-graph closed loop (VecFlowEnv.capture around the torch GaussianPolicy(25, 5), resets in the graph);
  (d) the fused closed loop (VecFlowEnv.policy_rollout: k_merge_policy<PO>, the same GaussianPolicy's weights as a
      DevicePolicy with act_dim = 5, resets in the kernel) on a handle of the same shape.  (c) and (d) are timed
      alternately, `reps` times each; (d) is reported against (c) -- `fused_min_above_graph_max`: the ranges do not
      overlap -- and against (a), the open loop of the same run: what the policy costs.
Sub-steps/s and env-steps/s, and the kernel each leg reported.  One JSON object on stdout (and in --out)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--fused_only", action="store_true", help="leg (d) alone, two fragments (for rocprofv3 --kernel-trace)")
    args = ap.parse_args()
    import importlib
    import flow_amd
    from flow_amd.envs import VecFlowEnv
    from train_vec import GaussianPolicy
    flow_amd.install_as_flow()
    fp = dict(importlib.import_module("exp_configs.rl.singleagent.singleagent_merge").flow_params)
    fp["sim"] = copy.deepcopy(fp["sim"])
    fp["sim"].seed = 11                                    # (the experiment ships seed = None: a seed drawn per handle)
    R, K = args.replicas, args.steps
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    if args.fused_only:
        from flow_amd.utils.device_policy import DevicePolicy
        vec = VecFlowEnv(fp, num_replicas=R, device=0)
        pi = GaussianPolicy(vec.obs_dim, vec.act_dim).to(dev)
        pol = DevicePolicy([pi.mu[0], pi.mu[2]], pi.mu[4], log_std=pi.log_std, seed=0, act_dim=vec.act_dim)
        vec.reset()
        out = vec.policy_rollout(pol, K, reset_done=True)
        vec.policy_rollout(pol, K, reset_done=True, out=out)
        torch.cuda.synchronize()
        print(json.dumps({"fused_only": vec.sim.last_kernel, "replicas": R, "steps": K}))
        vec.close()
        return
    queue = VecFlowEnv(fp, num_replicas=R, device=0)
    os.environ["FLOWSIM_NO_QUEUE"] = "1"                  # (read when a handle is created)
    try:
        slot = VecFlowEnv(fp, num_replicas=R, device=0)
    finally:
        os.environ.pop("FLOWSIM_NO_QUEUE")
    sps = int(queue.sim.spec.get("sims_per_step", 1))
    A = queue.act_dim
    tape = ((torch.rand((K, R, A), device=dev) * 2 - 1) * 1.5).contiguous()
    res = {"experiment": "singleagent_merge", "replicas": R, "steps": K, "reps": args.reps, "sims_per_step": sps,
           "obs_dim": queue.obs_dim, "act_dim": A, "device": torch.cuda.get_device_name(0)}

    def episode(vec, out):
        vec.reset()
        vec.sim.rollout_dev(K, *out, actions=tape)

    legs = []
    for vec in (queue, slot):
        out = (torch.empty((K, R, vec.obs_dim), device=dev), torch.empty((K, R), device=dev),
               torch.empty((K, R), dtype=torch.uint8, device=dev))
        episode(vec, out)                                  # warm-up launch
        torch.cuda.synchronize()
        legs.append((vec, out, vec.sim.last_kernel, []))
    for _ in range(args.reps):                             # alternately: drifts of the clock hit both legs alike
        for vec, out, _, ts in legs:
            vec.reset()
            torch.cuda.synchronize()
            ts.append(seconds(lambda: vec.sim.rollout_dev(K, *out, actions=tape)))
    for key, (vec, out, kernel, ts) in zip(("queue_order", "slot_order"), legs):
        res[key] = {"last_kernel": kernel, "substeps_per_s": rates(ts, K * R * sps), "env_steps_per_s": rates(ts, K * R)}
    same = all(torch.equal(x, y) for x, y in zip(legs[0][1], legs[1][1]))
    res["outputs_identical"] = bool(same)
    res["queue_over_slot_median"] = res["queue_order"]["substeps_per_s"]["median"] / res["slot_order"]["substeps_per_s"]["median"]
    res["queue_min_above_slot_max"] = res["queue_order"]["substeps_per_s"]["min"] > res["slot_order"]["substeps_per_s"]["max"]
    slot.close()
    # (c) the closed loop of `train.py singleagent_merge --rl_trainer device`
    pi = GaussianPolicy(queue.obs_dim, A).to(dev)
    queue.reset()
    queue.step(tape[0])                                    # (the kernel of the step the graph records: the graph's last
    step_kernel = queue.sim.last_kernel                    # launch is the masked reset's observation, on k_steps_open)
    graph = queue.capture(K, policy=pi.act, reset_done=True)
    graph.begin(queue.reset())
    graph.replay()
    torch.cuda.synchronize()
    # (d) the fused closed loop: the same weights, one launch per fragment
    from flow_amd.utils.device_policy import DevicePolicy
    fusedv = VecFlowEnv(fp, num_replicas=R, device=0)
    pol = DevicePolicy([pi.mu[0], pi.mu[2]], pi.mu[4], log_std=pi.log_std, seed=0, act_dim=A)
    fusedv.reset()
    fout = fusedv.policy_rollout(pol, K, reset_done=True)  # warm-up launch (and the buffers of the timed ones)
    torch.cuda.synchronize()
    fused_kernel = fusedv.sim.last_kernel
    ts, tf = [], []
    for _ in range(max(args.reps, 5)):                     # alternately, as (a) and (b)
        ts.append(seconds(graph.replay))
        tf.append(seconds(lambda: fusedv.policy_rollout(pol, K, reset_done=True, out=fout)))
    res["closed_loop_graph"] = {"last_kernel": step_kernel, "substeps_per_s": rates(ts, K * R * sps),
                                "env_steps_per_s": rates(ts, K * R)}
    res["closed_loop_fused"] = {"last_kernel": fused_kernel, "substeps_per_s": rates(tf, K * R * sps),
                                "env_steps_per_s": rates(tf, K * R)}
    g, f, o = (res[k]["env_steps_per_s"] for k in ("closed_loop_graph", "closed_loop_fused", "queue_order"))
    res["fused_over_graph_median"] = f["median"] / g["median"]
    res["fused_min_above_graph_max"] = f["min"] > g["max"]
    res["fused_over_open_loop_median"] = f["median"] / o["median"]
    fusedv.close()
    queue.close()
    text = json.dumps(res, indent=1)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    import warnings
    warnings.simplefilter("ignore")
    main()
