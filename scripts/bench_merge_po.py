"""MergePOEnv (examples/exp_configs/rl/singleagent/singleagent_merge.py) on the queue-order kernel against the slot-order
kernel, and the closed loop the device trainer runs:
python scripts/bench_merge_po.py [--replicas 1024] [--steps 600] [--reps 5] [--out profiles/merge_po_bench.json]

In ONE process, one `steps`-step episode per launch:
  (a) open-loop rollout_dev with an action tape on k_merge_queue;
  (b) the same tape on k_steps_open -- a second handle created under FLOWSIM_NO_QUEUE=1.  (a) and (b) are timed
      alternately, `reps` times each after one warm-up launch; median, min and max of each;
  (c) the captured-graph closed loop (VecFlowEnv.capture around the torch GaussianPolicy(25, 5), resets in the graph).
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
    ts = [seconds(graph.replay) for _ in range(args.reps)]
    res["closed_loop_graph"] = {"last_kernel": step_kernel, "substeps_per_s": rates(ts, K * R * sps),
                                "env_steps_per_s": rates(ts, K * R)}
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
