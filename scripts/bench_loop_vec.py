"""figureeight1 (7 noisy IDM + 7 RL vehicles, one network 28 -> 7) and figureeight2 (14 RL vehicles, 28 -> 14) as shipped in
flow_amd/benchmarks, in the closed loop:
python scripts/bench_loop_vec.py [--replicas 1024 4096] [--steps 100] [--reps 7] [--parent_lib PATH]
                                 [--out profiles/loop_vec_policy_bench.json]

In ONE process, per experiment and replica count one handle per form, one fragment of `steps` steps per launch, resets
inside:
  (fused)        VecFlowEnv.policy_rollout: one k_loop_policy<AccelVec> launch per fragment;
  (kernel_graph) the same fragment as a captured HIP graph of `steps` x (fs_policy_act_dev = k_policy_act_row, fs_step_dev,
                 fs_reset_dev(done)) launches (VecFlowEnv.capture with the DevicePolicy);
  (torch_graph)  the same as a captured graph around the torch module (VecFlowEnv.capture with GaussianPolicy.act): the
                 path train.py takes without --fuse_policy;
  (single)       k_loop_policy (AccelEnv head, ONE RL vehicle) on a singleagent_figure_eight handle of the same size: what
                 the action-vector head costs next to the scalar one.
The forms are timed alternately, `reps` fragments each after one warm-up fragment, on the host clock between device
synchronisations; median, min and max of each in env-steps/s.
--parent_lib PATH (libflowsim.so built from the parent commit; the C ABI and the Python side of (single) are the same):
(single) is timed in child processes of the same run (--only_single, FLOWSIM_LIB), this library's and the parent's, in
both orders; `single_ranges_overlap_parent` says per order whether the shared body left k_loop_policy where it was.
One JSON object on stdout (and in --out)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def seconds(torch, fn, wait=None):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    (wait or torch.cuda.synchronize)()
    return time.perf_counter() - t0


def rates(ts, work):
    r = sorted(work / t for t in ts)
    return {"median": r[len(r) // 2], "min": r[0], "max": r[-1]}


def overlap(a, b):
    return a["max"] >= b["min"] and b["max"] >= a["min"]


def single_child(lib, args):
    env = dict(os.environ)
    if lib:
        env["FLOWSIM_LIB"] = os.path.abspath(lib)
    else:
        env.pop("FLOWSIM_LIB", None)
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--only_single", "--steps", str(args.steps), "--reps",
                            str(args.reps), "--replicas"] + [str(r) for r in args.replicas], capture_output=True, text=True,
                           env=env)
    if child.returncode != 0:
        raise SystemExit("bench_loop_vec.py: the --only_single child failed:\n" + child.stderr[-2000:])
    return json.loads(child.stdout.strip().splitlines()[-1])["single"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent_lib", default=None, help="libflowsim.so built from the parent commit")
    ap.add_argument("--only_single", action="store_true", help="time the single-policy form alone (the children of --parent_lib)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    sys.path.insert(0, ROOT)
    import importlib
    import torch
    import flow_amd
    from flow_amd.envs import VecFlowEnv
    from flow_amd.utils.device_policy import DevicePolicy
    from train_vec import GaussianPolicy
    flow_amd.install_as_flow()
    from exp_configs.rl.singleagent import singleagent_figure_eight as single_exp
    K = args.steps
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    res = {"steps": K, "reps": args.reps, "device": torch.cuda.get_device_name(0), "clock": "host, device-synchronised",
           "single": {}, "experiments": {}}
    legs, keep = [], []                                      # (where the rates go, work, timed call, times)

    def policy(A, seed):
        torch.manual_seed(seed)
        pi = GaussianPolicy(28, A).to(dev)
        return pi, DevicePolicy([pi.mu[0], pi.mu[2]], pi.mu[4], log_std=pi.log_std, seed=seed, act_dim=A)

    for R in args.replicas:
        pi, pol = policy(1, 0)
        vec = VecFlowEnv(single_exp.flow_params, num_replicas=R, device=0)
        vec.reset()
        out = vec.policy_rollout(pol, K, reset_done=True)
        torch.cuda.synchronize()
        entry = res["single"][str(R)] = {"experiment": "singleagent_figure_eight", "kernel": vec.sim.last_kernel}
        legs.append((entry, K * R, lambda v=vec, p=pol, o=out: seconds(
            torch, lambda: v.policy_rollout(p, K, reset_done=True, out=o)), []))
        keep.append((vec, pi, pol))
    for name in ([] if args.only_single else ["figureeight1", "figureeight2"]):
        fp = importlib.import_module("flow.benchmarks." + name).flow_params
        exp = res["experiments"][name] = {}
        for R in args.replicas:
            entry = exp[str(R)] = {"kernels": {}}
            fused_v, kg_v, tg_v = (VecFlowEnv(fp, num_replicas=R, device=0) for _ in range(3))
            A = fused_v.act_dim
            entry["num_rl"] = A
            pi, pol = policy(A, 1)
            fused_v.reset()
            fout = fused_v.policy_rollout(pol, K, reset_done=True)
            torch.cuda.synchronize()
            entry["kernels"]["fused"] = fused_v.sim.last_kernel
            kg_v.reset()
            kg_v.policy_act(pol)
            entry["kernels"]["kernel_graph"] = "%s + step + masked reset" % kg_v.sim.last_kernel
            kgraph = kg_v.capture(K, policy=pol, reset_done=True)
            kgraph.begin(kg_v.reset())
            tgraph = tg_v.capture(K, policy=pi.act, reset_done=True)
            tgraph.begin(tg_v.reset())
            entry["kernels"]["torch_graph"] = "torch module + step + masked reset"
            for form, call, wait in (
                    ("fused", lambda v=fused_v, p=pol, o=fout: v.policy_rollout(p, K, reset_done=True, out=o), None),
                    ("kernel_graph", kgraph.replay, kgraph.synchronize), ("torch_graph", tgraph.replay, tgraph.synchronize)):
                entry[form] = {}
                call()                                       # the warm-up fragment
                torch.cuda.synchronize()
                legs.append((entry[form], K * R, lambda c=call, w=wait: seconds(torch, c, w), []))
            keep.append((fused_v, kg_v, tg_v, pi, pol, kgraph, tgraph))
    for _ in range(args.reps):                               # alternately: drifts of the clock hit every form alike
        for _, _, fn, ts in legs:
            ts.append(fn())
    for entry, work, _, ts in legs:
        entry["env_steps_per_s"] = rates(ts, work)
    for item in keep:
        for v in item:
            if isinstance(v, VecFlowEnv):
                v.close()
    if not args.only_single:
        for name, exp in res["experiments"].items():
            for R, entry in exp.items():
                f, g, t = (entry[k]["env_steps_per_s"] for k in ("fused", "kernel_graph", "torch_graph"))
                s = res["single"][R]["env_steps_per_s"]
                entry["fused_over_kernel_graph_median"] = f["median"] / g["median"]
                entry["fused_over_torch_graph_median"] = f["median"] / t["median"]
                entry["fused_over_single_median"] = f["median"] / s["median"]
                entry["fused_min_above_kernel_graph_max"] = f["min"] > g["max"]
        if args.parent_lib:
            orders = res["single_children"] = []
            for order in (("this", "parent"), ("parent", "this")):
                got = {who: single_child(args.parent_lib if who == "parent" else None, args) for who in order}
                row = {"order": list(order)}
                for R in res["single"]:
                    a, b = got["this"][R]["env_steps_per_s"], got["parent"][R]["env_steps_per_s"]
                    row[R] = {"this": a, "parent": b, "this_over_parent_median": a["median"] / b["median"],
                              "single_ranges_overlap_parent": overlap(a, b)}
                orders.append(row)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    import warnings
    warnings.simplefilter("ignore")
    main()
