"""adversarial_figure_eight (13 noisy IDM vehicles + 1 RL vehicle, AdversarialAccelEnv: two policies on the one RL vehicle) in
the closed loop, three ways:
python scripts/bench_adversarial.py [--replicas 1024 4096] [--steps 100] [--reps 7] [--parent_tree DIR]
                                    [--out profiles/adversarial_policy_bench.json]

In ONE process, per replica count one handle per form, one fragment of `steps` steps per launch, resets inside:
  (fused)        VecFlowEnv.policy_pair_rollout: one k_loop_policy<Adversarial> launch per fragment;
  (kernel_graph) the same fragment as a captured HIP graph of `steps` x (fs_policy_pair_act_dev, fs_step_dev(cmd),
                 fs_reset_dev(done)) launches: the only other way to keep the two-policy loop on the device;
  (single)       VecFlowEnv.policy_rollout with ONE policy on the same handle (k_loop_policy, AccelEnv head): the ceiling --
                 the fused pair evaluates two networks where it evaluates one.
The forms are timed alternately, `reps` fragments each after one warm-up fragment; median, min and max of each in
env-steps/s.  `fused_min_above_kernel_graph_max` is the bar: the fused form's slowest fragment against the graph's fastest.
--parent_tree DIR (a checkout of the parent commit with its library built): (single) is timed there too, in a child process
of the same run (--only_single --tree DIR), and `single_ranges_overlap_parent` says whether the shared body left
k_loop_policy where it was.  One JSON object on stdout (and in --out)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def seconds(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def rates(ts, work):
    r = sorted(work / t for t in ts)
    return {"median": r[len(r) // 2], "min": r[0], "max": r[-1]}


class PairGraph(object):
    """`steps` x (policy_pair_act_dev, step_dev(cmd), reset_dev(done)) captured once (VecFlowEnv.capture's recipe)."""

    def __init__(self, vec, av, adv, weight, K):
        import torch
        R, dev, sim = vec.num_envs, vec.device, vec.sim
        self.obs = torch.zeros((K + 1, R, vec.obs_dim), device=dev)
        self.act, self.logp = torch.zeros((K, 2, R), device=dev), torch.zeros((K, 2, R), device=dev)
        self.cmd, self.rew = torch.zeros((K, R, 1), device=dev), torch.zeros((K, R), device=dev)
        self.done = torch.zeros((K, R), dtype=torch.uint8, device=dev)
        self.carry = vec.reset().clone()
        torch.cuda.synchronize(dev)
        self.stream = torch.cuda.Stream(dev)
        names = []

        def body(steps):
            for k in range(steps):
                sim.policy_pair_act_dev(av.struct, adv.struct, weight, self.obs[k], self.act[k], self.logp[k], self.cmd[k])
                names.append(sim.last_kernel)
                sim.step_dev(self.obs[k + 1], self.rew[k], self.done[k], self.cmd[k])
                names.append(sim.last_kernel)
                sim.reset_dev(self.obs[k + 1], self.done[k])
        with torch.cuda.stream(self.stream):
            vec.use_current_stream()                         # bind BEFORE the capture: fs_set_stream synchronises
            self.obs[0].copy_(self.carry)
            body(2)                                          # eager warm-up: the draw counters and lazy host work
            sim.sync()
        self.stream.synchronize()
        self.kernels = "%s + %s + masked reset" % (names[0], names[1])
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=self.stream):
            self.obs[0].copy_(self.carry)
            body(K)
            self.carry.copy_(self.obs[K])
        self.torch = torch

    def replay(self):
        with self.torch.cuda.stream(self.stream):
            t = seconds(self.torch, self.graph.replay)
        return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent_tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--only_single", action="store_true", help="time the single-policy form alone (the child of --parent_tree)")
    ap.add_argument("--tree", default=ROOT, help="import flow_amd from this tree (with --only_single)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    import flow_amd
    from flow_amd.envs import VecFlowEnv
    from flow_amd.utils.device_policy import DevicePolicy
    from train_vec import GaussianPolicy
    flow_amd.install_as_flow()
    from exp_configs.rl.multiagent import adversarial_figure_eight as exp
    fp = exp.flow_params
    K = args.steps
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    res = {"experiment": "adversarial_figure_eight", "steps": K, "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "replicas": {}}
    legs, keep = [], []                                      # (R, form, timed call, times)
    for R in args.replicas:
        entry = {"kernels": {}}
        res["replicas"][str(R)] = entry
        pis = []
        for j in range(2):
            torch.manual_seed(j)
            pis.append(GaussianPolicy(28, 1).to(dev))
        pols = [DevicePolicy([pi.mu[0], pi.mu[2]], pi.mu[4], log_std=pi.log_std, seed=j) for j, pi in enumerate(pis)]
        single_v = VecFlowEnv(fp, num_replicas=R, device=0)
        single_v.reset()
        sout = single_v.policy_rollout(pols[0], K, reset_done=True)
        torch.cuda.synchronize()
        entry["kernels"]["single"] = single_v.sim.last_kernel
        legs.append((R, "single", lambda v=single_v, p=pols[0], o=sout: seconds(
            torch, lambda: v.policy_rollout(p, K, reset_done=True, out=o)), []))
        vecs = [single_v]
        if not args.only_single:
            weight = float(fp["env"].additional_params["perturb_weight"])
            entry["perturb_weight"] = weight
            fused_v, graph_v = VecFlowEnv(fp, num_replicas=R, device=0), VecFlowEnv(fp, num_replicas=R, device=0)
            vecs += [fused_v, graph_v]
            fused_v.reset()
            fout = fused_v.policy_pair_rollout(pols[0], pols[1], K, reset_done=True)
            torch.cuda.synchronize()
            entry["kernels"]["fused"] = fused_v.sim.last_kernel
            graph = PairGraph(graph_v, pols[0], pols[1], weight, K)
            graph.replay()
            entry["kernels"]["kernel_graph"] = graph.kernels
            legs.append((R, "fused", lambda v=fused_v, p=pols, o=fout: seconds(
                torch, lambda: v.policy_pair_rollout(p[0], p[1], K, reset_done=True, out=o)), []))
            legs.append((R, "kernel_graph", graph.replay, []))
            keep.append(graph)
        keep.append((vecs, pis, pols))
    for _ in range(args.reps):                               # alternately: drifts of the clock hit every form alike
        for _, _, fn, ts in legs:
            ts.append(fn())
    for R, form, _, ts in legs:
        res["replicas"][str(R)][form] = {"env_steps_per_s": rates(ts, K * R)}
    for item in keep:
        if isinstance(item, tuple):
            for v in item[0]:
                v.close()
    if not args.only_single:
        parent = None
        if args.parent_tree:
            child = subprocess.run([sys.executable, os.path.abspath(__file__), "--only_single", "--tree", args.parent_tree,
                                    "--steps", str(K), "--reps", str(args.reps), "--replicas"] + [str(r) for r in args.replicas],
                                   capture_output=True, text=True)
            if child.returncode != 0:
                raise SystemExit("bench_adversarial.py --parent_tree: the child failed:\n" + child.stderr[-2000:])
            parent = json.loads(child.stdout.strip().splitlines()[-1])
        for R, entry in res["replicas"].items():
            f, g, s = (entry[k]["env_steps_per_s"] for k in ("fused", "kernel_graph", "single"))
            entry["fused_over_kernel_graph_median"] = f["median"] / g["median"]
            entry["fused_over_single_median"] = f["median"] / s["median"]
            entry["fused_min_above_kernel_graph_max"] = f["min"] > g["max"]
            if parent is not None:
                p = parent["replicas"][R]["single"]["env_steps_per_s"]
                entry["single_parent"] = {"env_steps_per_s": p}
                entry["single_over_parent_median"] = s["median"] / p["median"]
                entry["single_ranges_overlap_parent"] = s["max"] >= p["min"] and p["max"] >= s["min"]
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    import warnings
    warnings.simplefilter("ignore")
    main()
