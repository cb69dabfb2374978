"""What fs_policy.greedy costs the sampling path of the fused policy kernels, and what the episode statistics cost the log:
python scripts/bench_policy_greedy.py [--replicas 1024 4096] [--steps 100] [--reps 7] [--parent_tree DIR]
                                      [--out profiles/policy_greedy_bench.json]

In ONE process, per replica count one handle per form, one fragment of `steps` steps per launch with resets inside:
  (ring)        k_ring_policy: examples/train_vec.py's ring (21 IDM + 1 RL vehicle, WaveAttenuationPOEnv), sampling;
  (ring_greedy) the same with the mean action (DevicePolicy.greedy);
  (loop)        k_loop_policy: singleagent_figure_eight (AccelEnv head), sampling;
  (merge_po)    k_merge_policy<PO>: singleagent_merge (five places), sampling;
  (episode_stats) one VecFlowEnv.episode_stats call on the ring fragment's rew / done [steps, R], timed on its own right
                after the fragment it follows: what --episode_stats adds to an iteration.
A device-synchronised host clock around each launch, one warm-up fragment per form, then `reps` fragments per form, the
forms alternated; median, min and max of each in env-steps/s (episode_stats: seconds per call).
--parent_tree DIR (a checkout of the parent commit with its library built): the three sampling forms are timed there too,
in a child process of the same run (--only_sampling --tree DIR), next to a child of the same shape on THIS tree
(`sampling_child`: the same handles in the same order, so that the two differ in the library alone -- the main process
holds more handles and times more forms); per form `over_parent_median` and `ranges_overlap_parent` compare those two and
say whether the flag left the sampling path where it was -- the project's condition: the range over the fragments
overlaps the parent's range measured in the same run.  The pair of children runs a second time in the other order
(`parent_first`), because the child that runs second finds the device warmer: recorded next to the condition.  The greedy
rate is recorded, not held to anything.  One JSON object on stdout (and in --out)."""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLING = ("ring", "loop", "merge_po")


def seconds(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def spread(values):
    v = sorted(values)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent_tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--only_sampling", action="store_true", help="time the sampling forms alone (the child of --parent_tree)")
    ap.add_argument("--tree", default=ROOT, help="import flow_amd from this tree (with --only_sampling)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    import flow_amd
    from flow_amd.envs import VecFlowEnv
    from flow_amd.utils.device_policy import DevicePolicy
    from train_vec import GaussianPolicy, ring_flow_params
    flow_amd.install_as_flow()
    params = {"ring": ring_flow_params(500),
              "loop": importlib.import_module("exp_configs.rl.singleagent.singleagent_figure_eight").flow_params,
              "merge_po": dict(importlib.import_module("exp_configs.rl.singleagent.singleagent_merge").flow_params)}
    K = args.steps
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    res = {"steps": K, "reps": args.reps, "device": torch.cuda.get_device_name(0), "clock": "host, device-synchronised",
           "replicas": {}}
    legs, keep = [], []                                      # (R, form, timed call, times, work per call)
    forms = SAMPLING if args.only_sampling else ("ring", "ring_greedy", "loop", "merge_po")
    for R in args.replicas:
        entry = {"kernels": {}}
        res["replicas"][str(R)] = entry
        for form in forms:
            vec = VecFlowEnv(params["ring" if form == "ring_greedy" else form], num_replicas=R, device=0)
            vector = form == "merge_po"                      # (ONE network, an action vector)
            torch.manual_seed(0)
            pi = GaussianPolicy(vec.obs_dim, vec.act_dim).to(dev)
            pol = DevicePolicy([pi.mu[0], pi.mu[2]], pi.mu[4], log_std=pi.log_std, seed=0, **(dict(act_dim=vec.act_dim) if vector else {}))
            if form == "ring_greedy":
                pol.greedy = True
            vec.reset()
            out = vec.policy_rollout(pol, K, reset_done=True)          # warm-up launch (and the buffers of the timed ones)
            torch.cuda.synchronize()
            entry["kernels"][form] = vec.sim.last_kernel
            legs.append((R, form, lambda v=vec, p=pol, o=out: seconds(
                torch, lambda: v.policy_rollout(p, K, reset_done=True, out=o)), [], K * R))
            if form == "ring" and not args.only_sampling:
                vec.episode_stats(out[3], out[4], reset=True)          # (warm-up: the buffers and the library's scratch)
                torch.cuda.synchronize()
                entry["kernels"]["episode_stats"] = vec.sim.last_kernel
                legs.append((R, "episode_stats", lambda v=vec, o=out: seconds(
                    torch, lambda: v.episode_stats(o[3], o[4], accumulate=False)), [], None))
            keep.append((vec, pi, pol, out))
    for _ in range(args.reps):                               # alternately: drifts of the clock hit every form alike
        for _, _, fn, ts, _ in legs:
            ts.append(fn())
    for R, form, _, ts, work in legs:
        if work is None:
            res["replicas"][str(R)][form] = {"seconds_per_call": spread(ts)}
        else:
            res["replicas"][str(R)][form] = {"env_steps_per_s": spread([work / t for t in ts]), "seconds_per_fragment": spread(ts)}
    for item in keep:
        item[0].close()
    if not args.only_sampling:
        def child(tree):
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "--only_sampling", "--tree", tree, "--steps", str(K),
                                  "--reps", str(args.reps), "--replicas"] + [str(r) for r in args.replicas],
                                 capture_output=True, text=True)
            if run.returncode != 0:
                raise SystemExit("bench_policy_greedy.py --parent_tree: the child on %s failed:\n%s" % (tree, run.stderr[-2000:]))
            return json.loads(run.stdout.strip().splitlines()[-1])
        here, parent = (child(ROOT), child(args.parent_tree)) if args.parent_tree else (None, None)
        # ... and once more in the other order (the child that runs second finds the device warmer): recorded, not the condition
        parent2, here2 = (child(args.parent_tree), child(ROOT)) if args.parent_tree else (None, None)
        for R, entry in res["replicas"].items():
            entry["greedy_over_sampling_median"] = (entry["ring_greedy"]["env_steps_per_s"]["median"] /
                                                    entry["ring"]["env_steps_per_s"]["median"])
            entry["episode_stats_over_fragment_median"] = (entry["episode_stats"]["seconds_per_call"]["median"] /
                                                           entry["ring"]["seconds_per_fragment"]["median"])
            if parent is not None:
                for form in SAMPLING:
                    s, p = here["replicas"][R][form]["env_steps_per_s"], parent["replicas"][R][form]["env_steps_per_s"]
                    entry[form]["sampling_child"] = {"env_steps_per_s": s, "kernel": here["replicas"][R]["kernels"][form]}
                    entry[form]["parent"] = {"env_steps_per_s": p, "kernel": parent["replicas"][R]["kernels"][form]}
                    entry[form]["over_parent_median"] = s["median"] / p["median"]
                    entry[form]["ranges_overlap_parent"] = s["max"] >= p["min"] and p["max"] >= s["min"]
                    s2, p2 = here2["replicas"][R][form]["env_steps_per_s"], parent2["replicas"][R][form]["env_steps_per_s"]
                    entry[form]["parent_first"] = {"sampling_child": s2, "parent": p2, "over_parent_median": s2["median"] / p2["median"],
                                                   "ranges_overlap_parent": s2["max"] >= p2["min"] and p2["max"] >= s2["min"]}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    import warnings
    warnings.simplefilter("ignore")
    main()
