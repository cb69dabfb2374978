"""What the MultiWaveAttenuationPOEnv head costs in a fused fragment, next to the head it was derived from:
python scripts/bench_multi_ring.py [--rows 1024 4096] [--reps 7] [--parent_tree DIR] [--out profiles/multi_ring_policy_bench.json]

lord_of_the_rings.py as shipped (one ring per row, 21 noisy IDM vehicles + 1 RL vehicle, horizon 3000, warm-up 750) and
singleagent_ring.py as shipped, fragments of 100 closed-loop steps, per number of rows, in ONE process, `reps` fragments per
form, the forms alternated, on a device-synchronised host clock:
  fused_head4    k_ring_policy<MultiRing>: policy, action, step, reset in one launch (fs_policy_rollout_dev)
  graph_head4    the same fragment as a captured HIP graph around k_policy_act + fs_step_dev + masked fs_reset_dev
  fused_head1    k_ring_policy (WaveAttenuationPOEnv) on a singleagent_ring handle of the same rows
  parent_head1   fused_head1 on the library of --parent_tree DIR (a checkout of the parent commit with its library built), in a
                 child process of this run
Per step the new head adds two exact divisions per lane (the on-edge test of its two vehicles) and one masked reduction per
row to HEAD 1.  `head1_overlaps_parent`: the [min, max] ranges of fused_head1 and parent_head1 overlap -- the shared code was
not disturbed.  One JSON object on stdout (and in --out)."""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 100


def seconds(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def spread(values):
    v = sorted(values)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def rates(ts, rows):
    s = spread(ts)
    return {"seconds": s, "env_steps_per_s": {"median": STEPS * rows / s["median"], "min": STEPS * rows / s["max"],
                                              "max": STEPS * rows / s["min"]}}


def setup(tree):
    sys.path.insert(0, os.path.join(os.path.abspath(tree), "examples"))
    sys.path.insert(0, os.path.abspath(tree))
    import torch
    import flow_amd
    flow_amd.install_as_flow()
    torch.cuda.set_device(0)
    return torch


def device_policy(torch, vec, greedy=False):
    from flow_amd.utils.device_policy import DevicePolicy
    from train_vec import GaussianPolicy
    torch.manual_seed(0)
    pi = GaussianPolicy(vec.obs_dim, vec.act_dim).to(vec.device)
    return DevicePolicy([pi.mu[0], pi.mu[2]], pi.mu[4], log_std=pi.log_std, seed=0, greedy=greedy)


def fused_leg(torch, module, rows):
    """(timed callable, kernel name, env) of 100-step fused fragments of the experiment `module` at `rows` rows."""
    from flow_amd.envs import VecFlowEnv
    fp = dict(importlib.import_module(module).flow_params)
    vec = VecFlowEnv(fp, num_replicas=rows, device=0, seed=7)
    pol = device_policy(torch, vec)
    vec.reset()
    out = vec.policy_rollout(pol, STEPS, reset_done=True)              # warm-up
    kernel = vec.sim.last_kernel

    def timed():
        vec.use_current_stream()
        return seconds(torch, lambda: vec.policy_rollout(pol, STEPS, reset_done=True, out=out))
    return timed, kernel, vec


def child(args):
    """--child: `reps` fused fragments of singleagent_ring at --rows[0] on the tree of --tree."""
    torch = setup(args.tree)
    timed, kernel, vec = fused_leg(torch, "exp_configs.rl.singleagent.singleagent_ring", args.rows[0])
    ts = [timed() for _ in range(args.reps)]
    vec.close()
    print(json.dumps({"seconds": ts, "kernel": kernel, "tree": args.tree}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent_tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--child", action="store_true", help="(child) time fused_head1 on --tree")
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    if args.child:
        return child(args)
    torch = setup(ROOT)
    from flow_amd.envs import VecFlowEnv
    res = {"steps": STEPS, "reps": args.reps, "device": torch.cuda.get_device_name(0), "clock": "host, device-synchronised",
           "rows": {}}
    for rows in args.rows:
        legs, keep = [], []
        lord = "exp_configs.rl.multiagent.lord_of_the_rings"
        t4, k4, v4 = fused_leg(torch, lord, rows)
        legs.append(("fused_head4", k4, t4, []))
        # the same fragment as a captured graph around the eager policy kernel
        vg = VecFlowEnv(dict(importlib.import_module(lord).flow_params), num_replicas=rows, device=0, seed=7)
        pg = device_policy(torch, vg)
        vg.reset()
        vg.policy_act(pg)
        graph = vg.capture(STEPS, policy=pg, reset_done=True)
        graph.begin(vg.reset())
        graph.replay()
        graph.synchronize()                                            # warm-up

        def replay(graph=graph):
            def run():
                graph.replay()
                graph.synchronize()
            return seconds(torch, run)
        legs.append(("graph_head4", "k_policy_act + " + vg.sim.last_kernel, replay, []))
        t1, k1, v1 = fused_leg(torch, "exp_configs.rl.singleagent.singleagent_ring", rows)
        legs.append(("fused_head1", k1, t1, []))
        keep += [v4, vg, v1]
        for _ in range(args.reps):                                     # alternately: drifts of the clock hit every leg alike
            for _, _, fn, ts in legs:
                ts.append(fn())
        entry = {"vehicles": v4.sim.N, "num_rings": v4.num_rings}
        for name, kernel, _, ts in legs:
            entry[name] = dict(rates(ts, rows), kernel=kernel)
        for v in keep:
            v.close()
        if args.parent_tree:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", args.parent_tree, "--rows", str(rows),
                   "--reps", str(args.reps)]
            run = subprocess.run(cmd, capture_output=True, text=True)
            if run.returncode != 0:
                raise SystemExit("bench_multi_ring.py: the child on %s failed:\n%s" % (args.parent_tree, run.stderr[-2000:]))
            got = json.loads(run.stdout.strip().splitlines()[-1])
            entry["parent_head1"] = dict(rates(got["seconds"], rows), kernel=got["kernel"])
            a, b = entry["fused_head1"]["seconds"], entry["parent_head1"]["seconds"]
            entry["head1_overlaps_parent"] = a["min"] <= b["max"] and b["min"] <= a["max"]
            entry["head1_over_parent_median"] = a["median"] / b["median"]
        entry["head4_over_head1_median"] = entry["fused_head4"]["seconds"]["median"] / entry["fused_head1"]["seconds"]["median"]
        entry["graph_over_fused_head4_median"] = entry["graph_head4"]["seconds"]["median"] / entry["fused_head4"]["seconds"]["median"]
        res["rows"][str(rows)] = entry
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    import warnings
    warnings.simplefilter("ignore")
    main()
