"""What a snapshot of a handle costs (fs_snapshot_dev / fs_restore_dev: k_snapshot), and what in-training evaluation adds:
python scripts/bench_snapshot.py [--replicas 1024] [--reps 7] [--parent_tree DIR] [--out profiles/snapshot_bench.json]

Per shape -- singleagent_ring (22 vehicles) and singleagent_bottleneck as shipped -- in ONE process, two handles: one as
shipped and one created with FLOWSIM_SNAPSHOT_COPIES=1, whose unmasked snapshot / restore is the sequence of per-field
stream-ordered copies the kernel replaces.  Timed, `reps` times each, the legs alternated, on a device-synchronised host clock:
  snapshot, restore           the kernel, every replica
  restore_half                the kernel, every second replica masked out
  memcpy                      ONE device-to-device copy of the blob's bytes: the floor
  copies_snapshot, copies_restore   the per-field sequence: the reference the single launch has to beat
`single_launch_not_slower` per shape: the kernel's median <= the sequence's median, for snapshot and for restore.

The bracket in training (the ring, `--fragment 100`): seconds per training iteration of train_on_device(device_adam) with
evaluation_interval=1, evaluation_steps=100 and without, each in a child process of this run (the median over the last `reps`
of reps + 3 iterations), one greedy 100-step fragment on its own, and -- with --parent_tree DIR, a checkout of the parent
commit with its library built -- the same iteration without evaluation on the parent's library.  `bracket_seconds` = the
iteration with evaluation - the iteration without - the fragment.  One JSON object on stdout (and in --out)."""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def seconds(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def spread(values):
    v = sorted(values)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def iteration_child(args):
    """--iteration: seconds per training iteration (and per greedy fragment) on the tree of --tree."""
    sys.path.insert(0, os.path.join(os.path.abspath(args.tree), "examples"))
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    import train_vec
    stamps = []

    def log(line):
        if line.startswith("iteration"):
            torch.cuda.synchronize()
            stamps.append(time.perf_counter())
    kw = dict(evaluation_interval=1, evaluation_steps=args.steps) if args.evaluation else {}
    train_vec.train_on_device(train_vec.ring_flow_params(500), replicas=args.replicas, fragment=args.steps,
                              iterations=args.reps + 3, epochs=4, log=log, device_update=True, device_adam=True, **kw)
    gaps = [b - a for a, b in zip(stamps[:-1], stamps[1:])][-args.reps:]
    print(json.dumps({"seconds_per_iteration": spread(gaps), "evaluation": bool(args.evaluation), "tree": args.tree}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent_tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--iteration", action="store_true", help="(child) time training iterations on --tree")
    ap.add_argument("--evaluation", action="store_true", help="(child) with evaluation_interval=1")
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    if args.iteration:
        return iteration_child(args)
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    sys.path.insert(0, ROOT)
    import torch
    import flow_amd
    from flow_amd.envs import VecFlowEnv
    from flow_amd.utils.device_policy import DevicePolicy
    from train_vec import GaussianPolicy
    flow_amd.install_as_flow()
    R = args.replicas
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    res = {"replicas": R, "reps": args.reps, "device": torch.cuda.get_device_name(0), "clock": "host, device-synchronised",
           "shapes": {}}
    legs, keep = [], []
    for shape in ("singleagent_ring", "singleagent_bottleneck"):
        fp = dict(importlib.import_module("exp_configs.rl.singleagent." + shape).flow_params)
        vec = VecFlowEnv(fp, num_replicas=R, device=0, seed=7)
        os.environ["FLOWSIM_SNAPSHOT_COPIES"] = "1"
        try:
            twin = VecFlowEnv(fp, num_replicas=R, device=0, seed=7)
        finally:
            del os.environ["FLOWSIM_SNAPSHOT_COPIES"]
        info = vec.sim.snapshot_info()
        entry = {"blob_bytes": int(info.bytes), "fields": int(info.num_fields), "vehicles": vec.sim.N, "obs_dim": vec.obs_dim}
        res["shapes"][shape] = entry
        half = torch.zeros(R, dtype=torch.uint8, device=dev)
        half[::2] = 1
        blobs = [torch.zeros(int(info.bytes), dtype=torch.uint8, device=dev) for _ in range(3)]
        for v in (vec, twin):
            v.reset()
            v.rollout(20)                                        # a state worth keeping
            v.sim.snapshot_dev(blobs[0] if v is vec else blobs[1])
            v.sim.restore_dev(blobs[0] if v is vec else blobs[1])
        torch.cuda.synchronize()
        sim, tsim = vec.sim, twin.sim
        for name, fn in (("snapshot", lambda s=sim, b=blobs[0]: s.snapshot_dev(b)),
                         ("restore", lambda s=sim, b=blobs[0]: s.restore_dev(b)),
                         ("restore_half", lambda s=sim, b=blobs[0], m=half: s.restore_dev(b, m)),
                         ("memcpy", lambda a=blobs[2], b=blobs[0]: a.copy_(b)),
                         ("copies_snapshot", lambda s=tsim, b=blobs[1]: s.snapshot_dev(b)),
                         ("copies_restore", lambda s=tsim, b=blobs[1]: s.restore_dev(b))):
            def timed(fn=fn, on=(vec if not name.startswith("copies") else twin)):
                on.use_current_stream()
                return seconds(torch, fn)
            timed()                                              # warm-up
            legs.append((shape, name, timed, []))
        keep.append((vec, twin, blobs, half))
    for _ in range(args.reps):                                   # alternately: drifts of the clock hit every leg alike
        for _, _, fn, ts in legs:
            ts.append(fn())
    for shape, name, _, ts in legs:
        res["shapes"][shape][name] = {"seconds": spread(ts)}
    for shape, entry in res["shapes"].items():
        med = lambda k: entry[k]["seconds"]["median"]            # noqa: E731
        entry["single_launch_not_slower"] = {"snapshot": med("snapshot") <= med("copies_snapshot"),
                                             "restore": med("restore") <= med("copies_restore")}
        entry["snapshot_over_memcpy_median"] = med("snapshot") / med("memcpy")
        entry["snapshot_over_copies_median"] = med("snapshot") / med("copies_snapshot")
        entry["restore_over_copies_median"] = med("restore") / med("copies_restore")
    # one greedy fragment on the ring, alone
    vec = keep[0][0]
    torch.manual_seed(0)
    pi = GaussianPolicy(vec.obs_dim, vec.act_dim).to(dev)
    pol = DevicePolicy([pi.mu[0], pi.mu[2]], pi.mu[4], log_std=pi.log_std, seed=0, greedy=True)
    vec.reset()
    out = vec.policy_rollout(pol, args.steps, reset_done=True)
    frag = [seconds(torch, lambda: vec.policy_rollout(pol, args.steps, reset_done=True, out=out)) for _ in range(args.reps)]
    for item in keep:
        item[0].close(), item[1].close()

    def child(tree, evaluation):
        cmd = [sys.executable, os.path.abspath(__file__), "--iteration", "--tree", tree, "--steps", str(args.steps), "--reps",
               str(args.reps), "--replicas", str(R)] + (["--evaluation"] if evaluation else [])
        run = subprocess.run(cmd, capture_output=True, text=True)
        if run.returncode != 0:
            raise SystemExit("bench_snapshot.py: the child on %s failed:\n%s" % (tree, run.stderr[-2000:]))
        return json.loads(run.stdout.strip().splitlines()[-1])
    plain, with_ev = child(ROOT, False), child(ROOT, True)
    it = {"steps": args.steps, "fragment_seconds": spread(frag), "without_evaluation": plain["seconds_per_iteration"],
          "with_evaluation": with_ev["seconds_per_iteration"]}
    it["bracket_seconds"] = (with_ev["seconds_per_iteration"]["median"] - plain["seconds_per_iteration"]["median"]
                             - it["fragment_seconds"]["median"])
    if args.parent_tree:
        parent = child(args.parent_tree, False)
        it["parent_without_evaluation"] = parent["seconds_per_iteration"]
        it["without_evaluation_over_parent_median"] = plain["seconds_per_iteration"]["median"] / parent["seconds_per_iteration"]["median"]
    res["training_iteration"] = it
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    import warnings
    warnings.simplefilter("ignore")
    main()
