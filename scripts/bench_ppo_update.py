"""The PPO update of examples/train_vec.py, torch against the device path (DeviceLearner: k_ppo_eval, k_gae, k_ppo_grad):
python scripts/bench_ppo_update.py [--replicas 1024] [--steps 100] [--epochs 4] [--reps 7] [--out profiles/ppo_update_bench.json]

In ONE process, per shape (obs_dim, act_dim) of singleagent_ring (3, 1), singleagent_merge (25, 5) and
singleagent_bottleneck (141, 20): one fragment of `steps` steps of `replicas` replicas -- random observations, actions
sampled from the initial policy, random rewards, 1 % of the episodes ending: the update's cost does not depend on the
values -- and two copies of the same GaussianPolicy with an Adam optimiser each.  ppo_update(..., learner=None) and
ppo_update(..., learner=DeviceLearner) on that fragment are timed alternately, `reps` times each after one warm-up call,
host clock around a device synchronisation (the update has host work of its own: the Python loop of gae(), the
statistics' read-backs); median, min and max in milliseconds.  `device_max_below_torch_min` is the bar: the device path's
slowest update against torch's fastest.
Then one whole training iteration of the ring (train_on_device: rollout, update, bookkeeping) with and without
device_update: `reps` iterations after the first of one run each (two handles cannot share the loop), the same figures.
One JSON object on stdout (and in --out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

import torch

SHAPES = [("singleagent_ring", 3, 1), ("singleagent_merge", 25, 5), ("singleagent_bottleneck", 141, 20)]


def millis(ts):
    r = sorted(1e3 * t for t in ts)
    return {"median": r[len(r) // 2], "min": r[0], "max": r[-1]}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import flow_amd
    from flow_amd.envs import VecFlowEnv
    from flow_amd.utils.device_ppo import DeviceLearner
    from train_vec import GaussianPolicy, ppo_update, ring_flow_params, train_on_device
    flow_amd.install_as_flow()
    R, K = args.replicas, args.steps
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    res = {"replicas": R, "steps": K, "epochs": args.epochs, "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "shapes": {}}
    vec = VecFlowEnv(ring_flow_params(500), num_replicas=2, device=0)        # lends its stream to the learners
    legs = []
    for name, D, A in SHAPES:
        torch.manual_seed(0)
        pis = [GaussianPolicy(D, A).to(dev) for _ in range(2)]
        pis[1].load_state_dict(pis[0].state_dict())
        opts = [torch.optim.Adam(p.parameters(), lr=3e-4) for p in pis]
        obs = torch.randn(K + 1, R, D, device=dev)
        act = pis[0].act(obs[:K].reshape(K * R, D)).view(K, R, A)
        shard = (obs, act, torch.randn(K, R, device=dev), (torch.rand(K, R, device=dev) < 0.01).to(torch.uint8))
        pi = pis[1]
        learner = DeviceLearner(vec, [pi.mu[0], pi.mu[2]], pi.mu[4], pi.log_std, [pi.value[0], pi.value[2]], pi.value[4])
        runs = {"torch": lambda p=pis[0], o=opts[0], s=shard: ppo_update(p, o, [s], epochs=args.epochs),
                "device": lambda p=pis[1], o=opts[1], s=shard, l=learner: ppo_update(p, o, [s], epochs=args.epochs, learner=l)}
        for fn in runs.values():
            wall(fn)                                                         # warm-up
        legs.append((name, D, A, runs, {"torch": [], "device": []}))
    for _ in range(args.reps):                                               # alternately: drifts of the clock hit both alike
        for _, _, _, runs, ts in legs:
            for k, fn in runs.items():
                ts[k].append(wall(fn))
    for name, D, A, _, ts in legs:
        t, d = millis(ts["torch"]), millis(ts["device"])
        res["shapes"][name] = {"obs_dim": D, "act_dim": A, "samples": K * R, "torch_ms": t, "device_ms": d,
                               "torch_over_device_median": t["median"] / d["median"],
                               "device_max_below_torch_min": d["max"] < t["min"]}
    vec.close()
    # one whole training iteration of the ring, rollout and update
    res["train_iteration_ring"] = {}
    for key, flag in (("torch_update", False), ("device_update", True)):
        stamps = []

        def log(msg, stamps=stamps):
            if msg.startswith("iteration"):
                torch.cuda.synchronize()
                stamps.append(time.perf_counter())
        train_on_device(ring_flow_params(500), replicas=R, fragment=K, iterations=args.reps + 2, epochs=args.epochs,
                        device_update=flag, log=log)
        res["train_iteration_ring"][key + "_ms"] = millis([b - a for a, b in zip(stamps[1:-1], stamps[2:])])
    it = res["train_iteration_ring"]
    it["torch_over_device_median"] = it["torch_update_ms"]["median"] / it["device_update_ms"]["median"]
    it["device_max_below_torch_min"] = it["device_update_ms"]["max"] < it["torch_update_ms"]["min"]
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    import warnings
    warnings.simplefilter("ignore")
    main()
