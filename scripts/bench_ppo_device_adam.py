"""The PPO update of examples/train_vec.py, the device update with torch's statistics and Adam (--device_update:
ppo_update(..., learner=DeviceLearner)) against the whole update on the device (--device_adam: DeviceLearner.update --
k_adv_stats, k_adv_finish, k_ppo_grad with n on the device, k_adam, parameters adopted into the packed weights):
python scripts/bench_ppo_device_adam.py [--replicas 1024] [--steps 100] [--epochs 4] [--reps 7] [--out profiles/ppo_device_adam_bench.json]

The protocol of scripts/bench_ppo_update.py (profiles/ppo_update_bench.json).  In ONE process, per shape (obs_dim, act_dim)
of singleagent_ring (3, 1), singleagent_merge (25, 5) and singleagent_bottleneck (141, 20): one fragment of `steps` steps
of `replicas` replicas -- random observations, actions sampled from the initial policy, random rewards, 1 % of the episodes
ending -- and copies of the same GaussianPolicy.  The two updates on that fragment are timed alternately, `reps` times each
after one warm-up call, host clock around a device synchronisation; median, min and max in milliseconds.  A third leg
replays DeviceLearner.update captured into a HIP graph (one graph launch per update).  `ranges_apart`: the new path's
slowest update against the device update's fastest.
Then one whole training iteration of the ring (train_on_device: rollout, update, bookkeeping) with --device_update and with
--device_adam: `reps` iterations after the first of one run each, the same figures.
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
LEGS = ("device_update", "device_adam", "device_adam_graph")


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

    def learner_of(pi):
        return DeviceLearner(vec, [pi.mu[0], pi.mu[2]], pi.mu[4], pi.log_std, [pi.value[0], pi.value[2]], pi.value[4])

    legs, side = [], torch.cuda.Stream(dev)
    for name, D, A in SHAPES:
        torch.manual_seed(0)
        pis = [GaussianPolicy(D, A).to(dev) for _ in range(3)]
        for p in pis[1:]:
            p.load_state_dict(pis[0].state_dict())
        obs = torch.randn(K + 1, R, D, device=dev)
        act = pis[0].act(obs[:K].reshape(K * R, D)).view(K, R, A)
        shard = (obs, act, torch.randn(K, R, device=dev), (torch.rand(K, R, device=dev) < 0.01).to(torch.uint8))
        opt = torch.optim.Adam(pis[0].parameters(), lr=3e-4)
        parent, whole, captured = (learner_of(p) for p in pis)
        whole.adopt_parameters()
        captured.adopt_parameters()
        # the graph leg first: its warm-up call binds the handle to the capture stream (fs_set_stream synchronises)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            captured.update([shard], epochs=args.epochs)
            side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            captured.update([shard], epochs=args.epochs)
        torch.cuda.synchronize()
        runs = {"device_update": lambda p=pis[0], o=opt, s=shard, l=parent: ppo_update(p, o, [s], epochs=args.epochs, learner=l),
                "device_adam": lambda s=shard, l=whole: l.update([s], epochs=args.epochs),
                "device_adam_graph": graph.replay}
        legs.append((name, D, A, runs, {k: [] for k in LEGS}))
    for _, _, _, runs, _ in legs:
        for fn in runs.values():
            wall(fn)                                                         # warm-up
    for _ in range(args.reps):                                               # alternately: drifts of the clock hit all alike
        for _, _, _, runs, ts in legs:
            for k, fn in runs.items():
                ts[k].append(wall(fn))
    for name, D, A, _, ts in legs:
        m = {k: millis(ts[k]) for k in LEGS}
        res["shapes"][name] = {"obs_dim": D, "act_dim": A, "samples": K * R, "device_update_ms": m["device_update"],
                               "device_adam_ms": m["device_adam"], "device_adam_graph_ms": m["device_adam_graph"],
                               "device_update_over_device_adam_median": m["device_update"]["median"] / m["device_adam"]["median"],
                               "ranges_apart": m["device_adam"]["max"] < m["device_update"]["min"],
                               "graph_ranges_apart": m["device_adam_graph"]["max"] < m["device_update"]["min"]}
    vec.close()
    # one whole training iteration of the ring, rollout and update
    res["train_iteration_ring"] = {}
    for key, flag in (("device_update", False), ("device_adam", True)):
        stamps = []

        def log(msg, stamps=stamps):
            if msg.startswith("iteration"):
                torch.cuda.synchronize()
                stamps.append(time.perf_counter())
        train_on_device(ring_flow_params(500), replicas=R, fragment=K, iterations=args.reps + 2, epochs=args.epochs,
                        device_update=True, device_adam=flag, log=log)
        res["train_iteration_ring"][key + "_ms"] = millis([b - a for a, b in zip(stamps[1:-1], stamps[2:])])
    it = res["train_iteration_ring"]
    it["device_update_over_device_adam_median"] = it["device_update_ms"]["median"] / it["device_adam_ms"]["median"]
    it["ranges_apart"] = it["device_adam_ms"]["max"] < it["device_update_ms"]["min"]
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    import warnings
    warnings.simplefilter("ignore")
    main()
