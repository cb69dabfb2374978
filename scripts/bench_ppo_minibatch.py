"""Minibatch SGD in the device PPO update: one epoch of minibatch steps of B samples as (a) ONE launch per step -- the
minibatch form of k_ppo_grad with the reduction, the division and Adam in its tail (FS_MB_STEP) --, (b) the chain of two
launches per step -- the same kernel reducing only (FS_MB_PARTIAL), then k_mb_finish -- and (c) torch's
ppo_update(minibatch=B):
python scripts/bench_ppo_minibatch.py [--replicas 1024] [--steps 100] [--reps 7] [--out profiles/ppo_minibatch_bench.json]

The protocol of scripts/bench_ppo_loss.py.  In ONE process, per shape (obs_dim, act_dim) of singleagent_ring (3, 1),
singleagent_merge (25, 5) and singleagent_bottleneck (141, 20) and per B in 128, 1024, 4096: one fragment of `steps` steps of
`replicas` replicas and copies of the same GaussianPolicy; every leg is one update of ONE epoch with the reference's loss
terms on, timed alternately, `reps` times each after one warm-up call, host clock around a device synchronisation; median,
min and max in milliseconds.  The legs: the three paths called eagerly, the two device paths replayed from a captured
graph (what a training loop that captures its update pays: no Python between the launches), and per shape the update with
NO epoch (`prelude`: eval, gae, statistics; the one-thread k_kl_adapt that ends an update with epochs stays in the epoch's
time), eager for the device and for torch, whose median is taken off an epoch's.
Per point: milliseconds per epoch and microseconds per minibatch step for each path, and chain over fused.
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
BATCHES = (128, 1024, 4096)
TERMS = dict(kl_target=0.02, entropy_coef=0.01, vf_clip=10.0)


def millis(ts):
    r = sorted(1e3 * t for t in ts)
    return {"median": r[len(r) // 2], "min": r[0], "max": r[-1]}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def captured(fn):
    """``fn`` captured into a graph after one eager call on the capture stream; returns the replay."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
        side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        fn()
    torch.cuda.synchronize()
    return graph.replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default=None, help="comma-separated names among %s (default: all)" % ", ".join(s[0] for s in SHAPES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    shapes = [s for s in SHAPES if args.shapes is None or s[0] in args.shapes.split(",")]
    import flow_amd
    from flow_amd.envs import VecFlowEnv
    from flow_amd.utils.device_ppo import DeviceLearner
    from train_vec import AdaptiveKL, GaussianPolicy, ppo_update, ring_flow_params
    flow_amd.install_as_flow()
    R, K = args.replicas, args.steps
    n = R * K
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    res = {"replicas": R, "steps": K, "samples": n, "epochs": 1, "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "terms": TERMS, "shapes": {}}
    vec = VecFlowEnv(ring_flow_params(500), num_replicas=2, device=0)        # lends its stream to the learners

    def learner_of(pi):
        learner = DeviceLearner(vec, [pi.mu[0], pi.mu[2]], pi.mu[4], pi.log_std, [pi.value[0], pi.value[2]], pi.value[4])
        learner.adopt_parameters()
        return learner

    legs = []                                                                # (shape, B or None, leg, fn, times)
    for name, D, A in shapes:
        torch.manual_seed(0)
        pis = [GaussianPolicy(D, A).to(dev) for _ in range(3)]
        for p in pis[1:]:
            p.load_state_dict(pis[0].state_dict())
        obs = torch.randn(K + 1, R, D, device=dev)
        act = pis[0].act(obs[:K].reshape(K * R, D)).view(K, R, A)
        shard = (obs, act, torch.randn(K, R, device=dev), (torch.rand(K, R, device=dev) < 0.01).to(torch.uint8))
        fused, chain = learner_of(pis[0]), learner_of(pis[1])
        opt, kl = torch.optim.Adam(pis[2].parameters(), lr=3e-4), AdaptiveKL(TERMS["kl_target"], 0.2)

        def device_leg(learner, B, one_launch, epochs=1, s=shard):
            return lambda: learner.update([s], epochs=epochs, minibatch=B, fused=one_launch, **TERMS)

        def torch_leg(B, epochs=1, p=pis[2], o=opt, s=shard, k=kl):
            return lambda: ppo_update(p, o, [s], epochs=epochs, kl=k, entropy_coef=TERMS["entropy_coef"],
                                      vf_clip=TERMS["vf_clip"], minibatch=B)
        legs.append((name, None, "prelude", device_leg(fused, 128, True, epochs=0), []))
        legs.append((name, None, "torch_prelude", torch_leg(128, epochs=0), []))
        for B in BATCHES:
            legs.append((name, B, "fused", device_leg(fused, B, True), []))
            legs.append((name, B, "chain", device_leg(chain, B, False), []))
            legs.append((name, B, "torch", torch_leg(B), []))
            legs.append((name, B, "fused_graph", captured(device_leg(fused, B, True)), []))
            legs.append((name, B, "chain_graph", captured(device_leg(chain, B, False)), []))
        legs.append((name, None, "prelude_graph", captured(device_leg(fused, 128, True, epochs=0)), []))
    for leg in legs:
        wall(leg[3])                                                         # warm-up
        print("warm-up %s B=%s %s" % leg[:3], file=sys.stderr, flush=True)
    for rep in range(args.reps):                                             # alternately: drifts of the clock hit all alike
        for leg in legs:
            leg[4].append(wall(leg[3]))
        print("repetition %d" % rep, file=sys.stderr, flush=True)
    for name, D, A in shapes:
        mine = {(B, leg): millis(ts) for nm, B, leg, _, ts in legs if nm == name}
        out = {"obs_dim": D, "act_dim": A, "prelude_ms": mine[(None, "prelude")], "prelude_graph_ms": mine[(None, "prelude_graph")],
               "torch_prelude_ms": mine[(None, "torch_prelude")], "batches": {}}
        for B in BATCHES:
            steps = -(-n // B)
            point = {"steps_per_epoch": steps}
            for leg, pre in (("fused", "prelude"), ("chain", "prelude"), ("torch", "torch_prelude"),
                             ("fused_graph", "prelude_graph"), ("chain_graph", "prelude_graph")):
                m = mine[(B, leg)]
                epoch = m["median"] - mine[(None, pre)]["median"]
                point[leg] = {"update_ms": m, "epoch_ms": epoch, "step_us": 1e3 * epoch / steps,
                              "step_us_min_max": [1e3 * (m["min"] - mine[(None, pre)]["median"]) / steps,
                                                  1e3 * (m["max"] - mine[(None, pre)]["median"]) / steps]}
            point["chain_over_fused_eager"] = point["chain"]["epoch_ms"] / point["fused"]["epoch_ms"]
            point["chain_over_fused_graph"] = point["chain_graph"]["epoch_ms"] / point["fused_graph"]["epoch_ms"]
            point["torch_over_fused_eager"] = point["torch"]["epoch_ms"] / point["fused"]["epoch_ms"]
            out["batches"][str(B)] = point
        res["shapes"][name] = out
    vec.close()
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    import warnings
    warnings.simplefilter("ignore")
    main()
