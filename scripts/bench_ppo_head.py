"""The whole PPO update on the device (DeviceLearner.update) with the reference's loss terms on, for the two forms of the
policy head: the free log_std (k_ppo_eval, k_ppo_grad_loss, k_ppo_minibatch) against the head of 2 act_dim outputs whose
log stds come from the network (DeviceLearner(net_log_std=True): k_ppo_eval_ls, k_ppo_grad_loss_ls, k_ppo_minibatch_ls):
python scripts/bench_ppo_head.py [--replicas 1024] [--steps 100] [--epochs 4] [--reps 7] [--out profiles/ppo_head_bench.json]

The protocol of scripts/bench_ppo_loss.py.  In ONE process, per shape (obs_dim, act_dim) of singleagent_ring (3, 1),
singleagent_merge (25, 5) and singleagent_bottleneck (141, 20): one fragment of `steps` steps of `replicas` replicas --
random observations, actions sampled from the initial free-head policy, random rewards, 1 % of the episodes ending -- and
two policies with the same trunk, mean rows and value network; the network head starts as GaussianPolicy(net_log_std=True)
does (zero log-std weights, bias -0.5), so both forms see the same distribution at the start.  Per shape two pairs of legs,
the whole batch per step (`full`) and shuffled minibatches of 128 on the chain PARTIAL + mb_finish (`mb128`, one epoch);
all legs are timed alternately, `reps` times each after one warm-up call, host clock around a device synchronisation;
median, min and max in milliseconds.
Per pair: the network head's median over the free head's, the free head's own min-max spread, and what the new form adds by
count: one 32-input layer forward and one 32-unit block backward per tile next to the 2 (ceil(D / 32) + L) layer blocks both
networks have in each direction, A more floats per row of the old distribution, 1056 floats of LDS.
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
TERMS = dict(kl_target=0.02, entropy_coef=0.01, vf_clip=10.0)
LAYERS, BATCH = 2, 128


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
    from train_vec import GaussianPolicy, ring_flow_params
    flow_amd.install_as_flow()
    R, K = args.replicas, args.steps
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    res = {"replicas": R, "steps": K, "epochs": args.epochs, "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "terms": TERMS, "minibatch": BATCH, "shapes": {}}
    vec = VecFlowEnv(ring_flow_params(500), num_replicas=2, device=0)        # lends its stream to the learners

    def learner_of(pi):
        ls = None if pi.net_log_std else pi.log_std
        lr = DeviceLearner(vec, [pi.mu[0], pi.mu[2]], pi.mu[4], ls, [pi.value[0], pi.value[2]], pi.value[4],
                           net_log_std=pi.net_log_std)
        lr.adopt_parameters()
        return lr

    legs = []
    for name, D, A in SHAPES:
        torch.manual_seed(0)
        free = GaussianPolicy(D, A).to(dev)
        obs = torch.randn(K + 1, R, D, device=dev)
        act = free.act(obs[:K].reshape(K * R, D)).view(K, R, A)
        shard = (obs, act, torch.randn(K, R, device=dev), (torch.rand(K, R, device=dev) < 0.01).to(torch.uint8))
        runs = {}
        for mode in ("full", "mb128"):
            for head in ("free", "net"):
                pi = GaussianPolicy(D, A, net_log_std=head == "net").to(dev)
                with torch.no_grad():
                    for i in (0, 2):
                        pi.mu[i].load_state_dict(free.mu[i].state_dict())
                    pi.mu[4].weight[:A].copy_(free.mu[4].weight)
                    pi.mu[4].bias[:A].copy_(free.mu[4].bias)
                    pi.value.load_state_dict(free.value.state_dict())
                kw = dict(epochs=args.epochs, **TERMS) if mode == "full" else dict(epochs=1, minibatch=BATCH, **TERMS)
                runs[mode + "_" + head] = lambda s=shard, l=learner_of(pi), kw=kw: l.update([s], **kw)
        legs.append((name, D, A, runs, {k: [] for k in runs}))
    for _, _, _, runs, _ in legs:
        for fn in runs.values():
            wall(fn)                                                         # warm-up
    for _ in range(args.reps):                                               # alternately: drifts of the clock hit all alike
        for _, _, _, runs, ts in legs:
            for k, fn in runs.items():
                ts[k].append(wall(fn))
    for name, D, A, _, ts in legs:
        m = {k: millis(v) for k, v in ts.items()}
        blocks = 2 * (-(-D // 32) + LAYERS)
        out = {"obs_dim": D, "act_dim": A, "samples": K * R, "added_layer_blocks_share": 1.0 / blocks,
               "added_bytes_share": float(A) / (D + 2 * A + 5.0), "added_lds_floats": 1056}
        for mode in ("full", "mb128"):
            base, net = m[mode + "_free"], m[mode + "_net"]
            out[mode] = {"free_ms": base, "net_ms": net, "net_over_free_median": net["median"] / base["median"],
                         "free_spread": (base["max"] - base["min"]) / base["median"]}
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
