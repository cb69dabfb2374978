"""The whole PPO update on the device (DeviceLearner.update) with the plain loss -- the clipped surrogate and (v - ret)^2:
k_ppo_grad -- against the same update with the reference's loss terms on -- KL penalty with its adaptive coefficient,
clipped value loss, entropy: k_ppo_eval with the old means, the full-loss form of k_ppo_grad, k_kl_adapt -- and against
torch's ppo_update with the same terms on:
python scripts/bench_ppo_loss.py [--replicas 1024] [--steps 100] [--epochs 4] [--reps 7] [--out profiles/ppo_loss_bench.json]

The protocol of scripts/bench_ppo_device_adam.py (profiles/ppo_device_adam_bench.json).  In ONE process, per shape (obs_dim,
act_dim) of singleagent_ring (3, 1), singleagent_merge (25, 5) and singleagent_bottleneck (141, 20): one fragment of `steps`
steps of `replicas` replicas -- random observations, actions sampled from the initial policy, random rewards, 1 % of the
episodes ending -- and copies of the same GaussianPolicy.  The three updates on that fragment are timed alternately, `reps`
times each after one warm-up call, host clock around a device synchronisation; median, min and max in milliseconds.
`terms_off` is the update of profiles/ppo_device_adam_bench.json's `device_adam` leg, launch for launch: the baseline.
Per shape: the full-loss median over the baseline's, the baseline's own min-max spread, and the share of bytes the terms
add per epoch, n (A + 1) floats next to n (D + A + 4).
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
LEGS = ("terms_off", "terms_on", "torch_terms_on")
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
    from train_vec import AdaptiveKL, GaussianPolicy, ppo_update, ring_flow_params
    flow_amd.install_as_flow()
    R, K = args.replicas, args.steps
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    res = {"replicas": R, "steps": K, "epochs": args.epochs, "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "terms": TERMS, "shapes": {}}
    vec = VecFlowEnv(ring_flow_params(500), num_replicas=2, device=0)        # lends its stream to the learners

    def learner_of(pi):
        return DeviceLearner(vec, [pi.mu[0], pi.mu[2]], pi.mu[4], pi.log_std, [pi.value[0], pi.value[2]], pi.value[4])

    legs = []
    for name, D, A in SHAPES:
        torch.manual_seed(0)
        pis = [GaussianPolicy(D, A).to(dev) for _ in range(3)]
        for p in pis[1:]:
            p.load_state_dict(pis[0].state_dict())
        obs = torch.randn(K + 1, R, D, device=dev)
        act = pis[0].act(obs[:K].reshape(K * R, D)).view(K, R, A)
        shard = (obs, act, torch.randn(K, R, device=dev), (torch.rand(K, R, device=dev) < 0.01).to(torch.uint8))
        off, on = learner_of(pis[0]), learner_of(pis[1])
        off.adopt_parameters()
        on.adopt_parameters()
        opt, kl = torch.optim.Adam(pis[2].parameters(), lr=3e-4), AdaptiveKL(TERMS["kl_target"], 0.2)
        runs = {"terms_off": lambda s=shard, l=off: l.update([s], epochs=args.epochs),
                "terms_on": lambda s=shard, l=on: l.update([s], epochs=args.epochs, **TERMS),
                "torch_terms_on": lambda p=pis[2], o=opt, s=shard, k=kl: ppo_update(
                    p, o, [s], epochs=args.epochs, kl=k, entropy_coef=TERMS["entropy_coef"], vf_clip=TERMS["vf_clip"])}
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
        base = m["terms_off"]
        res["shapes"][name] = {"obs_dim": D, "act_dim": A, "samples": K * R, "terms_off_ms": base, "terms_on_ms": m["terms_on"],
                               "torch_terms_on_ms": m["torch_terms_on"],
                               "terms_on_over_terms_off_median": m["terms_on"]["median"] / base["median"],
                               "terms_off_spread": (base["max"] - base["min"]) / base["median"],
                               "added_bytes_share": (A + 1.0) / (D + A + 4.0),
                               "torch_over_terms_on_median": m["torch_terms_on"]["median"] / m["terms_on"]["median"]}
    vec.close()
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    import warnings
    warnings.simplefilter("ignore")
    main()
