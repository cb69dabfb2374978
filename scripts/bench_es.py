"""What a policy population costs the single-policy rollout, what it costs itself, and what one ES generation costs:
python scripts/bench_es.py [--replicas 1024 4096] [--steps 100] [--reps 7] [--parent_tree DIR] [--out profiles/es_bench.json]

At singleagent_ring's shipped parameters, per replica count, fragments of `steps` steps with resets inside, a
device-synchronised host clock around each call, one warm-up call per form, then `reps` calls per form, the forms
alternated; median, min and max.
  (a) policy      fs_policy_rollout_dev (k_ring_policy), sampling, on this library;
  (b) parent      the same fragment on the parent commit's library (--parent_tree DIR: a checkout of the parent with its
                  library built), in a child process of the same run (--only_policy --tree DIR), next to a child of the
                  same shape on THIS tree (`policy_child`); `ranges_overlap_parent` compares those two: the project's
                  condition is that the ranges overlap at every size.  The pair of children runs a second time in the
                  other order (`parent_first`), recorded next to the condition;
  (c) population  fs_population_rollout_dev with R / 16 distinct weight sets (k_ring_policy<Population>), as a ratio to (a);
  (d) generation  one DeviceES generation (R / 16 members, no evaluation members: perturb, reset, horizon / steps
                  population fragments with the mean action, fitness after each, weights, gradient, Adam), as a whole and
                  launch by launch (each timed on its own, so the parts add up to more than the whole), next to one PPO
                  iteration on the same handle: one sampled fragment and DeviceLearner.update (--device_adam's update, 4
                  epochs).
One JSON object on stdout (and in --out)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent_tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--only_policy", action="store_true", help="time form (a) alone (the child of --parent_tree)")
    ap.add_argument("--tree", default=ROOT, help="import flow_amd from this tree (with --only_policy)")
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, os.path.join(tree, "examples"))
    sys.path.insert(0, tree)
    import torch
    import flow_amd
    from flow_amd.envs import VecFlowEnv
    from flow_amd.utils.device_policy import DevicePolicy
    from train_vec import GaussianPolicy
    flow_amd.install_as_flow()
    params = importlib.import_module("exp_configs.rl.singleagent.singleagent_ring").flow_params
    K = args.steps
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    res = {"steps": K, "reps": args.reps, "device": torch.cuda.get_device_name(0), "clock": "host, device-synchronised",
           "experiment": "singleagent_ring", "replicas": {}}
    legs, keep = [], []                                      # (R, form, timed call, times, env steps per call or None)

    def policy_of(vec, seed=0):
        torch.manual_seed(seed)
        pi = GaussianPolicy(vec.obs_dim, vec.act_dim).to(dev)
        return pi, DevicePolicy([pi.mu[0], pi.mu[2]], pi.mu[4], log_std=pi.log_std, seed=0)

    for R in args.replicas:
        entry = {"kernels": {}}
        res["replicas"][str(R)] = entry
        # (a) the single-policy fragment
        vec = VecFlowEnv(params, num_replicas=R, device=0)
        pi, pol = policy_of(vec)
        vec.reset()
        out = vec.policy_rollout(pol, K, reset_done=True)
        torch.cuda.synchronize()
        entry["kernels"]["policy"] = vec.sim.last_kernel
        legs.append((R, "policy", lambda v=vec, p=pol, o=out: seconds(torch, lambda: v.policy_rollout(p, K, reset_done=True, out=o)), [], K * R))
        keep.append((vec, pi, pol, out))
        if args.only_policy:
            continue
        # (c) the population fragment: R / 16 distinct weight sets
        vec = VecFlowEnv(params, num_replicas=R, device=0)
        pi, pol = policy_of(vec)
        M, P = R // 16, pol.buf.numel()
        w = pol.buf.repeat(M, 1) + 0.02 * torch.randn((M, P), device=dev)
        pop = pol.population(w.contiguous(), M, 16)
        vec.reset()
        out = vec.population_rollout(pop, K, reset_done=True)
        torch.cuda.synchronize()
        entry["kernels"]["population"] = vec.sim.last_kernel
        entry["members"] = M
        legs.append((R, "population", lambda v=vec, p=pop, o=out: seconds(torch, lambda: v.population_rollout(p, K, reset_done=True, out=o)), [], K * R))
        keep.append((vec, pi, pol, out, w, pop))
        # (d) one ES generation and its launches, next to one PPO iteration with the update on the device, on one handle
        from flow_amd.utils.device_es import DeviceES
        from flow_amd.utils.device_ppo import DeviceLearner
        vec = VecFlowEnv(params, num_replicas=R, device=0)
        pi, pol = policy_of(vec)
        es = DeviceES(vec, pol, pairs=M // 2, eval_members=0, sigma=0.02, mode="es", lr=0.02, l2=0.005, noise_seed=1)
        horizon = int(params["env"].horizon)
        es.generation(horizon, K)                              # warm-up: the buffers and the library's scratch
        torch.cuda.synchronize()
        entry["kernels"]["generation_rollout"] = es.rollout_kernel
        entry["generation_shape"] = dict(pairs=es.N, members=es.M, group=es.group, params=es.P, horizon=horizon,
                                         fragments=-(-horizon // K))
        frag = es._outs[K]
        legs.append((R, "generation", lambda e=es: seconds(torch, lambda: e.generation(horizon, K)), [], horizon * R))
        legs.append((R, "es_perturb", lambda e=es: seconds(torch, e.perturb), [], None))
        legs.append((R, "es_reset", lambda v=vec: seconds(torch, v.reset), [], None))
        legs.append((R, "es_fitness", lambda e=es, o=frag: seconds(torch, lambda: e.fitness(o[3], o[4], accumulate=True)), [], None))
        legs.append((R, "es_weights", lambda e=es: seconds(torch, e.direction_weights), [], None))
        legs.append((R, "es_gradient", lambda e=es: seconds(torch, e.gradient), [], None))
        legs.append((R, "es_adam", lambda e=es: seconds(torch, e.adam), [], None))
        keep.append((vec, pi, pol, es))
        vec = VecFlowEnv(params, num_replicas=R, device=0)
        torch.manual_seed(0)
        pi = GaussianPolicy(vec.obs_dim, vec.act_dim).to(dev)
        learner = DeviceLearner(vec, [pi.mu[0], pi.mu[2]], pi.mu[4], pi.log_std, [pi.value[0], pi.value[2]], pi.value[4])
        learner.adopt_parameters()
        pol = DevicePolicy([pi.mu[0], pi.mu[2]], pi.mu[4], log_std=pi.log_std, seed=0).share(learner)
        vec.reset()
        out = vec.policy_rollout(pol, K, reset_done=True)

        def ppo_iteration(v=vec, p=pol, o=out, l=learner):
            obs, act, _, rew, done = v.policy_rollout(p, K, reset_done=True, out=o)
            l.update([(obs, act, rew, done)], epochs=4, lr=3e-4)
        ppo_iteration()
        torch.cuda.synchronize()
        legs.append((R, "ppo_iteration", lambda f=ppo_iteration: seconds(torch, f), [], K * R))
        keep.append((vec, pi, pol, learner, out))
    for _ in range(args.reps):                               # alternately: drifts of the clock hit every form alike
        for _, _, fn, ts, _ in legs:
            ts.append(fn())
    for R, form, _, ts, work in legs:
        e = res["replicas"][str(R)]
        e[form] = {"seconds_per_call": spread(ts)}
        if work is not None:
            e[form]["env_steps_per_s"] = spread([work / t for t in ts])
    for item in keep:
        item[0].close()
    if not args.only_policy:
        for R, e in res["replicas"].items():
            e["population_over_policy_median"] = e["population"]["env_steps_per_s"]["median"] / e["policy"]["env_steps_per_s"]["median"]
            e["generation_over_ppo_iteration_seconds"] = (e["generation"]["seconds_per_call"]["median"] /
                                                          e["ppo_iteration"]["seconds_per_call"]["median"])

        def child(tree):
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "--only_policy", "--tree", tree, "--steps", str(K),
                                  "--reps", str(args.reps), "--replicas"] + [str(r) for r in args.replicas],
                                 capture_output=True, text=True)
            if run.returncode != 0:
                raise SystemExit("bench_es.py --parent_tree: the child on %s failed:\n%s" % (tree, run.stderr[-2000:]))
            return json.loads(run.stdout.strip().splitlines()[-1])
        if args.parent_tree:
            here, parent = child(ROOT), child(args.parent_tree)
            parent2, here2 = child(args.parent_tree), child(ROOT)
            overlap = lambda s, p: s["max"] >= p["min"] and p["max"] >= s["min"]      # noqa: E731
            for R, e in res["replicas"].items():
                s, p = here["replicas"][R]["policy"]["env_steps_per_s"], parent["replicas"][R]["policy"]["env_steps_per_s"]
                s2, p2 = here2["replicas"][R]["policy"]["env_steps_per_s"], parent2["replicas"][R]["policy"]["env_steps_per_s"]
                e["policy"].update(policy_child={"env_steps_per_s": s, "kernel": here["replicas"][R]["kernels"]["policy"]},
                                   parent={"env_steps_per_s": p, "kernel": parent["replicas"][R]["kernels"]["policy"]},
                                   over_parent_median=s["median"] / p["median"], ranges_overlap_parent=overlap(s, p),
                                   parent_first={"policy_child": s2, "parent": p2, "over_parent_median": s2["median"] / p2["median"],
                                                 "ranges_overlap_parent": overlap(s2, p2)})
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    import warnings
    warnings.simplefilter("ignore")
    main()
