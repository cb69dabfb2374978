"""Closed-loop env-steps/s of the reference's multi-agent experiments with one policy shared by the agents:
python scripts/bench_ma_policy.py [--replicas 4096] [--steps 500] [--reps 3] [--merge-replicas 1024] [--merge-steps 600]

Per experiment (multiagent_ring: MultiAgentWaveAttenuationPOEnv; multiagent_figure_eight: MultiAgentAccelPOEnv;
multiagent_merge: MultiAgentMergePOEnv with its actions applied), two numbers from the same process: the fused policy +
step kernel (VecFlowEnv.policy_rollout, one launch per fragment) and K single steps around the torch policy captured as
one HIP graph (VecFlowEnv.capture).  The merge leg (BASELINE's C5 share of one GPU, one 600-step episode) also reports
sub-steps/s and the open-loop k_merge_queue rate of the same handle.  One JSON object on stdout."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

import torch


def timed(fn, reps):
    """Median seconds of fn() over `reps` runs after one untimed run (one event pair around each run)."""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return sorted(ts)[len(ts) // 2]


def leg(name, R, K, reps):
    import importlib
    import flow_amd
    from flow_amd.envs import VecFlowEnv
    from flow_amd.utils.device_policy import DevicePolicy
    from train_vec import GaussianPolicy
    flow_amd.install_as_flow()
    fp = importlib.import_module("exp_configs.rl.multiagent." + name).flow_params
    if name == "multiagent_merge":                     # the shipped env applies no action: the actions-applied subclass
        from flow_amd.envs.multiagent.merge import MultiAgentMergePOEnv

        class MultiAgentMergeAppliedPOEnv(MultiAgentMergePOEnv):
            APPLY_ENUMERATE_QUIRK = False
        fp = dict(fp, env_name=MultiAgentMergeAppliedPOEnv)
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    vec = VecFlowEnv(fp, num_replicas=R, device=0)
    n_ag = vec.act_dim
    k = vec.obs_dim // n_ag
    pi = GaussianPolicy(k, 1).to(dev)
    out = {"replicas": R, "steps": K, "agents": n_ag}
    # fused: one launch per fragment
    fused = DevicePolicy([pi.mu[0], pi.mu[2]], pi.mu[4], log_std=pi.log_std, seed=0)
    vec.reset()
    bufs = vec.policy_rollout(fused, K, reset_done=True)
    torch.cuda.synchronize()
    out["fused_kernel"] = vec.sim.last_kernel
    t = timed(lambda: vec.policy_rollout(fused, K, reset_done=True, out=bufs), reps)
    out["fused_env_steps_per_s"] = K * R / t
    # the HIP graph of K single steps around the torch policy
    def act_shared(obs):
        return pi.act(obs.view(R * n_ag, k)).view(R, n_ag)
    graph = vec.capture(K, policy=act_shared, reset_done=True)
    graph.begin(vec.reset())
    t = timed(graph.replay, reps)
    out["graph_env_steps_per_s"] = K * R / t
    out["fused_over_graph"] = out["fused_env_steps_per_s"] / out["graph_env_steps_per_s"]
    if name == "multiagent_merge":
        sps = vec.sim.spec.get("sims_per_step", 1)
        out["sims_per_step"] = sps
        out["fused_substeps_per_s"] = out["fused_env_steps_per_s"] * sps
        out["graph_substeps_per_s"] = out["graph_env_steps_per_s"] * sps
        # the open-loop kernel of the same handle (no actions: every vehicle on its car-following model)
        ob, rw, dn = (torch.empty((K, R, vec.obs_dim), device=dev), torch.empty((K, R), device=dev),
                      torch.empty((K, R), dtype=torch.uint8, device=dev))

        def open_loop():
            vec.sim.rollout_dev(K, ob, rw, dn)
        vec.sim.reset()
        open_loop()
        torch.cuda.synchronize()
        out["open_loop_kernel"] = vec.sim.last_kernel
        t = timed(open_loop, reps)
        out["open_loop_substeps_per_s"] = K * R * sps / t
    vec.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--merge-replicas", type=int, default=1024)
    ap.add_argument("--merge-steps", type=int, default=600)
    ap.add_argument("--legs", default="multiagent_ring,multiagent_figure_eight,multiagent_merge")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    res = {}
    for name in args.legs.split(","):
        merge = name == "multiagent_merge"
        res[name] = leg(name, args.merge_replicas if merge else args.replicas, args.merge_steps if merge else args.steps,
                        args.reps)
    print(json.dumps(res))


if __name__ == "__main__":
    import warnings
    warnings.simplefilter("ignore")              # (the pending-ring-length notice of policy_rollout / capture)
    main()
