"""Closed-loop env-steps/s of the reference's multi-agent experiments with one policy shared by the agents:
python scripts/bench_ma_policy.py [--replicas 4096] [--steps 500] [--reps 3]

Per experiment (multiagent_ring: MultiAgentWaveAttenuationPOEnv; multiagent_figure_eight: MultiAgentAccelPOEnv), two
numbers from the same process: the fused policy + step kernel (VecFlowEnv.policy_rollout, one launch per fragment) and
K single steps around the torch policy captured as one HIP graph (VecFlowEnv.capture).  One JSON object on stdout."""
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
    vec.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    res = {name: leg(name, args.replicas, args.steps, args.reps) for name in ("multiagent_ring", "multiagent_figure_eight")}
    print(json.dumps(res))


if __name__ == "__main__":
    import warnings
    warnings.simplefilter("ignore")              # (the pending-ring-length notice of policy_rollout / capture)
    main()
