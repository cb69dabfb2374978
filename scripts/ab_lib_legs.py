"""A/B of two builds of libflowsim.so on the ring and figure-eight legs, one process per sample:
    FLOWSIM_LIB=<library> python scripts/ab_lib_legs.py sample OUT.json       # one sample per leg of that library
    python scripts/ab_lib_legs.py table A1.json B1.json A2.json B2.json ...   # alternating samples -> the table

Legs: bench.py's rl_ring (open loop and closed_loop_fused_policy, three labels), c3_figure_eight, c3_closed_loop (both
heads), the fused rate of scripts/bench_ma_policy.py for multiagent_ring / multiagent_figure_eight / multiagent_merge and
of scripts/bench_merge_po.py for singleagent_merge (env-steps/s).
Boxes differ by ~25 %: run every sample of a table in one job, the libraries alternating.  The table gives, per leg,
the samples, the median of each library and the spread of library A against itself ((max - min) / median): B holds A's
rate when its median lies within that spread of A's."""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "examples"), os.path.join(ROOT, "scripts")):
    sys.path.insert(0, p)


def sample():
    import warnings
    import torch
    warnings.simplefilter("ignore")              # (the pending-ring-length notice of policy_rollout)
    import bench
    import bench_ma_policy
    import flow_amd
    from flow_amd.envs import VecFlowEnv
    from flow_amd.utils.device_policy import DevicePolicy
    from train_vec import GaussianPolicy
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    out = {}
    rl = bench.rl_ring_legs(dev)
    for label in ("f32_noise_0.2", "mixed_noise_0.2", "mixed_quiet"):
        for form in ("open_loop", "closed_loop_fused_policy"):
            out["rl_ring/%s/%s" % (label, form)] = rl[label][form]["value"]
    out["c3_figure_eight"] = bench.c3_leg(dev)["value"]
    c3 = bench.c3_closed_loop_leg(dev)
    out["c3_closed_loop/po_head"] = c3["po_head"]["value"]
    out["c3_closed_loop/accel_head"] = c3["accel_head"]["value"]
    flow_amd.install_as_flow()
    for name in ("multiagent_ring", "multiagent_figure_eight"):      # bench_ma_policy.leg without its captured-graph half
        fp = importlib.import_module("exp_configs.rl.multiagent." + name).flow_params
        torch.manual_seed(0)
        vec = VecFlowEnv(fp, num_replicas=4096, device=0)
        pi = GaussianPolicy(vec.obs_dim // vec.act_dim, 1).to(dev)
        fused = DevicePolicy([pi.mu[0], pi.mu[2]], pi.mu[4], log_std=pi.log_std, seed=0)
        vec.reset()
        bufs = vec.policy_rollout(fused, 500, reset_done=True)
        torch.cuda.synchronize()
        t = bench_ma_policy.timed(lambda: vec.policy_rollout(fused, 500, reset_done=True, out=bufs), 3)
        out["ma_policy/%s/fused" % name] = 500 * 4096 / t
        vec.close()
    # the merge heads, one 600-step episode of 1024 replicas per launch: multiagent_merge with its actions applied
    # (bench_ma_policy's leg: k_merge_policy) and singleagent_merge (bench_merge_po's leg (d): k_merge_policy<PO>)
    import copy
    from flow_amd.envs.multiagent.merge import MultiAgentMergePOEnv

    class MultiAgentMergeAppliedPOEnv(MultiAgentMergePOEnv):
        APPLY_ENUMERATE_QUIRK = False
    ma = dict(importlib.import_module("exp_configs.rl.multiagent.multiagent_merge").flow_params,
              env_name=MultiAgentMergeAppliedPOEnv)
    po = dict(importlib.import_module("exp_configs.rl.singleagent.singleagent_merge").flow_params)
    po["sim"] = copy.deepcopy(po["sim"])
    po["sim"].seed = 11                                    # (the experiment ships seed = None: a seed drawn per handle)
    for leg, fp, shared in (("ma_policy/multiagent_merge/fused", ma, True), ("merge_po/singleagent_merge/fused", po, False)):
        torch.manual_seed(0)
        vec = VecFlowEnv(fp, num_replicas=1024, device=0)
        if shared:
            pi = GaussianPolicy(vec.obs_dim // vec.act_dim, 1).to(dev)
            fused = DevicePolicy([pi.mu[0], pi.mu[2]], pi.mu[4], log_std=pi.log_std, seed=0)
        else:
            pi = GaussianPolicy(vec.obs_dim, vec.act_dim).to(dev)
            fused = DevicePolicy([pi.mu[0], pi.mu[2]], pi.mu[4], log_std=pi.log_std, seed=0, act_dim=vec.act_dim)
        vec.reset()
        bufs = vec.policy_rollout(fused, 600, reset_done=True)
        torch.cuda.synchronize()
        t = bench_ma_policy.timed(lambda: vec.policy_rollout(fused, 600, reset_done=True, out=bufs), 3)
        out[leg] = 600 * 1024 / t
        vec.close()
    return out


def table(files):
    runs = [json.load(open(f)) for f in files]
    a, b = runs[0::2], runs[1::2]
    med = lambda xs: sorted(xs)[len(xs) // 2]
    rows = {}
    for leg in runs[0]:
        xa, xb = [r[leg] for r in a], [r[leg] for r in b]
        spread = (max(xa) - min(xa)) / med(xa)
        rows[leg] = {"a": xa, "b": xb, "a_median": med(xa), "b_median": med(xb), "a_spread": spread,
                     "b_over_a": med(xb) / med(xa), "b_within_a_spread": abs(med(xb) / med(xa) - 1.0) <= spread}
    return rows


if __name__ == "__main__":
    if sys.argv[1] == "sample":
        res = sample()
        with open(sys.argv[2], "w") as f:
            json.dump(res, f, indent=1)
    else:
        res = table(sys.argv[2:])
    print(json.dumps(res))
