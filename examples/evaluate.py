#!/usr/bin/env python3
"""Replay a trained policy and report its episode returns -- the numbers of the reference's
flow/visualize/visualizer_rllib.py (per-round ``Return``, then ``Average, std``) for a checkpoint of train.py /
train_vec.py (``--checkpoint_dir``), computed on the device.

    python examples/evaluate.py CHECKPOINT [--num_rollouts N] [--stochastic] [--fragment K]

CHECKPOINT is a ``checkpoint_<iteration>`` directory (state.pt, params.json).  A VecFlowEnv of N replicas (default 1024)
is built from params.json -- every replica is one of the visualizer's rollouts --, the policy is loaded into a
DevicePolicy that applies the MEAN action (``fs_policy.greedy``; ``--stochastic`` samples as training does), and
``horizon`` env steps run after a reset, in fragments of K (``--fragment`` or the largest divisor of the horizon below it)
with finished episodes reset inside the fragment, on the path
train_on_device takes for the experiment: the fused policy + step kernel if there is one, else a captured graph around
the policy kernel, else around the torch module with ``explore=False``.  ``VecFlowEnv.episode_stats`` accumulates over the
fragments; every episode that ended within those steps counts.  An adversarial checkpoint replays both policies
(k_loop_policy<Adversarial>) and reports the av's return; the adversary's is its negation.

Not reported: the visualizer's speed / outflow / throughput lines, rendering, emission files.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def evaluate_checkpoint(checkpoint, num_rollouts=1024, stochastic=False, fragment=100, seed=None, log=print):
    """Returns ``flow_amd.utils.episode_stats.summarize``'s dict (``episodes``, ``episode_reward_mean / min / max / std``,
    ``episode_len_mean`` ...) with ``kernel`` (``fs_last_kernel`` of the rollout: the fused kernel's name, or the step
    kernel inside the captured graph), ``path`` ('fused', 'kernel_graph' or 'torch_graph'), ``steps`` and ``iteration``."""
    import torch
    from train_vec import GaussianPolicy, choose_rollout, load_checkpoint, restore_policy
    from flow_amd.envs import VecFlowEnv
    from flow_amd.utils import episode_stats as es
    ck = load_checkpoint(checkpoint)
    flow_params, model = ck["flow_params"], ck.get("model", {})
    seed = int(ck.get("seed", 0)) if seed is None else int(seed)
    greedy = not stochastic
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    quiet = lambda *a: None                                                     # noqa: E731
    vec = VecFlowEnv(flow_params, num_replicas=int(num_rollouts), device=0)
    horizon = int(flow_params["env"].horizon)
    if horizon < 1:
        raise ValueError("evaluate_checkpoint: the environment's horizon is %d" % horizon)
    # the largest divisor of the horizon within `fragment`: a captured graph replays whole fragments, and exactly `horizon`
    # steps run on every path
    K = max(k for k in range(1, min(max(int(fragment), 1), horizon) + 1) if horizon % k == 0)

    def load(name):
        D, A, _, net_ls = ck["policies"][name]["descriptor"]
        pi = GaussianPolicy(D, A, net_log_std=net_ls).to(dev)
        restore_policy(ck["policies"][name], pi, log=quiet, name=name, model_only=True)
        return pi

    stats, steps = None, 0
    if model.get("adversarial"):
        from flow_amd.utils.device_policy import DevicePolicy
        pols = []
        for j, name in enumerate(("av", "adversary")):
            pi = load(name)
            pols.append(DevicePolicy([pi.mu[0], pi.mu[2]], pi.mu[4], log_std=None if pi.net_log_std else pi.log_std,
                                     seed=seed + 104729 * j, greedy=greedy))
        vec.reset()
        path = "fused"
        while steps < horizon:
            k = min(K, horizon - steps)
            out = vec.policy_pair_rollout(pols[0], pols[1], k, reset_done=True)
            kernel = vec.sim.last_kernel
            stats = vec.episode_stats(out[3], out[4], reset=steps == 0)
            steps += k
    else:
        pi = load("av")
        shared = bool(model.get("shared_agents"))
        fused, graph, graph_policy = choose_rollout(vec, pi, K, seed, log, shared_agents=shared,
                                                    fuse_action_vector=bool(model.get("fuse_action_vector")), greedy=greedy)
        path = "fused" if fused is not None else "kernel_graph" if graph_policy is not None else "torch_graph"
        while steps < horizon:
            if fused is not None:
                k = min(K, horizon - steps)
                _, _, _, rew, done = vec.policy_rollout(fused, k, reset_done=True)
            else:                                               # (a captured fragment has its length; K divides the horizon)
                k = K
                _, _, rew, done = graph.replay()
            kernel = vec.sim.last_kernel
            stats = vec.episode_stats(rew, done, reset=steps == 0)
            steps += k
    out = es.summarize(stats)                                   # (reads the device: the one synchronisation)
    out.update(kernel=kernel, path=path, steps=steps, iteration=int(ck["iteration"]), num_rollouts=int(num_rollouts),
               greedy=greedy)
    vec.close()
    return out


def print_summary(res, log=print):
    """The visualizer's summary wording (visualizer_rllib.py: 'Return', 'Average, std')."""
    log("==== Summary: %d rollouts of %d steps, %s actions, checkpoint iteration %d (%s: %s) ===="
        % (res["num_rollouts"], res["steps"], "mean" if res["greedy"] else "sampled", res["iteration"], res["path"], res["kernel"]))
    if not res["episodes"]:
        log("Return:\nno episode ended within %d steps" % res["steps"])
        return
    log("Return:\nmin %.4f, max %.4f over %d episodes" % (res["episode_reward_min"], res["episode_reward_max"], res["episodes"]))
    log("Average, std: {:.2f}, {:.5f}".format(res["episode_reward_mean"], res["episode_reward_std"]))
    log("Episodes: %d" % res["episodes"])
    log("Episode length, mean (min, max): %.1f (%d, %d)" % (res["episode_len_mean"], res["episode_len_min"], res["episode_len_max"]))


def main(argv=None):
    ap = argparse.ArgumentParser(description="Evaluate a checkpoint of train.py / train_vec.py on the device.")
    ap.add_argument("checkpoint", type=str, help="a checkpoint_<iteration> directory")
    ap.add_argument("--num_rollouts", type=int, default=1024, help="replicas, each one rollout of `horizon` steps")
    ap.add_argument("--stochastic", action="store_true", help="sample the actions as training does (default: the mean action)")
    ap.add_argument("--fragment", type=int, default=100, help="env steps per launch / captured graph")
    args = ap.parse_args(argv)
    res = evaluate_checkpoint(args.checkpoint, num_rollouts=args.num_rollouts, stochastic=args.stochastic, fragment=args.fragment)
    print_summary(res)
    return res


if __name__ == "__main__":
    main()
