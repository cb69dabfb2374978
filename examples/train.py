#!/usr/bin/env python3
"""Runner for RL experiments on the GPU step loop -- the command line of the reference's examples/train.py:34-71.

    python examples/train.py singleagent_ring [--rl_trainer device|es|ars|rllib] [--num_steps N] [--rollout_size K]
                                              [--num_cpus C] [--replicas R]

``--rl_trainer es`` / ``ars``: the reference's other two trainers (flow/benchmarks/rllib/es_runner.py, ars_runner.py) on
the device: ``replicas / 16`` perturbed policies roll out whole episodes in one launch per fragment, a workgroup per
member (train_vec.train_es_on_device; ``--es_sigma --es_stepsize --es_l2 --es_top --es_eval_members``).

``--rl_trainer device`` (default here): PPO with the rollout on the device -- R replicas of the experiment in one
handle, a fragment of ``rollout_size`` closed-loop steps (policy, Env.step, reset of finished episodes) replayed as one
HIP graph, observations / actions / the update never leave HBM (examples/train_vec.py).  It takes the place of the
reference's RLlib rollout workers, each of which drives one SUMO process (train.py:149-212).
``--rl_trainer rllib``: the reference's own route -- register the environment (flow.utils.registry.make_create_env) and
hand it to ray.tune with the reference's PPO settings; needs ray, which this image does not ship.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import flow_amd  # noqa: E402

flow_amd.install_as_flow()


def parse_args(args):
    parser = argparse.ArgumentParser(description="Train an RL experiment from exp_configs/rl.",
                                     epilog="python train.py EXP_CONFIG")
    parser.add_argument('exp_config', type=str,
                        help='module in exp_configs/rl/singleagent or exp_configs/rl/multiagent, or a benchmark '
                             '(flow.benchmarks: figureeight0, figureeight1, figureeight2)')
    parser.add_argument('--rl_trainer', type=str, default="device",
                        help='device (on-GPU PPO), es or ars (evolution strategies / augmented random search on the device: '
                             'one perturbed policy per workgroup) or rllib')
    parser.add_argument('--gpus', type=int, default=1, help='es / ars: GPUs (more than one is refused: not built)')
    parser.add_argument('--num_cpus', type=int, default=1, help='rollout workers (rllib only)')
    parser.add_argument('--num_steps', type=int, default=20, help='training iterations')
    parser.add_argument('--rollout_size', type=int, default=100, help='env steps per rollout fragment')
    parser.add_argument('--checkpoint_path', type=str, default=None,
                        help='rllib: checkpoint to restore (device: --checkpoint_dir / --restore)')
    parser.add_argument('--replicas', type=int, default=1024, help='device: environment replicas in the handle')
    parser.add_argument('--fuse_policy', action='store_true',
                        help='device: roll an action-vector policy (singleagent_merge, lord_of_the_rings, figureeight1 / figureeight2) out through the fused policy + '
                             'step kernel instead of the captured graph; where there is none (singleagent_bottleneck, compiled_highway_ring), '
                             'capture the graph around the policy kernel instead of the torch module')
    parser.add_argument('--device_update', action='store_true',
                        help='device: run the PPO update on the library\'s kernels (fs_ppo_eval_dev, fs_gae_dev, '
                             'fs_ppo_grad_dev) instead of torch')
    parser.add_argument('--device_adam', action='store_true',
                        help='device: run the whole PPO update, Adam included, on the device with no host round trip '
                             '(DeviceLearner.update); implies --device_update')
    parser.add_argument('--train_adversary', action='store_true',
                        help='device: train BOTH policies of an adversarial experiment (adversarial_figure_eight: the av '
                             'and the adversary that perturbs its accelerations, opposite rewards) -- one fused two-policy '
                             'rollout per fragment, one update per policy; without it such an experiment is refused')
    parser.add_argument('--epochs', type=int, default=4, help='device: passes over a rollout fragment per update')
    from train_vec import add_checkpoint_flags, add_es_flags, add_model_flags, add_ppo_loss_flags
    add_es_flags(parser)                    # --es_sigma --es_stepsize --es_l2 --es_top --es_eval_members
    add_checkpoint_flags(parser)            # --checkpoint_dir --checkpoint_freq --restore --episode_stats --checkpoint_env_state
                                            # --evaluation_interval --evaluation_steps: all off by default
    add_ppo_loss_flags(parser)              # --kl_target --kl_coeff --entropy_coeff --vf_clip --sgd_minibatch_size: all off by default
    add_model_flags(parser)                 # --net_log_std: off by default
    parser.add_argument('--reference_ppo', action='store_true',
                        help='device: the loss and settings the reference trains with (RLlib PPO as its train.py sets it '
                             'up): --kl_target 0.02 --kl_coeff 0.2 --vf_clip 10 --epochs 10, vf_loss_coeff 1.0, '
                             'clip_param 0.3.  With --sgd_minibatch_size 128 --device_adam on top, every epoch is a '
                             'shuffled pass of minibatch steps: the reference\'s optimisation; --net_log_std on top of '
                             'that gives the policy the reference\'s head of 2 x act_dim outputs (without it the log std '
                             'is a free parameter)')
    return parser.parse_known_args(args)[0]


def ppo_loss_settings(flags):
    """train_on_device's loss keywords from the flags.  --reference_ppo: what the reference's train.py hands RLlib
    (kl_target 0.02, num_sgd_iter 10) on top of RLlib's PPO defaults (kl_coeff 0.2, vf_clip_param 10, vf_loss_coeff 1.0,
    clip_param 0.3, entropy_coeff 0); gamma 0.999 and lambda 0.97 are train_on_device's already.  --reference_ppo keeps
    its meaning: the minibatches are a flag of their own, and ``--reference_ppo --sgd_minibatch_size 128 --device_adam`` is
    the reference's optimisation (num_sgd_iter passes of sgd_minibatch_size samples); the reference's model, the head of
    2 act_dim outputs, is the flag --net_log_std (train_device passes it on)."""
    if flags.reference_ppo:
        return dict(kl_target=0.02, kl_coeff=0.2, vf_clip=10.0, epochs=10, vf_coef=1.0, clip=0.3,
                    entropy_coeff=flags.entropy_coeff, sgd_minibatch_size=flags.sgd_minibatch_size)
    return dict(kl_target=flags.kl_target, kl_coeff=flags.kl_coeff, vf_clip=flags.vf_clip, epochs=flags.epochs,
                entropy_coeff=flags.entropy_coeff, sgd_minibatch_size=flags.sgd_minibatch_size)


def checkpoint_settings(flags):
    """train_on_device's checkpoint and log keywords from the flags (all off by default)."""
    return dict(checkpoint_dir=flags.checkpoint_dir, checkpoint_freq=flags.checkpoint_freq, restore=flags.restore,
                episode_stats=flags.episode_stats)


def env_state_settings(flags):
    """--checkpoint_env_state (both trainers) and --evaluation_interval / --evaluation_steps (train_on_device), off by default."""
    return dict(checkpoint_env_state=flags.checkpoint_env_state, evaluation_interval=flags.evaluation_interval,
                evaluation_steps=flags.evaluation_steps)


def load_experiment(name):
    """The module of an experiment: exp_configs/rl/singleagent first, then multiagent (train.py:318-330), then the
    benchmarks package (flow.benchmarks: figureeight0 / figureeight1 / figureeight2)."""
    for pkg in ("exp_configs.rl.singleagent", "exp_configs.rl.multiagent"):
        try:
            module = __import__(pkg, fromlist=[name])
            return getattr(module, name), pkg.endswith("multiagent")
        except (ImportError, AttributeError):
            continue
    try:
        import importlib
        return importlib.import_module("flow.benchmarks." + name), False
    except ImportError:
        pass
    raise ValueError("Unable to find experiment config %r" % name)


def train_rllib(submodule, flags):
    """The reference's RLlib set-up (train.py:110-212) over make_create_env; FlowVectorEnv lets RLlib step all
    replicas of a worker in one call."""
    try:
        import ray
        from ray.tune import run_experiments
        from ray.tune.registry import register_env
        try:
            from ray.rllib.agents.agent import get_agent_class
        except ImportError:
            from ray.rllib.agents.registry import get_agent_class
    except ImportError as e:
        raise ImportError("--rl_trainer rllib needs ray[rllib], which is not installed here; use --rl_trainer device") from e
    from copy import deepcopy
    from flow.utils.registry import make_create_env
    from flow.utils.rllib import FlowParamsEncoder
    flow_params = submodule.flow_params
    horizon = flow_params['env'].horizon
    config = deepcopy(get_agent_class("PPO")._default_config)
    config.update(num_workers=flags.num_cpus, train_batch_size=horizon * submodule.N_ROLLOUTS, gamma=0.999,
                  use_gae=True, kl_target=0.02, num_sgd_iter=10, horizon=horizon)
    config["lambda"] = 0.97
    config["model"].update({"fcnet_hiddens": [32, 32, 32]})
    config['env_config']['flow_params'] = json.dumps(flow_params, cls=FlowParamsEncoder, sort_keys=True, indent=4)
    config['env_config']['run'] = "PPO"
    create_env, gym_name = make_create_env(params=flow_params)
    register_env(gym_name, create_env)
    ray.init(num_cpus=flags.num_cpus + 1)
    exp = {"run": "PPO", "env": gym_name, "config": config, "checkpoint_freq": 20, "checkpoint_at_end": True,
           "max_failures": 999, "stop": {"training_iteration": flags.num_steps}}
    if flags.checkpoint_path is not None:
        exp['restore'] = flags.checkpoint_path
    run_experiments({flow_params["exp_tag"]: exp})


def train_device(submodule, flags, multiagent=False):
    from train_vec import train_on_device
    fp = submodule.flow_params
    fp['sim'].render = False
    # lord_of_the_rings (MultiWaveAttenuationPOEnv on MultiRingNetwork): every ring is a row of the handle with ONE agent,
    # so the rows are the sample streams of the shared policy -- RLlib's treatment of agents that share a policy -- and the
    # experiment takes singleagent_ring's flags and paths (n_ag = 1).  --episode_stats then reports per RING: RLlib's
    # policy_reward_mean/av, not its per-environment episode_reward_mean (the sum over an environment's rings)
    from flow_amd import _lib
    if getattr(fp['env_name'], 'FS_ENV', None) == _lib.FS_ENV_MULTI_WAVE_ATTENUATION_PO:
        multiagent = False
    # a CompiledEnv (FS_ENV_USER) has no fused policy + step kernel: --fuse_policy captures the graph around the eager policy
    # kernel, for its shared agents (OBSERVE = "rl") as for one RL vehicle
    user_head = getattr(fp['env_name'], 'FS_ENV', None) == _lib.FS_ENV_USER
    return train_on_device(fp, replicas=flags.replicas, fragment=flags.rollout_size, iterations=flags.num_steps,
                           shared_agents=multiagent, fuse_action_vector=flags.fuse_policy and not multiagent,
                           fuse_shared_agents=flags.fuse_policy and multiagent and user_head,
                           device_update=flags.device_update or flags.device_adam, device_adam=flags.device_adam,
                           net_log_std=flags.net_log_std, **checkpoint_settings(flags), **env_state_settings(flags),
                           **ppo_loss_settings(flags))


def train_es(submodule, flags, multiagent=False):
    """--rl_trainer es | ars: train_es_on_device (a population of perturbed policies, no backward pass)."""
    from train_vec import train_es_on_device
    from flow_amd import _lib
    fp = submodule.flow_params
    fp['sim'].render = False
    if getattr(fp['env_name'], 'FS_ENV', None) == _lib.FS_ENV_MULTI_WAVE_ATTENUATION_PO:
        multiagent = False                                  # (lord_of_the_rings: a ring per row, one agent each)
    return train_es_on_device(fp, mode=flags.rl_trainer.lower(), replicas=flags.replicas, fragment=flags.rollout_size,
                              iterations=flags.num_steps, sigma=flags.es_sigma, stepsize=flags.es_stepsize, l2=flags.es_l2,
                              top=flags.es_top, eval_members=flags.es_eval_members, shared_agents=multiagent, gpus=flags.gpus,
                              checkpoint_dir=flags.checkpoint_dir, checkpoint_freq=flags.checkpoint_freq, restore=flags.restore)


def train_adversary(submodule, flags):
    """--train_adversary: the two policies of an adversarial experiment ('av' and 'adversary', opposite rewards)."""
    from train_vec import train_adversarial_on_device
    fp = submodule.flow_params
    fp['sim'].render = False
    return train_adversarial_on_device(fp, replicas=flags.replicas, fragment=flags.rollout_size, iterations=flags.num_steps,
                                       device_update=flags.device_update or flags.device_adam,
                                       device_adam=flags.device_adam, net_log_std=flags.net_log_std,
                                       checkpoint_env_state=flags.checkpoint_env_state,
                                       **checkpoint_settings(flags), **ppo_loss_settings(flags))


def main(args):
    flags = parse_args(args)
    submodule, multiagent = load_experiment(flags.exp_config)
    if flags.rl_trainer.lower() == "rllib":
        return train_rllib(submodule, flags)
    if flags.rl_trainer.lower() in ("es", "ars"):
        if multiagent and (len(getattr(submodule, "POLICIES_TO_TRAIN", ["av"])) > 1 or flags.exp_config.startswith("adversarial")):
            raise NotImplementedError("--rl_trainer %s trains one policy; there is no population form of fs_policy_pair (%s "
                                      "trains two)" % (flags.rl_trainer, flags.exp_config))
        return train_es(submodule, flags, multiagent)
    if flags.rl_trainer.lower() == "device":
        # multi-agent experiments whose agents share the policy 'av' (multiagent_ring / _figure_eight / _merge: one
        # observation block and one action column per agent) train that ONE policy; adversarial_figure_eight has two
        # policies with opposite rewards: not this loop, but train_adversarial_on_device's behind --train_adversary
        two = multiagent and (len(getattr(submodule, "POLICIES_TO_TRAIN", ["av"])) > 1
                              or flags.exp_config.startswith("adversarial"))
        if flags.train_adversary:
            if not two:
                raise ValueError("--train_adversary trains the two policies of an adversarial experiment "
                                 "(adversarial_figure_eight); %s trains one" % flags.exp_config)
            return train_adversary(submodule, flags)
        if two:
            raise ValueError("--rl_trainer device trains one shared policy; %s trains %s: add --train_adversary to train "
                             "both (one fused two-policy rollout, one update per policy)"
                             % (flags.exp_config, getattr(submodule, "POLICIES_TO_TRAIN", "two")))
        return train_device(submodule, flags, multiagent)
    raise ValueError("rl_trainer should be 'device', 'es', 'ars' or 'rllib'.")


if __name__ == "__main__":
    main(sys.argv[1:])
