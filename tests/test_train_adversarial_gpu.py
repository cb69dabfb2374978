"""Training the two policies of adversarial_figure_eight on the device (examples/train_vec.py
train_adversarial_on_device, examples/train.py --train_adversary).

* wiring: the update step of the loop (train_vec.update_adversarial) hands the av (obs, act[0], rew, done) and the
  adversary (obs, act[1], -rew, done) -- a swapped column or a missing negation changes the weights;
* the command line trains both policies for two iterations on the fused kernel, on the torch update and on the
  reference's optimisation on the device."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "examples"))

pytestmark = pytest.mark.gpu


def adversarial_flow_params(horizon=1500):
    """examples/exp_configs/rl/multiagent/adversarial_figure_eight.py, from the package's own classes."""
    from copy import deepcopy

    from flow_amd.controllers import ContinuousRouter, IDMController, RLController
    from flow_amd.core.params import (EnvParams, InitialConfig, NetParams, SumoCarFollowingParams, SumoParams,
                                      VehicleParams)
    from flow_amd.envs.multiagent import AdversarialAccelEnv
    from flow_amd.networks import FigureEightNetwork
    from flow_amd.networks.figure_eight import ADDITIONAL_NET_PARAMS
    veh = VehicleParams()
    for veh_id, controller, count in (("human", (IDMController, {"noise": 0.2}), 13), ("rl", (RLController, {}), 1)):
        veh.add(veh_id=veh_id, acceleration_controller=controller, routing_controller=(ContinuousRouter, {}),
                car_following_params=SumoCarFollowingParams(speed_mode="obey_safe_speed"), num_vehicles=count)
    return dict(exp_tag="adversarial_figure_eight", env_name=AdversarialAccelEnv, network=FigureEightNetwork,
                simulator="traci", sim=SumoParams(sim_step=0.1, render=False),
                env=EnvParams(horizon=horizon, additional_params={"target_velocity": 20, "max_accel": 3, "max_decel": 3,
                                                                  "perturb_weight": 0.03, "sort_vehicles": False}),
                net=NetParams(additional_params=deepcopy(ADDITIONAL_NET_PARAMS)), veh=veh, initial=InitialConfig())


def test_each_policy_learns_from_its_own_column_and_the_adversary_from_the_negated_reward():
    import torch
    import train_vec
    from flow_amd.envs import VecFlowEnv
    from flow_amd.utils.device_policy import DevicePolicy
    from flow_amd.utils.device_ppo import DeviceLearner
    R, K = 32, 12
    dev = torch.device("cuda", 0)
    vec = VecFlowEnv(adversarial_flow_params(horizon=8), num_replicas=R, device=0)
    try:
        def learner(seed):
            torch.manual_seed(seed)
            pi = train_vec.GaussianPolicy(vec.obs_dim, 1).to(dev)
            ln = DeviceLearner(vec, [pi.mu[0], pi.mu[2]], pi.mu[4], pi.log_std, [pi.value[0], pi.value[2]], pi.value[4])
            ln.adopt_parameters()
            return pi, ln
        (pi_a, want_a), (pi_b, want_b) = learner(1), learner(2)
        (_, got_a), (_, got_b) = learner(1), learner(2)
        assert torch.equal(want_a.weights, got_a.weights) and not torch.equal(want_a.weights, want_b.weights)
        pol_a = DevicePolicy([pi_a.mu[0], pi_a.mu[2]], pi_a.mu[4], log_std=pi_a.log_std, seed=3).share(want_a)
        pol_b = DevicePolicy([pi_b.mu[0], pi_b.mu[2]], pi_b.mu[4], log_std=pi_b.log_std, seed=4).share(want_b)
        vec.reset()
        del vec.env.env_params.additional_params['perturb_weight']      # weight=None reads it: absent, the key is named
        with pytest.raises(ValueError, match="perturb_weight"):
            vec.policy_pair_rollout(pol_a, pol_b, K, reset_done=True)
        vec.env.env_params.additional_params['perturb_weight'] = 0.03
        rollout = vec.policy_pair_rollout(pol_a, pol_b, K, reset_done=True)
        assert vec.sim.last_kernel == "k_loop_policy<Adversarial>"
        obs, act, logp, rew, done = rollout
        assert tuple(act.shape) == (2, K, R) and tuple(logp.shape) == (2, K, R) and tuple(rew.shape) == (K, R)
        assert int((done != 0).sum()) >= R and float(rew.abs().sum()) > 0.0     # (horizon 8: episodes ended, rewards flowed)
        assert not torch.equal(act[0], act[1])
        kw = dict(epochs=2, lr=1e-3)
        want_a.update([(obs, act[0].unsqueeze(-1).contiguous(), rew, done)], **kw)
        want_b.update([(obs, act[1].unsqueeze(-1).contiguous(), (-rew).contiguous(), done)], **kw)
        train_vec.update_adversarial(rollout, lambda shard: got_a.update([shard], **kw), lambda shard: got_b.update([shard], **kw))
        torch.cuda.synchronize()
        assert torch.equal(got_a.weights, want_a.weights)
        assert torch.equal(got_b.weights, want_b.weights)
        assert bool(torch.isfinite(got_a.weights).all()) and bool(torch.isfinite(got_b.weights).all())
    finally:
        vec.close()


@pytest.mark.parametrize("extra", [[], ["--device_adam", "--reference_ppo", "--sgd_minibatch_size", "128", "--net_log_std"]],
                         ids=["torch_update", "reference_ppo_on_device"])
def test_train_script_trains_both_policies(extra):
    script = os.path.join(ROOT, "examples", "train.py")
    res = subprocess.run([sys.executable, script, "adversarial_figure_eight", "--train_adversary", "--num_steps", "2",
                          "--rollout_size", "12", "--replicas", "32"] + extra, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("iteration")]
    assert len(lines) == 2 and all(np.isfinite(float(ln.split()[5])) for ln in lines), res.stdout
    assert "k_loop_policy<Adversarial>" in res.stdout
    if extra:
        assert "av KL" in res.stdout and "adversary KL" in res.stdout
