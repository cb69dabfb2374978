"""Checkpoints on the device update (--device_adam) and the evaluation script.

* DeviceLearner.state_dict / load_state_dict: one update on a stored shard, a checkpoint, a FRESH learner (other initial
  weights) with adopted parameters and a DevicePolicy sharing its buffer, the checkpoint loaded -- the next update on the
  same shard is the uninterrupted run's, bit for bit, in weights, m, v, state and kl_state, with minibatches on (the epoch
  counter travels); the adopted parameters and the shared policy see the loaded values; another model is refused by name.
* train_on_device(..., checkpoint_dir=) followed by examples/evaluate.py's evaluate_checkpoint, and the same for the
  adversarial trainer: finite returns, every replica's episode counted, the fused kernel named; --restore continues at
  iteration + 1; --episode_stats extends the line and leaves it alone when off."""
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "examples"))

import train_vec  # noqa: E402
from helpers import ring_spec  # noqa: E402

pytestmark = pytest.mark.gpu

D, A, K, R = 3, 1, 64, 8
NAMES = ("weights", "m", "v", "state", "kl_state", "mb_epoch")
UPDATE = dict(epochs=2, lr=1e-2, kl_target=0.02, kl_coef_init=0.2, entropy_coef=0.01, vf_clip=10.0, minibatch=128, shuffle_seed=5)


def shard(seed, dev):
    g = torch.Generator().manual_seed(seed)
    out = (torch.randn(K + 1, R, D, generator=g), torch.randn(K, R, A, generator=g), torch.randn(K, R, generator=g),
           (torch.rand(K, R, generator=g) < 0.1).to(torch.uint8))
    return tuple(t.to(dev).contiguous() for t in out)


def learner_and_policy(sim, seed, net_log_std):
    from flow_amd.utils.device_policy import DevicePolicy
    from flow_amd.utils.device_ppo import DeviceLearner
    torch.manual_seed(seed)
    pi = train_vec.GaussianPolicy(D, A, net_log_std=net_log_std).to("cuda:0")
    learner = DeviceLearner(sim, [pi.mu[0], pi.mu[2]], pi.mu[4], None if net_log_std else pi.log_std,
                            [pi.value[0], pi.value[2]], pi.value[4], net_log_std=net_log_std)
    learner.adopt_parameters()
    pol = DevicePolicy([pi.mu[0], pi.mu[2]], pi.mu[4], log_std=None if net_log_std else pi.log_std, seed=1).share(learner)
    return pi, learner, pol


def snapshot(learner):
    torch.cuda.synchronize()
    return {n: getattr(learner, n).detach().cpu().clone() for n in NAMES}


@pytest.mark.parametrize("net_log_std", [False, True])
def test_the_update_after_a_checkpoint_is_the_uninterrupted_update(tmp_path, net_log_std):
    from flow_amd.sim import FlowSim
    sim = FlowSim(ring_spec(R=2, N=5, bunching=0), "f32")
    dev = torch.device("cuda", 0)
    first, second = shard(1, dev), shard(2, dev)
    pi, learner, pol = learner_and_policy(sim, 0, net_log_std)
    learner.update([first], **UPDATE)
    path = train_vec.save_checkpoint(str(tmp_path), 0, train_vec.ring_flow_params(50),
                                     dict(av=train_vec.policy_state(pi, None, None, learner)), update_path="device_adam")
    at_save = snapshot(learner)
    learner.update([second], **UPDATE)
    want = snapshot(learner)
    assert int(at_save["mb_epoch"]) == UPDATE["epochs"] and float(at_save["state"][0]) > 0
    assert not torch.equal(at_save["kl_state"], torch.tensor([0.2, 0.0], dtype=torch.float64))
    # a fresh learner from another seed
    pi2, learner2, pol2 = learner_and_policy(sim, 99, net_log_std)
    assert not torch.equal(learner2.weights.cpu(), at_save["weights"])
    w_ptr, p_ptr = learner2.weights.data_ptr(), pol2.struct.weights_dev
    ck = train_vec.load_checkpoint(path)
    assert ck["update_path"] == "device_adam" and ck["policies"]["av"]["learner"]["descriptor"] == [D, A, 2, net_log_std]
    assert train_vec.restore_policy(ck["policies"]["av"], pi2, None, None, learner2, name="av") is True
    got = snapshot(learner2)
    for n in NAMES:
        assert torch.equal(got[n], at_save[n]), "after load: " + n
    # in place: the adopted parameters and the policy that shares the buffer see the loaded values
    assert learner2.weights.data_ptr() == w_ptr and pol2.struct.weights_dev == p_ptr == w_ptr
    flat = torch.cat([p.detach().reshape(-1) for p in learner2.params]).cpu()
    assert torch.equal(flat, at_save["weights"])
    assert all(p.data_ptr() >= w_ptr and p.data_ptr() < w_ptr + 4 * learner2.P for p in pi2.parameters())
    assert torch.equal(pol2.buf.cpu(), at_save["weights"][:learner2.n_policy])
    learner2.update([second], **UPDATE)
    got = snapshot(learner2)
    for n in NAMES:
        assert torch.equal(got[n], want[n]), "after the next update: " + n
    # another model is refused by name, before anything is written
    pi3 = train_vec.GaussianPolicy(D + 1, A, net_log_std=net_log_std).to("cuda:0")
    from flow_amd.utils.device_ppo import DeviceLearner
    other = DeviceLearner(sim, [pi3.mu[0], pi3.mu[2]], pi3.mu[4], None if net_log_std else pi3.log_std,
                          [pi3.value[0], pi3.value[2]], pi3.value[4], net_log_std=net_log_std)
    before = other.weights.clone()
    with pytest.raises(ValueError, match=re.escape("obs_dim D")):
        other.load_state_dict(ck["policies"]["av"]["learner"])
    assert torch.equal(other.weights, before)
    sim.close()


def _run(fn, params, tmp, lines, **kw):
    return fn(params, replicas=32, fragment=8, iterations=2, epochs=1, log=lines.append, device_update=True, device_adam=True,
              sgd_minibatch_size=128, kl_target=0.02, checkpoint_dir=str(tmp), **kw)


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """Two iterations of train_on_device on the ring (horizon 8 = the fragment: one episode per replica and iteration) with
    --device_adam, --episode_stats and a checkpoint directory: (directory, log lines, history, episode history)."""
    tmp = tmp_path_factory.mktemp("ckpt")
    lines = []
    params = train_vec.ring_flow_params(8)
    eps = []
    hist = _run(train_vec.train_on_device, params, tmp, lines, episode_stats=True, on_episodes=lambda it, s: eps.append((it, s)))
    assert [it for it, _ in eps] == [0, 1]
    return tmp, lines, hist, [s for _, s in eps], params


def test_train_on_device_writes_a_checkpoint_and_logs_the_episodes(trained):
    tmp, lines, hist, eps, _ = trained
    assert len(hist) == 2 and sorted(os.listdir(tmp)) == ["checkpoint_1"]            # (no frequency: the end alone)
    its = [ln for ln in lines if ln.startswith("iteration")]
    assert len(its) == 2 and all("episode_reward_mean" in ln and ln.rstrip().endswith("episodes 32") for ln in its)
    assert [e["episodes"] for e in eps] == [32, 32] and all(e["episode_len_mean"] == 8.0 for e in eps)
    assert all(np.isfinite(e["episode_reward_mean"]) and e["episode_reward_min"] <= e["episode_reward_mean"] <= e["episode_reward_max"]
               for e in eps)
    assert any(ln.startswith("checkpoint:") and ln.endswith("checkpoint_1") for ln in lines)


@pytest.mark.parametrize("stochastic", [False, True])
def test_evaluate_checkpoint(trained, stochastic):
    import evaluate
    ck = os.path.join(str(trained[0]), "checkpoint_1")
    res = evaluate.evaluate_checkpoint(ck, num_rollouts=32, fragment=8, stochastic=stochastic, log=lambda *a: None)
    print(res)
    assert res["kernel"] == "k_ring_policy" and res["path"] == "fused" and res["steps"] == 8 and res["iteration"] == 1
    assert res["episodes"] >= 32 and res["episode_len_mean"] == 8.0 and res["greedy"] is (not stochastic)
    for key in ("episode_reward_mean", "episode_reward_min", "episode_reward_max", "episode_reward_std"):
        assert np.isfinite(res[key]), key
    assert res["episode_reward_min"] <= res["episode_reward_mean"] <= res["episode_reward_max"]
    out = []
    evaluate.print_summary(res, log=out.append)
    text = "\n".join(out)
    assert "Return:" in text and "Average, std:" in text and "Episodes: 32" in text


def test_restore_continues_at_the_next_iteration(trained, tmp_path):
    """Two more iterations, numbered from 2, the optimiser state taken over; without --episode_stats the line is the line
    of before."""
    ck, params = os.path.join(str(trained[0]), "checkpoint_1"), trained[4]
    more = []
    _run(train_vec.train_on_device, params, tmp_path, more, restore=ck)
    its = [ln for ln in more if ln.startswith("iteration")]
    assert [int(ln.split()[1]) for ln in its] == [2, 3] and not any("episode_reward" in ln for ln in its)
    assert all(re.search(r"episodes ended \d+  KL", ln) for ln in its)
    assert any(ln.startswith("restore:") and "continuing at iteration 2" in ln for ln in more)
    assert not any("dropped" in ln for ln in more)
    assert sorted(os.listdir(tmp_path)) == ["checkpoint_3"]
    state = train_vec.load_checkpoint(os.path.join(str(tmp_path), "checkpoint_3"))
    learner = state["policies"]["av"]["learner"]
    assert float(learner["state"][0]) == 4 * (8 * 32 // 128) and int(learner["mb_epoch"]) == 4      # (the steps of 4 updates)


def test_restore_onto_the_torch_path_says_what_it_dropped(trained):
    ck, params = os.path.join(str(trained[0]), "checkpoint_1"), trained[4]
    lines = []
    train_vec.train_on_device(params, replicas=32, fragment=8, iterations=1, epochs=1, log=lines.append, restore=ck)
    assert any("dropped" in ln and "optimiser state" in ln for ln in lines)
    assert [int(ln.split()[1]) for ln in lines if ln.startswith("iteration")] == [2]


def test_the_adversarial_trainer_saves_both_policies_and_evaluates(tmp_path):
    import evaluate
    from test_train_adversarial_gpu import adversarial_flow_params
    params = adversarial_flow_params(horizon=8)
    lines = []
    eps = []
    hist = _run(train_vec.train_adversarial_on_device, params, tmp_path, lines, episode_stats=True,
                on_episodes=lambda it, s: eps.append(s))
    assert len(hist) == 2
    ck = os.path.join(str(tmp_path), "checkpoint_1")
    state = train_vec.load_checkpoint(ck)
    assert sorted(state["policies"]) == ["adversary", "av"] and state["model"]["adversarial"] is True
    assert not torch.equal(state["policies"]["av"]["learner"]["weights"], state["policies"]["adversary"]["learner"]["weights"])
    assert [e["episodes"] for e in eps] == [32, 32]
    res = evaluate.evaluate_checkpoint(ck, num_rollouts=32, fragment=8, log=lines.append)
    print(res)
    assert res["kernel"] == "k_loop_policy<Adversarial>" and res["episodes"] >= 32
    assert np.isfinite(res["episode_reward_mean"]) and np.isfinite(res["episode_reward_min"]) and np.isfinite(res["episode_reward_max"])
