"""Exact resume and in-training evaluation (examples/train_vec.py: checkpoint_env_state, restore, evaluation_interval).

Set-up as tests/test_checkpoint_gpu.py's ``_run``: 32 replicas, fragment 8, ``device_adam``, minibatches and the KL target on.

* four iterations in one go equal two iterations + checkpoint + restore + two iterations -- ``history`` and every tensor of
  the final ``learner.state_dict()`` (read from the last checkpoint) under ``torch.equal``, the environments' final state
  too -- on the fused ring kernel (also with a ring length redrawn per episode, which the host generator draws), on the
  graph around the policy kernel (``fuse_action_vector`` on singleagent_bottleneck) and for the two-policy trainer;
  without ``checkpoint_env_state`` the histories differ (today's behaviour: asserted, so the test is known to see it);
* ``evaluation_interval``: history and final weights are bit-equal to the run without it, ``on_evaluation`` receives 32
  finished episodes of length 8 per call, and the greedy evaluation mean is not the sampled training mean;
* a checkpoint written at 32 replicas restored into a run of 16 logs the layout difference, resets and trains;
* the graph around the torch module samples from torch's CUDA generator: with its state in the checkpoint the resumed run
  is exact as well, and without it it is not."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "examples"))

import train_vec  # noqa: E402

pytestmark = pytest.mark.gpu


def run(fn, params, tmp, lines, iterations, replicas=32, **kw):
    return fn(params, replicas=replicas, fragment=8, iterations=iterations, epochs=1, log=lines.append, device_update=True,
              device_adam=True, sgd_minibatch_size=128, kl_target=0.02, checkpoint_dir=str(tmp), **kw)


def final(tmp, it=3):
    return train_vec.load_checkpoint(os.path.join(str(tmp), "checkpoint_%d" % it))


def same_learners(a, b):
    assert sorted(a["policies"]) == sorted(b["policies"])
    for name in a["policies"]:
        la, lb = a["policies"][name]["learner"], b["policies"][name]["learner"]
        for key in la:
            if torch.is_tensor(la[key]):
                assert torch.equal(la[key], lb[key]), "%s: learner.%s" % (name, key)
            else:
                assert la[key] == lb[key], "%s: learner.%s" % (name, key)


def same_env(a, b):
    ea, eb = a["env"], b["env"]
    assert sorted(ea) == sorted(eb) and ea["handle_seed"] == eb["handle_seed"]
    for key in ("blob", "obs", "done"):
        assert torch.equal(ea["snapshot"][key], eb["snapshot"][key]), "env.snapshot." + key
    assert ea["snapshot"]["host"] == eb["snapshot"]["host"]
    if "carry" in ea:
        assert torch.equal(ea["carry"], eb["carry"])


def resume_equals_the_whole_run(fn, params, tmp_path, **kw):
    whole_lines, eps_whole, eps_parts = [], [], []
    more = dict(kw)
    if "episode_stats" in kw:
        more_whole = dict(kw, on_episodes=lambda it, s: eps_whole.append((it, s)))
        more = dict(kw, on_episodes=lambda it, s: eps_parts.append((it, s)))
    else:
        more_whole = dict(kw)
    whole = run(fn, params, tmp_path / "whole", whole_lines, 4, checkpoint_env_state=True, **more_whole)
    first = run(fn, params, tmp_path / "first", [], 2, checkpoint_env_state=True, **more)
    lines = []
    second = run(fn, params, tmp_path / "second", lines, 2, checkpoint_env_state=True,
                 restore=os.path.join(str(tmp_path / "first"), "checkpoint_1"), **more)
    print("whole %r\nparts %r" % (whole, first + second))
    assert any(ln.startswith("restore:") and "continue from the checkpoint's state" in ln for ln in lines), lines
    assert first == whole[:2]
    assert second == whole[2:]
    a, b = final(tmp_path / "whole"), final(tmp_path / "second")
    same_learners(a, b)
    same_env(a, b)
    if eps_whole:
        assert eps_whole == eps_parts
    return whole, lines


def ring_params(resample=False):
    params = train_vec.ring_flow_params(8)
    if resample:
        params["env"].additional_params["ring_length"] = [220, 270]
    return params


@pytest.mark.parametrize("resample", [False, True])
def test_resume_is_exact_on_the_fused_ring_kernel(tmp_path, resample):
    params = ring_params(resample)
    whole, lines = resume_equals_the_whole_run(train_vec.train_on_device, params, tmp_path, episode_stats=True)
    assert any("k_ring_policy" in ln for ln in lines)
    if resample:
        return
    # without the flag: the environments restart from a reset, and the run is another run
    plain = run(train_vec.train_on_device, params, tmp_path / "plain", [], 2)
    assert plain == whole[:2]                                   # (the flag changes nothing but the checkpoint)
    assert "env" not in final(tmp_path / "plain", 1)
    lines = []
    after = run(train_vec.train_on_device, params, tmp_path / "plain2", lines, 2,
                restore=os.path.join(str(tmp_path / "plain"), "checkpoint_1"))
    assert after != whole[2:]
    assert not any("continue from the checkpoint's state" in ln for ln in lines)


def bottleneck_params():
    from test_policy_wide_gpu import singleagent_bottleneck_params
    fp = singleagent_bottleneck_params()
    fp["sim"].seed = 11                                         # (the experiment ships seed = None: a seed drawn per handle)
    fp["env"] = copy.deepcopy(fp["env"])
    fp["env"].horizon = 8
    return fp


def test_resume_is_exact_on_the_graph_around_the_policy_kernel(tmp_path):
    """(The outflow reward of this eight-step horizon is zero throughout, so the history alone shows little here: the
    learner's tensors, which follow the observations, and the environments' final blob -- vehicles, inflow bookkeeping, the
    policy's draw counters -- carry the comparison.)"""
    whole, lines = resume_equals_the_whole_run(train_vec.train_on_device, bottleneck_params(), tmp_path, fuse_action_vector=True)
    assert any("around the policy kernel (k_policy_act_wide)" in ln for ln in lines), lines


def test_an_unseeded_experiment_resumes_on_the_seed_its_handle_drew(tmp_path):
    """``SumoParams(seed=None)`` (singleagent_ring as shipped) draws the handle's Philox key per process: the checkpoint
    carries it, and the restored environments are created with it -- the second half of a run is repeated by a restore of
    its own middle checkpoint."""
    params = ring_params(resample=True)
    params["sim"].seed = None
    whole = run(train_vec.train_on_device, params, tmp_path / "whole", [], 4, checkpoint_env_state=True, checkpoint_freq=2)
    again = run(train_vec.train_on_device, params, tmp_path / "again", [], 2, checkpoint_env_state=True,
                restore=os.path.join(str(tmp_path / "whole"), "checkpoint_1"))
    assert again == whole[2:]
    a, b = final(tmp_path / "whole"), final(tmp_path / "again")
    same_learners(a, b)
    same_env(a, b)
    assert a["env"]["handle_seed"] == b["env"]["handle_seed"]


def test_resume_is_exact_for_the_two_policy_trainer(tmp_path):
    from test_train_adversarial_gpu import adversarial_flow_params
    params = adversarial_flow_params(horizon=8)
    params["sim"].seed = 5
    whole, lines = resume_equals_the_whole_run(train_vec.train_adversarial_on_device, params, tmp_path)
    assert any("k_loop_policy<Adversarial>" in ln for ln in lines)


def test_training_with_evaluation_is_training_without_it_on_the_fused_kernel(tmp_path):
    params = ring_params()
    evs, eps, lines = [], [], []
    plain = run(train_vec.train_on_device, params, tmp_path / "plain", [], 3, episode_stats=True,
                on_episodes=lambda it, s: eps.append(s))
    with_ev = run(train_vec.train_on_device, params, tmp_path / "ev", lines, 3, episode_stats=True, evaluation_interval=1,
                  evaluation_steps=8, on_evaluation=lambda it, s: evs.append((it, s)))
    assert with_ev == plain
    same_learners(final(tmp_path / "plain", 2), final(tmp_path / "ev", 2))
    assert [it for it, _ in evs] == [0, 1, 2]
    for (_, ev), ep in zip(evs, eps):
        print("evaluation %r\ntraining   %r" % (ev, ep))
        assert ev["episodes"] == 32 and ev["episode_len_mean"] == 8.0
        assert np.isfinite(ev["episode_reward_mean"]) and ev["episode_reward_min"] <= ev["episode_reward_mean"] <= ev["episode_reward_max"]
        assert ev["episode_reward_mean"] != ep["episode_reward_mean"]          # the mean action, not the samples relabelled
    its = [ln for ln in lines if ln.startswith("iteration")]
    assert len(its) == 3 and all("evaluation/episode_reward_mean" in ln and ln.rstrip().endswith("evaluation/episodes 32") for ln in its)
    assert any(ln.startswith("evaluation: rollout: fused policy + step kernel (k_ring_policy)") for ln in lines), lines


def test_training_with_evaluation_is_training_without_it_on_the_graph(tmp_path):
    params = bottleneck_params()
    evs, lines = [], []
    plain = run(train_vec.train_on_device, params, tmp_path / "plain", [], 4, fuse_action_vector=True)
    with_ev = run(train_vec.train_on_device, params, tmp_path / "ev", lines, 4, fuse_action_vector=True, evaluation_interval=2,
                  evaluation_steps=8, on_evaluation=lambda it, s: evs.append((it, s)))
    assert with_ev == plain
    same_learners(final(tmp_path / "plain"), final(tmp_path / "ev"))
    assert [it for it, _ in evs] == [1, 3]
    assert all(ev["episodes"] >= 32 and ev["episode_len_mean"] <= 8.0 for _, ev in evs), evs     # (a collision ends one early)
    its = [ln for ln in lines if ln.startswith("iteration")]
    assert ["evaluation/" in ln for ln in its] == [False, True, False, True]


def test_a_checkpoint_of_another_layout_falls_back_to_a_reset_and_trains(tmp_path):
    params = ring_params()
    run(train_vec.train_on_device, params, tmp_path / "first", [], 1, checkpoint_env_state=True)
    lines = []
    hist = run(train_vec.train_on_device, params, tmp_path / "second", lines, 2, replicas=16, checkpoint_env_state=True,
               restore=os.path.join(str(tmp_path / "first"), "checkpoint_0"))
    assert len(hist) == 2 and all(np.isfinite(h) for h in hist)
    assert any(ln.startswith("restore:") and "another layout" in ln and "32 replicas" in ln and "16 replicas" in ln
               for ln in lines), lines
    assert [int(ln.split()[1]) for ln in lines if ln.startswith("iteration")] == [1, 2]


def short_ring_params():
    """train_vec.ring_flow_params(8) with 13 humans instead of 21: fourteen vehicles are outside the fused ring kernel's rows
    (18 .. 32), so the trainer captures the graph around the torch module -- on an environment whose every step depends on
    the sampled action."""
    from flow_amd.controllers import ContinuousRouter, IDMController, RLController
    from flow_amd.core.params import VehicleParams
    params = train_vec.ring_flow_params(8)
    veh = VehicleParams()
    veh.add(veh_id="human", acceleration_controller=(IDMController, {"noise": 0.2}), routing_controller=(ContinuousRouter, {}),
            num_vehicles=13)
    veh.add(veh_id="rl", acceleration_controller=(RLController, {}), routing_controller=(ContinuousRouter, {}), num_vehicles=1)
    params["veh"] = veh
    return params


def test_the_graph_around_the_torch_module_resumes_exactly_with_torchs_generator_state(tmp_path):
    """The torch module samples from torch's CUDA generator inside the captured graph.  The checkpoint keeps that
    generator's state (``torch.cuda.get_rng_state``) and the restore sets it back; a replayed graph takes its Philox offset
    from the generator at replay time, so the resumed run repeats the uninterrupted one.  And it is that state which does
    it: the same restore without it is another run."""
    params = short_ring_params()
    whole, lines = resume_equals_the_whole_run(train_vec.train_on_device, params, tmp_path)
    assert any("around the torch policy" in ln for ln in lines), lines
    assert any("torch's CUDA generator state too" in ln for ln in lines), lines
    assert len(set(whole)) == 4
    state_path = os.path.join(str(tmp_path / "first"), "checkpoint_1", "state.pt")
    state = torch.load(state_path, map_location="cpu", weights_only=True)
    del state["env"]["torch_cuda_rng"]
    torch.save(state, state_path)
    other = run(train_vec.train_on_device, params, tmp_path / "other", [], 2, checkpoint_env_state=True,
                restore=os.path.join(str(tmp_path / "first"), "checkpoint_1"))
    print("without the generator state %r" % (other,))
    assert other != whole[2:]
