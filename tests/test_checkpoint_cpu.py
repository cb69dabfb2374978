"""Checkpoints and the fs_policy.greedy field, what can be checked without a GPU: an update after save_checkpoint /
load_checkpoint into fresh objects is the uninterrupted run's second update bit for bit (torch path, CPU tensors);
params.json round-trips through get_flow_params; a model of another shape is refused by name; the new flags are off by
default; fs_policy keeps its C layout with the new field in the old padding; the library exports fs_episode_stats_dev."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))

import train_vec  # noqa: E402


def _shard(seed, K=6, R=5, D=3):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(K + 1, R, D, generator=g), torch.randn(K, R, 1, generator=g), torch.randn(K, R, generator=g),
            (torch.rand(K, R, generator=g) < 0.1).to(torch.uint8))


def _fresh(seed, net_log_std=False, D=3):
    torch.manual_seed(seed)
    pi = train_vec.GaussianPolicy(D, 1, net_log_std=net_log_std)
    return pi, torch.optim.Adam(pi.parameters(), lr=1e-2), train_vec.AdaptiveKL(0.02, 0.2)


KW = dict(epochs=3, entropy_coef=0.01, vf_clip=10.0, minibatch=8, shuffle_seed=5)


def _update(pi, opt, kl, it, shard):
    train_vec.ppo_update(pi, opt, [shard], kl=kl, epoch0=it * KW["epochs"], **KW)


def _same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


@pytest.mark.parametrize("net_log_std", [False, True])
def test_an_update_after_a_checkpoint_is_the_uninterrupted_update(tmp_path, net_log_std):
    shards = [_shard(1), _shard(2)]
    fp = train_vec.ring_flow_params(50)
    # the uninterrupted run: two updates in a row
    pi, opt, kl = _fresh(0, net_log_std)
    _update(pi, opt, kl, 0, shards[0])
    path = train_vec.save_checkpoint(str(tmp_path), 0, fp, dict(av=train_vec.policy_state(pi, opt, kl)), seed=0,
                                     update_path="torch")
    _update(pi, opt, kl, 1, shards[1])
    assert os.path.basename(path) == "checkpoint_0"
    assert sorted(os.listdir(path)) == ["params.json", "state.pt"]
    # fresh policy / optimiser / AdaptiveKL from ANOTHER seed, the checkpoint, the second update
    pi2, opt2, kl2 = _fresh(123, net_log_std)
    ck = train_vec.load_checkpoint(path)
    assert ck["iteration"] == 0 and ck["seed"] == 0 and ck["update_path"] == "torch"
    assert train_vec.restore_policy(ck["policies"]["av"], pi2, opt2, kl2, name="av") is True
    assert kl2.coef != 0.2 or kl2.mean_kl is not None                   # (the adapted state came with it)
    _update(pi2, opt2, kl2, ck["iteration"] + 1, shards[1])
    for (n, a), (_, b) in zip(pi.named_parameters(), pi2.named_parameters()):
        assert torch.equal(a, b), n
    assert _same(opt.state_dict(), opt2.state_dict())
    assert (kl.coef, kl.mean_kl) == (kl2.coef, kl2.mean_kl)


def test_state_pt_holds_plain_tensors_and_numbers(tmp_path):
    pi, opt, kl = _fresh(0)
    _update(pi, opt, kl, 0, _shard(1))
    path = train_vec.save_checkpoint(str(tmp_path), 7, train_vec.ring_flow_params(50),
                                     dict(av=train_vec.policy_state(pi, opt, kl)), seed=3, update_path="torch",
                                     model=dict(shared_agents=False))
    state = torch.load(os.path.join(path, "state.pt"), weights_only=True)        # (refuses anything but plain data)
    assert state["iteration"] == 7 and state["seed"] == 3 and state["model"] == dict(shared_agents=False)
    assert state["policies"]["av"]["descriptor"] == [3, 1, 2, False]

    def plain(v):
        if isinstance(v, dict):
            return all(isinstance(k, (str, int)) and plain(x) for k, x in v.items())
        if isinstance(v, (list, tuple)):
            return all(plain(x) for x in v)
        return v is None or isinstance(v, (bool, int, float, str)) or (torch.is_tensor(v) and v.device.type == "cpu")
    assert plain(state)


def test_params_json_round_trips_through_get_flow_params(tmp_path):
    from flow_amd.utils.rllib import get_flow_params
    fp = train_vec.ring_flow_params(50)
    pi, opt, kl = _fresh(0)
    path = train_vec.save_checkpoint(str(tmp_path), 0, fp, dict(av=train_vec.policy_state(pi, opt, kl)))
    back = get_flow_params(os.path.join(path, "params.json"))
    assert back["env_name"] is fp["env_name"] and back["network"] is fp["network"] and back["exp_tag"] == fp["exp_tag"]
    assert back["env"].horizon == 50 and back["env"].additional_params == fp["env"].additional_params
    assert back["net"].additional_params == fp["net"].additional_params
    assert back["sim"].sim_step == fp["sim"].sim_step and back["sim"].seed == fp["sim"].seed
    assert back["initial"].bunching == fp["initial"].bunching
    assert [(v["veh_id"], v["num_vehicles"], v["acceleration_controller"][0].__name__) for v in back["veh"].initial] == \
        [(v["veh_id"], v["num_vehicles"], v["acceleration_controller"][0].__name__) for v in fp["veh"].initial]
    # ... and what load_checkpoint hands back is that dict
    assert train_vec.load_checkpoint(path)["flow_params"]["env"].horizon == 50
    # a second generation writes the same file
    path2 = train_vec.save_checkpoint(str(tmp_path / "again"), 0, back, dict(av=train_vec.policy_state(pi, opt, kl)))
    import json
    first, second = (json.load(open(os.path.join(p, "params.json"))) for p in (path, path2))
    second.pop("tls")                                                   # (get_flow_params fills in the default lights)
    assert first == second


@pytest.mark.parametrize("other,name", [(dict(D=4), "obs_dim D"), (dict(net_log_std=True), "net_log_std")])
def test_a_descriptor_mismatch_is_refused_by_name(tmp_path, other, name):
    pi, opt, kl = _fresh(0)
    path = train_vec.save_checkpoint(str(tmp_path), 0, train_vec.ring_flow_params(50),
                                     dict(av=train_vec.policy_state(pi, opt, kl)))
    pi2, opt2, kl2 = _fresh(0, **other)
    before = [p.detach().clone() for p in pi2.parameters()]
    with pytest.raises(ValueError, match=re.escape(name)) as e:
        train_vec.restore_policy(train_vec.load_checkpoint(path)["policies"]["av"], pi2, opt2, kl2, name="av")
    assert "(3, 1, 2, False)" in str(e.value)                           # (the checkpoint's whole descriptor is named too)
    assert all(torch.equal(a, b) for a, b in zip(before, pi2.parameters()))     # (refused before anything was written)
    from flow_amd.utils.device_ppo import check_descriptor
    for k, field in enumerate(("obs_dim D", "act_dim A", "num_hidden", "net_log_std")):
        d = [3, 1, 2, False]
        d[k] = True if k == 3 else d[k] + 1
        with pytest.raises(ValueError, match=re.escape(field)):
            check_descriptor("DeviceLearner.load_state_dict", [3, 1, 2, False], d)


def test_another_update_path_loads_the_model_and_says_what_it_dropped():
    pi, opt, kl = _fresh(0)
    _update(pi, opt, kl, 0, _shard(1))
    entry = train_vec.policy_state(pi, opt, kl)
    entry["learner"] = entry.pop("opt")                                 # (as a --device_adam run would have written it)
    lines = []
    pi2, opt2, kl2 = _fresh(9)
    assert train_vec.restore_policy(entry, pi2, opt2, kl2, log=lines.append, name="av") is False
    assert len(lines) == 1 and "optimiser state" in lines[0] and "dropped" in lines[0] and "device_adam" in lines[0]
    assert all(torch.equal(a, b) for a, b in zip(pi.parameters(), pi2.parameters()))
    assert opt2.state_dict()["state"] == {} and kl2.coef == 0.2


def test_the_new_flags_are_off_by_default():
    import inspect
    import train
    for fn in (train_vec.train_on_device, train_vec.train_adversarial_on_device):
        p = inspect.signature(fn).parameters
        assert p["checkpoint_dir"].default is None and p["checkpoint_freq"].default is None
        assert p["restore"].default is None and p["episode_stats"].default is False
    got = {}

    def fake(flow_params, **kw):
        got.update(kw)
        return []
    real, train_vec.train_on_device = train_vec.train_on_device, fake
    try:
        train_vec.main(["--iterations", "1"])
        assert got["checkpoint_dir"] is None and got["restore"] is None and got["episode_stats"] is False
        train_vec.main(["--iterations", "1", "--checkpoint_dir", "d", "--checkpoint_freq", "5", "--restore", "d/checkpoint_4",
                        "--episode_stats"])
        assert (got["checkpoint_dir"], got["checkpoint_freq"], got["restore"], got["episode_stats"]) == \
            ("d", 5, "d/checkpoint_4", True)
    finally:
        train_vec.train_on_device = real
    flags = train.parse_args(["singleagent_ring"])
    assert train.checkpoint_settings(flags) == dict(checkpoint_dir=None, checkpoint_freq=None, restore=None, episode_stats=False)
    flags = train.parse_args(["singleagent_ring", "--checkpoint_dir", "d", "--episode_stats"])
    assert train.checkpoint_settings(flags)["checkpoint_dir"] == "d" and flags.episode_stats is True
    assert [train_vec._checkpoint_due(it, 9, 4) for it in range(10)] == [it in (3, 7, 9) for it in range(10)]
    assert [train_vec._checkpoint_due(it, 2, None) for it in range(3)] == [False, False, True]


def test_the_mean_action_of_the_torch_fallback():
    for net_log_std in (False, True):
        pi, _, _ = _fresh(0, net_log_std)
        obs = torch.randn(7, 3)
        mu = pi.mu(obs)[..., :1]
        assert torch.equal(pi.act(obs, explore=False), mu)
        torch.manual_seed(1)
        a = pi.act(obs)
        torch.manual_seed(1)
        assert torch.equal(a, pi.act(obs, explore=True)) and not torch.equal(a, mu)


# ------------------------------------------------------------------------------------------------ the ABI of fs_policy
def test_fs_policy_keeps_its_layout_with_greedy_in_the_padding(tmp_path):
    from flow_amd import _lib
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "flowsim.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(fs_policy), offsetof(fs_policy, greedy), '
                   'offsetof(fs_policy, weights_dev), offsetof(fs_policy, activation), offsetof(fs_policy, log_std_dev), '
                   'offsetof(fs_policy, seed)); return 0;}\n')
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, greedy, weights, activation, log_std, seed = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    P = _lib.fs_policy
    assert size == ctypes.sizeof(P) == 48
    assert greedy == P.greedy.offset == 20 and activation == P.activation.offset == 16
    assert weights == P.weights_dev.offset == 24
    assert (log_std, seed) == (P.log_std_dev.offset, P.seed.offset) == (32, 40)
    assert [n for n, _ in P._fields_] == ["struct_size", "obs_dim", "num_hidden", "hidden_width", "activation", "greedy",
                                          "weights_dev", "log_std_dev", "seed"]
    assert P(struct_size=48).greedy == 0                                # (ctypes zeroes the struct: sampling)


def test_the_library_exports_fs_episode_stats_dev():
    from flow_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flowsim.h")).read(), flags=re.S)
    assert "fs_episode_stats_dev" in set(re.findall(r"\b(fs_[a-z_0-9]+)\s*\(", text))
    assert "fs_episode_stats_dev" in _lib.EXPORTS
    build.build()
    lib = _lib.load()
    assert hasattr(lib, "fs_episode_stats_dev")
    assert lib.fs_abi_version() == 8                                    # additive: the ABI version stays
    assert "k_episode_stats" in open(os.path.join(ROOT, "include", "flowsim.h")).read()
