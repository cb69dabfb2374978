"""The rest of the PPO update on the device (fs_adv_stats_dev, fs_adv_finish_dev, fs_ppo_grad_n_dev, fs_adam_dev;
DeviceLearner.update, DevicePolicy.share, train_on_device(device_adam=True)), what can be checked without a GPU:
the entry points are declared, bound and exported together; the numpy restatement of the Adam sequence (what the GPU
test holds fs_adam_dev to, bit for bit) is as close to torch float64 Adam as torch float32 is; the restatement of the
finish formula is ppo_update's torch expression bit for bit; device_adam is off by default; DevicePolicy.share and
DeviceLearner refuse what they do not serve, by name, before a device is touched."""
import inspect
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import device_adam_ref as ref  # noqa: E402

ENTRY_POINTS = ("fs_adv_stats_dev", "fs_adv_finish_dev", "fs_ppo_grad_n_dev", "fs_adam_dev")


def test_header_binding_and_library_agree_on_the_new_entry_points():
    from flow_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flowsim.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fs_[a-z_0-9]+)\s*\(", text))
    build.build()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert lib.fs_abi_version() == 8                        # additive: the ABI version stays


@pytest.mark.parametrize("P", [7, 259, 4000])
def test_the_adam_restatement_is_as_close_to_float64_adam_as_torch_float32(P):
    """Error over displacement after 10 steps, max|w - w64| / max|w64 - w0|: the restatement may show MARGIN times what
    torch float32 shows on the same inputs."""
    c = ref.adam_problem(P)
    assert any((x == 0).any() for x in c["grads"]) and (c["grads"][0][::7] == 0).all()
    mags = np.abs(np.concatenate(c["grads"]))
    mags = mags[mags > 0]
    assert mags.min() >= 0.99e-6 and mags.max() <= 1.0 and (P < 259 or (mags.min() < 1e-5 and mags.max() > 0.1))
    w = ref.run_adam_ref(c["w0"], c["grads"])[-1][0]
    err = ref.displacement_error(w, c["w64"], c["w0"])
    same = float(np.mean(w == c["w32"]))
    print("Adam P=%d: restatement %.3g, torch float32 %.3g (ratio %.2f); %.1f %% of the elements are torch float32's bits"
          % (P, err, c["err32"], err / c["err32"], 100 * same))
    assert c["err32"] > 0
    assert err <= ref.MARGIN * c["err32"]
    assert (w[::7] == c["w0"][::7]).all()                   # a gradient that is always zero moves nothing


@pytest.mark.parametrize("n,seed", [(5, 0), (64, 1), (259, 2), (4099, 3), (102400, 4)])
def test_the_finish_restatement_is_the_torch_expression_of_ppo_update_bit_for_bit(n, seed):
    g = torch.Generator().manual_seed(seed)
    adv = (torch.randn(n, generator=g) * 3 + 0.7).double()
    stats = torch.stack([adv.sum(), (adv * adv).sum(), torch.tensor(float(n), dtype=torch.float64)])
    cnt = stats[2]                                          # (ppo_update's own lines)
    mean = stats[0] / cnt
    std = ((stats[1] - cnt * mean * mean) / (cnt - 1)).clamp_min(0).sqrt()
    got = ref.finish_ref(stats.numpy())
    assert got.dtype == np.float64
    assert got[0].tobytes() == mean.numpy().tobytes() and got[1].tobytes() == std.numpy().tobytes() and got[2] == n
    # a variance that rounds below zero is clamped: n equal values
    flat = ref.finish_ref(np.array([n * 0.1, n * 0.1 * 0.1 * (1 - 1e-15), n], dtype=np.float64))
    assert flat[1] == 0.0


def test_device_adam_is_off_by_default():
    import train
    import train_vec
    assert inspect.signature(train_vec.train_on_device).parameters["device_adam"].default is False
    seen = {}

    def fake(flow_params, **kw):
        seen.update(kw)
        return []
    real, train_vec.train_on_device = train_vec.train_on_device, fake
    try:
        train_vec.main(["--iterations", "1"])
        assert seen["device_adam"] is False and seen["device_update"] is False
        train_vec.main(["--iterations", "1", "--device_update"])
        assert seen["device_adam"] is False and seen["device_update"] is True
        train_vec.main(["--iterations", "1", "--device_adam"])
        assert seen["device_adam"] is True and seen["device_update"] is True      # the flag implies the device update
    finally:
        train_vec.train_on_device = real
    assert train.parse_args(["singleagent_ring"]).device_adam is False
    assert train.parse_args(["singleagent_ring", "--device_adam"]).device_adam is True


def policy(D=3, A=1, layers=2, two_a=False):
    from flow_amd.utils.device_policy import DevicePolicy
    lin = torch.nn.Linear
    dims = [D] + [32] * layers
    hidden = [lin(dims[i], dims[i + 1]) for i in range(layers)]
    if two_a:
        return DevicePolicy(hidden, lin(32, 2 * A), log_std=None, act_dim=A)
    return DevicePolicy(hidden, lin(32, A), log_std=torch.nn.Parameter(torch.zeros(A)), act_dim=A)


def learner_shape(D=3, A=1, layers=2):
    """What DevicePolicy.share reads of a DeviceLearner before it touches its storage."""
    return types.SimpleNamespace(D=D, A=A, num_hidden=layers)


@pytest.mark.parametrize("kw,other,names", [
    (dict(two_a=True), dict(), "no free log_std"),
    (dict(A=2, two_a=True), dict(A=2), "no free log_std"),
    (dict(D=3), dict(D=4), "(3, 2, 1)"),
    (dict(layers=1), dict(layers=2), "hidden layers"),
    (dict(A=5, D=25), dict(A=4, D=25), "(25, 2, 4)"),
])
def test_device_policy_share_refuses_by_name_without_a_device(kw, other, names):
    with pytest.raises(NotImplementedError, match=re.escape(names)) as e:
        policy(**kw).share(learner_shape(**other))
    assert "DevicePolicy.share" in str(e.value)


def test_device_learner_still_refuses_the_2a_head_by_name_without_a_device():
    from flow_amd.utils.device_ppo import DeviceLearner
    from test_device_ppo_cpu import nets
    for kw in (dict(A=2, head_out=4), dict(A=1, head_out=2, free_log_std=False)):
        with pytest.raises(NotImplementedError, match="2A-output head") as e:
            DeviceLearner(None, *nets(**kw))
        assert "fs_ppo_model" in str(e.value)
    for name in ("adopt_parameters", "adam_step", "update", "adv_stats", "adv_finish", "gradients_n"):
        assert callable(getattr(DeviceLearner, name)), name
