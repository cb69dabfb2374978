"""The PPO update on the device, what can be checked without a GPU: the three entry points are declared, bound and
exported together; the ctypes mirror of fs_ppo_model has the C layout; DeviceLearner refuses every model outside its class
by name before it touches a device; the torch path stays the default of ppo_update and train_on_device."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))

ENTRY_POINTS = ("fs_ppo_eval_dev", "fs_gae_dev", "fs_ppo_grad_dev")


def test_header_binding_and_library_agree_on_the_entry_points():
    from flow_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flowsim.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fs_[a-z_0-9]+)\s*\(", text))
    build.build()
    lib = _lib.load()
    for name in ENTRY_POINTS + ("fs_ppo_workspace",):
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert hasattr(lib, name), name
    assert lib.fs_abi_version() == 8                        # additive: the ABI version stays


def test_fs_ppo_model_has_the_c_layout(tmp_path):
    from flow_amd import _lib
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "flowsim.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu\\n", sizeof(fs_ppo_model), offsetof(fs_ppo_model, act_dim),'
                   ' offsetof(fs_ppo_model, policy_weights_dev), offsetof(fs_ppo_model, log_std_dev),'
                   ' offsetof(fs_ppo_model, value_weights_dev)); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    M = _lib.fs_ppo_model
    assert out == [ctypes.sizeof(M), M.act_dim.offset, M.policy_weights_dev.offset, M.log_std_dev.offset,
                   M.value_weights_dev.offset]
    assert [n for n, _ in M._fields_] == ["struct_size", "obs_dim", "act_dim", "num_hidden", "hidden_width", "activation",
                                          "policy_weights_dev", "log_std_dev", "value_weights_dev"]


def nets(D=3, A=1, layers=2, width=32, head_out=None, value_out=1, free_log_std=True):
    lin = torch.nn.Linear
    dims = [D] + [width] * layers
    ph = [lin(dims[i], dims[i + 1]) for i in range(layers)]
    vh = [lin(dims[i], dims[i + 1]) for i in range(layers)]
    ls = torch.nn.Parameter(torch.zeros(A)) if free_log_std else None
    return ph, lin(width, A if head_out is None else head_out), ls, vh, lin(width, value_out)


@pytest.mark.parametrize("kw,names", [
    (dict(A=2, head_out=4), "2A-output head"),
    (dict(A=1, head_out=2, free_log_std=False), "2A-output head"),
    (dict(width=16), "hidden width other than 32"),
    (dict(layers=4), "4 hidden layers"),
    (dict(D=161), "obs_dim D = 161"),
    (dict(A=33), "act_dim A = 33"),
    (dict(value_out=2), "value network maps 32 units to 2 outputs"),
])
def test_device_learner_refuses_by_name_without_a_device(kw, names):
    """CPU tensors and no handle: the model class is checked first, so nothing below is reached."""
    from flow_amd.utils.device_ppo import DeviceLearner
    with pytest.raises(NotImplementedError, match=re.escape(names)) as e:
        DeviceLearner(None, *nets(**kw))
    assert "fs_ppo_model" in str(e.value)


def test_a_model_of_the_class_on_the_cpu_is_told_to_move():
    from flow_amd.utils.device_ppo import DeviceLearner
    with pytest.raises(ValueError, match="GPU"):
        DeviceLearner(None, *nets(D=160, A=32, layers=3))


def test_the_torch_path_stays_the_default():
    import train_vec
    assert inspect.signature(train_vec.ppo_update).parameters["learner"].default is None
    assert inspect.signature(train_vec.train_on_device).parameters["device_update"].default is False
    ap = {}

    def fake(flow_params, **kw):
        ap.update(kw)
        return []
    real, train_vec.train_on_device = train_vec.train_on_device, fake
    try:
        train_vec.main(["--iterations", "1"])
        assert ap["device_update"] is False
        train_vec.main(["--iterations", "1", "--device_update"])
        assert ap["device_update"] is True
    finally:
        train_vec.train_on_device = real
    import train
    assert train.parse_args(["singleagent_ring"]).device_update is False
    assert train.parse_args(["singleagent_ring", "--device_update"]).device_update is True


def test_ppo_update_without_a_learner_is_the_parent_update_bit_for_bit():
    """learner=None: the same weights after an update as the plain torch update written out in tests/test_ppo_absent_agents.py."""
    import train_vec
    from test_ppo_absent_agents import plain_update
    K, R, D = 6, 5, 3
    g = torch.Generator().manual_seed(4)
    shard = (torch.randn(K + 1, R, D, generator=g), torch.randn(K, R, 1, generator=g), torch.randn(K, R, generator=g),
             (torch.rand(K, R, generator=g) < 0.1).to(torch.uint8))
    out = []
    for fn in (train_vec.ppo_update, plain_update):
        torch.manual_seed(0)
        pi = train_vec.GaussianPolicy(D, 1)
        opt = torch.optim.Adam(pi.parameters(), lr=1e-2)
        fn(pi, opt, [shard], epochs=2)
        out.append(torch.cat([p.detach().reshape(-1) for p in pi.parameters()]))
    assert torch.equal(out[0], out[1])
