"""The head of 2 act_dim outputs (log stds from the network) in the device PPO update, what can be checked without a GPU:
DeviceLearner(net_log_std=True) gets past the model-class check and refuses what is outside it by name, and without the
keyword says what it said; the three workspace functions size for the new parameter count and the new form's own workgroup
cap; the host-n gradient and a separate old log_std are refused from the arguments alone; DevicePolicy.share pairs heads of
the same form only; and the torch statement the kernels are tested against -- GaussianPolicy(net_log_std=True) through
ppo_update -- starts as the free form with log_std = -0.5 does."""
import ctypes
import os
import re
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_device_ppo_cpu import nets  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from flow_amd import _lib, build
    build.build()
    return _lib.load()


def nets_ls(D=3, A=1, layers=2, head_out=None, log_std=None):
    ph, _, _, vh, vhead = nets(D=D, A=A, layers=layers)
    return ph, torch.nn.Linear(32, 2 * A if head_out is None else head_out), log_std, vh, vhead


# ------------------------------------------------------------------------------------------------------- DeviceLearner
@pytest.mark.parametrize("D,A,layers", [(3, 1, 2), (65, 13, 3), (160, 32, 3)])
def test_the_keyword_gets_a_2a_head_past_the_model_class_check(D, A, layers):
    """CPU tensors and no handle: what is left to say is that the parameters must live on a GPU."""
    from flow_amd.utils.device_ppo import DeviceLearner
    with pytest.raises(ValueError, match="GPU"):
        DeviceLearner(None, *nets_ls(D, A, layers), net_log_std=True)


@pytest.mark.parametrize("kw,names", [
    (dict(A=1, head_out=3), "3 outputs is odd"),
    (dict(A=33), "act_dim A = 33"),
    (dict(A=2, log_std=torch.nn.Parameter(torch.zeros(2))), "log_std must be None"),
    (dict(layers=4), "4 hidden layers"),
    (dict(D=161), "obs_dim D = 161"),
])
def test_the_keyword_refuses_by_name_what_is_outside_the_class(kw, names):
    from flow_amd.utils.device_ppo import DeviceLearner
    with pytest.raises(NotImplementedError, match=re.escape(names)) as e:
        DeviceLearner(None, *nets_ls(**kw), net_log_std=True)
    assert "fs_ppo_model" in str(e.value)


def test_without_the_keyword_the_messages_are_the_parents():
    from flow_amd.utils.device_ppo import DeviceLearner
    for args in (nets(A=2, head_out=4), nets(A=1, head_out=2, free_log_std=False), nets_ls(3, 1, 2)):
        for kw in ({}, dict(net_log_std=False)):
            with pytest.raises(NotImplementedError, match="2A-output head") as e:
                DeviceLearner(None, *args, **kw)
            assert "fs_ppo_model" in str(e.value) and "is not built" in str(e.value)


# ----------------------------------------------------------------------------------------------------------- workspace
def model_ls(D, A, layers, width=32, activation=0, value=64, struct_size=None):
    """The head of 2 A outputs: log_std_dev NULL (fs_policy's convention).  The workspace functions never read the weights."""
    from flow_amd import _lib
    M = _lib.fs_ppo_model
    return M(struct_size=ctypes.sizeof(M) if struct_size is None else struct_size, obs_dim=D, act_dim=A, num_hidden=layers,
             hidden_width=width, activation=activation, policy_weights_dev=64, log_std_dev=None, value_weights_dev=value)


def packed_ls(D, A, layers):
    """[policy with its 2A-row head][value], no log_std slot: torch's parameter order."""
    trunk = 32 * D + 32 + (layers - 1) * 1056
    return (trunk + 33 * 2 * A) + (trunk + 33)


def groups_ls(lib, D, A, layers, n):
    """The workgroups behind the three workspace functions, which must agree."""
    P, m = packed_ls(D, A, layers), model_ls(D, A, layers)
    out = []
    for fn, per in ((lib.fs_ppo_workspace, P + 2), (lib.fs_ppo_loss_workspace, P + 4), (lib.fs_ppo_minibatch_workspace, P + 5)):
        floats = int(fn(ctypes.byref(m), n))
        assert floats > 0 and floats % per == 0, (fn, floats, per)
        out.append(floats // per)
    assert out[0] == out[1] == out[2], out
    return out[0]


def test_the_parameter_count_is_torchs():
    import train_vec
    for D, A in ((3, 1), (25, 5)):
        pi = train_vec.GaussianPolicy(D, A, net_log_std=True)
        assert sum(p.numel() for p in pi.parameters()) == packed_ls(D, A, 2)
    assert packed_ls(3, 1, 2) == 2467 and packed_ls(160, 32, 3) == 16673


# LDS per workgroup of the new form's plain gradient, by flowsim_learn.h ppo_grad_lds(.., ls = true):
#   4 (2 (32 D + 32 + 1056 L) + 1056 + 4384 + round4(P + 2)) bytes,   P = 2 (32 D + 32 + 1056 (L - 1)) + 66 A + 33
# -- the free form's with one more 1056-float head block and the new P.  The cap is 256 x min(4, floor(163840 / LDS)):
#   (160, 32, 3): P = 16673, 4 (17696 + 4384 + 16676) = 155024 B -> 1      (141, 20, 2): P = 12553, 125232 B -> 1
#   (65, 13, 3):  P =  9339, 4 (11616 + 4384 +  9344) = 101376 B -> 1      (25, 5, 2):   P =  4139,  61888 B -> 2
#   (3, 1, 2):    P =  2467, 4 ( 5536 + 4384 +  2472) =  49568 B -> 3      (1, 1, 1):    P =   227,  31648 B -> 5: four
CAPS = [(160, 32, 3, 256), (141, 20, 2, 256), (65, 13, 3, 256), (25, 5, 2, 512), (3, 1, 2, 768), (1, 1, 1, 1024)]


@pytest.mark.parametrize("D,A,layers,cap", CAPS)
def test_the_workspaces_pin_the_new_forms_workgroups_on_every_branch_of_the_cap(lib, D, A, layers, cap):
    assert groups_ls(lib, D, A, layers, 1) == 1 and groups_ls(lib, D, A, layers, 64) == 1
    assert groups_ls(lib, D, A, layers, 65) == 2
    assert groups_ls(lib, D, A, layers, 259) == 5
    assert groups_ls(lib, D, A, layers, 64 * (cap - 1) + 1) == cap                  # the last tile below the cap, partial
    assert groups_ls(lib, D, A, layers, 64 * cap) == cap
    assert groups_ls(lib, D, A, layers, 64 * cap + 1) == cap                        # one tile more: still the cap
    assert groups_ls(lib, D, A, layers, 64 * (2 * cap + 1) + 5) == cap              # (tests/test_device_ppo_head_gpu.py)
    assert groups_ls(lib, D, A, layers, 102400) == min(1600, cap)
    assert groups_ls(lib, D, A, layers, 2 ** 31 - 1) == cap


def test_the_workspaces_count_the_new_parameters_and_are_zero_outside_the_class(lib):
    m = model_ls(3, 1, 2)
    assert int(lib.fs_ppo_workspace(ctypes.byref(m), 1)) == 2467 + 2
    assert int(lib.fs_ppo_loss_workspace(ctypes.byref(m), 1)) == 2467 + 4
    assert int(lib.fs_ppo_minibatch_workspace(ctypes.byref(m), 128)) == 2 * (2467 + 5)
    from test_device_ppo_cpu import ppo_model
    assert int(lib.fs_ppo_workspace(ctypes.byref(ppo_model(3, 1, 2)), 1)) == 2437   # (the free form's stays)
    for fn in (lib.fs_ppo_workspace, lib.fs_ppo_loss_workspace, lib.fs_ppo_minibatch_workspace):
        for n in (0, -1, 2 ** 31):
            assert int(fn(ctypes.byref(m), n)) == 0
        for bad in (model_ls(161, 1, 2), model_ls(0, 1, 2), model_ls(3, 33, 2), model_ls(3, 0, 2), model_ls(3, 1, 4),
                    model_ls(3, 1, 0), model_ls(3, 1, 2, width=16), model_ls(3, 1, 2, activation=1),
                    model_ls(3, 1, 2, value=None), model_ls(3, 1, 2, struct_size=8)):
            assert int(fn(ctypes.byref(bad), 64)) == 0
        assert int(fn(None, 64)) == 0


# ----------------------------------------------------------------------------------------- refusals from the arguments
def test_the_host_n_gradient_and_a_separate_old_log_std_are_refused_without_a_handle(lib):
    """No handle (NULL) and pointers that are never followed."""
    from flow_amd import _lib
    m = model_ls(3, 1, 2)
    rc = lib.fs_ppo_grad_dev(None, ctypes.byref(m), 64, 64, 64, 64, 64, 64, 64, 0.2, 0.5, 1.0 / 64, 0, 64, 64, 64, 1 << 30)
    msg = lib.fs_last_error().decode()
    assert rc == _lib.FS_ERR_UNSUPPORTED and "fs_ppo_grad_dev" in msg and "fs_ppo_model" in msg and "log_std_dev" in msg, msg
    loss = _lib.fs_ppo_loss(struct_size=ctypes.sizeof(_lib.fs_ppo_loss), clip=0.2, vf_coef=0.5, kl_state_dev=64)
    rc = lib.fs_ppo_grad_loss_dev(None, ctypes.byref(m), ctypes.byref(loss), 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 0, 64, 64,
                                  64, 1 << 30)
    msg = lib.fs_last_error().decode()
    assert rc == _lib.FS_ERR_INVALID and "fs_ppo_grad_loss_dev" in msg and "log_std_old_dev" in msg, msg
    from test_device_ppo_minibatch_cpu import mb_struct
    mb = mb_struct(weights_dev=64)
    m2 = model_ls(3, 1, 2, value=64 + 4 * (packed_ls(3, 1, 2) - (32 * 3 + 32 + 1056 + 33)))
    args = [None, ctypes.byref(m2), ctypes.byref(loss), ctypes.byref(mb), 259, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64,
            1 << 30]
    rc = lib.fs_ppo_minibatch_dev(*args)
    msg = lib.fs_last_error().decode()
    assert rc == _lib.FS_ERR_INVALID and "fs_ppo_minibatch_dev" in msg and "log_std_old_dev" in msg, msg
    # the packed buffer of this form is [policy][value]: a value pointer behind a log_std slot is not it
    args[1] = ctypes.byref(model_ls(3, 1, 2, value=64 + 4 * (packed_ls(3, 1, 2) - (32 * 3 + 32 + 1056 + 33) + 1)))
    args[9] = None
    rc = lib.fs_ppo_minibatch_dev(*args)
    msg = lib.fs_last_error().decode()
    assert rc == _lib.FS_ERR_INVALID and "weights_dev" in msg and "[policy][value]" in msg, msg


# ---------------------------------------------------------------------------------------------------- DevicePolicy.share
def test_share_pairs_heads_of_the_same_form_and_shape():
    from flow_amd.utils.device_policy import DevicePolicy
    ph, head, _, _, _ = nets_ls(3, 2, 2)
    pol = DevicePolicy(ph, head, log_std=None, act_dim=2)
    other = types.SimpleNamespace(D=5, A=2, num_hidden=2, net_log_std=True)
    with pytest.raises(NotImplementedError, match=re.escape("(3, 2, 2)")) as e:
        pol.share(other)
    assert "the packed layouts differ" in str(e.value)
    with pytest.raises(NotImplementedError, match="no free log_std"):               # the parent's words for a free-head learner
        pol.share(types.SimpleNamespace(D=3, A=2, num_hidden=2))
    ph, head, ls, _, _ = nets(3, 2, 2)
    free = DevicePolicy(ph, head, log_std=ls, act_dim=2)
    with pytest.raises(NotImplementedError, match="net_log_std=True") as e:
        free.share(types.SimpleNamespace(D=3, A=2, num_hidden=2, net_log_std=True))
    assert "free log_std" in str(e.value)


# ------------------------------------------------------------------------------------------------ the torch statement
def test_the_initial_network_head_is_the_free_form_with_log_std_minus_a_half():
    """The log-std rows start at zero weights and bias -0.5: through ppo_update with the terms on, the same gradients for
    the trunk and the mean rows as the free form (the log stds do not depend on the trunk yet), and the free form's
    log_std gradient at the log-std bias."""
    import train_vec
    D, A, K, R = 5, 3, 6, 7
    torch.manual_seed(3)
    free = train_vec.GaussianPolicy(D, A).double()
    net = train_vec.GaussianPolicy(D, A, net_log_std=True).double()
    assert not hasattr(net, "log_std") and net.mu[4].out_features == 2 * A
    assert not bool(net.mu[4].weight[A:].any()) and net.mu[4].bias[A:].tolist() == [-0.5] * A
    with torch.no_grad():
        for i in (0, 2):
            net.mu[i].load_state_dict(free.mu[i].state_dict())
        net.mu[4].weight[:A].copy_(free.mu[4].weight)
        net.mu[4].bias[:A].copy_(free.mu[4].bias)
        net.value.load_state_dict(free.value.state_dict())
    g = torch.Generator().manual_seed(8)
    obs = torch.randn(K + 1, R, D, generator=g, dtype=torch.float64)
    act = torch.randn(K, R, A, generator=g, dtype=torch.float64)
    act[2, 3, 1] = float("nan")                                                     # an absent agent
    rew = torch.randn(K, R, generator=g, dtype=torch.float64)
    done = (torch.rand(K, R, generator=g) < 0.2).to(torch.uint8)
    o, a = obs[:K].reshape(K * R, D), torch.nan_to_num(act.reshape(K * R, A))
    with torch.no_grad():
        l0, v0, m0, s0 = free.logp_value_dist(o, a)
        l1, v1, m1, s1 = net.logp_value_dist(o, a)
    assert s0.shape == (A,) and s1.shape == (K * R, A) and m1.shape == (K * R, A)
    assert torch.allclose(l0, l1, rtol=1e-13, atol=1e-13) and torch.equal(v0, v1) and torch.allclose(m0, m1, rtol=1e-13, atol=1e-14)
    assert torch.equal(s1, torch.full_like(s1, -0.5)) and torch.equal(s0.detach(), torch.full_like(s0, -0.5))
    assert torch.equal(net.logp_value(o, a)[0], net.logp_value_dist(o, a)[0])
    for minibatch in (None, 16):
        for terms in (dict(), dict(kl=True, entropy_coef=0.01, vf_clip=0.5)):
            grads = []
            for pi in (free, net):
                kw = dict(terms)
                if kw.pop("kl", False):
                    kw["kl"] = train_vec.AdaptiveKL(0.02, 0.3)
                opt = torch.optim.SGD(pi.parameters(), lr=0.0)
                train_vec.ppo_update(pi, opt, [(obs, act, rew, done)], epochs=1, minibatch=minibatch, **kw)
                grads.append(pi)
            close = lambda x, y: torch.allclose(x, y, rtol=1e-11, atol=1e-13)     # noqa: E731
            for i in (0, 2):
                assert close(free.mu[i].weight.grad, net.mu[i].weight.grad) and close(free.mu[i].bias.grad, net.mu[i].bias.grad)
            assert close(free.mu[4].weight.grad, net.mu[4].weight.grad[:A])
            assert close(free.mu[4].bias.grad, net.mu[4].bias.grad[:A])
            assert close(free.log_std.grad, net.mu[4].bias.grad[A:])
            assert float(net.mu[4].weight.grad[A:].abs().max()) > 0                # (the log-std rows do get a gradient)
            for x, y in zip(free.value.parameters(), net.value.parameters()):
                assert close(x.grad, y.grad)


def test_the_loss_of_the_network_head_is_the_free_forms_at_the_start():
    """ppo_update's loss itself, term by term, through the functions it calls: the per-sample entropy of the network head
    at its start is the free form's single number."""
    import train_vec
    ls_free, ls_net = torch.full((3,), -0.5, dtype=torch.float64), torch.full((11, 3), -0.5, dtype=torch.float64)
    h0, h1 = train_vec._entropy(ls_free), train_vec._entropy(ls_net)
    assert h0.shape == () and h1.shape == (11,) and torch.allclose(h1, h0.expand(11), rtol=1e-15)


def test_the_flag_is_off_by_default():
    import train
    import train_vec
    assert train.parse_args(["singleagent_ring"]).net_log_std is False
    assert train.parse_args(["singleagent_ring", "--net_log_std"]).net_log_std is True
    seen = {}

    def fake(flow_params, **kw):
        seen.update(kw)
        return []
    real, train_vec.train_on_device = train_vec.train_on_device, fake
    try:
        train_vec.main(["--iterations", "1"])
        assert seen["net_log_std"] is False
        train_vec.main(["--iterations", "1", "--device_adam", "--net_log_std"])
        assert seen["net_log_std"] is True and seen["device_adam"] is True
    finally:
        train_vec.train_on_device = real
    assert train_vec.GaussianPolicy(3, 1).net_log_std is False
    with pytest.raises(NotImplementedError, match="--device_adam"):
        train_vec.train_on_device(None, device_update=True, net_log_std=True)
