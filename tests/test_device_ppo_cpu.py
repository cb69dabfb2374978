"""The PPO update on the device, what can be checked without a GPU: the three entry points are declared, bound and
exported together; the ctypes mirror of fs_ppo_model has the C layout; DeviceLearner refuses every model outside its class
by name before it touches a device; the torch path stays the default of ppo_update and train_on_device; the workgroup
count of k_ppo_grad behind fs_ppo_workspace on every branch of its cap; the two restatements of tests/device_ppo_ref.py
(the composition of tile sums, the order of k_adv_stats) against float64 and against examples worked by hand."""
import ctypes
import inspect
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import device_ppo_ref as ppo_ref  # noqa: E402

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


# ------------------------------------------------------------------------------------------ fs_ppo_workspace: the cap
def ppo_model(D, A, layers, width=32, activation=0, value=64, struct_size=None):
    """fs_ppo_workspace never reads the weights: any non-zero address stands for them."""
    from flow_amd import _lib
    M = _lib.fs_ppo_model
    return M(struct_size=ctypes.sizeof(M) if struct_size is None else struct_size, obs_dim=D, act_dim=A, num_hidden=layers,
             hidden_width=width, activation=activation, policy_weights_dev=64, log_std_dev=64, value_weights_dev=value)


def groups_of(lib, D, A, layers, n):
    """Workgroups of k_ppo_grad as the library sizes its workspace: fs_ppo_workspace / (P + 2)."""
    floats = int(lib.fs_ppo_workspace(ctypes.byref(ppo_model(D, A, layers)), n))
    per_group = ppo_ref.packed(D, A, layers) + 2
    assert floats % per_group == 0, (floats, per_group)
    return floats // per_group


@pytest.fixture(scope="module")
def lib():
    from flow_amd import _lib, build
    build.build()
    return _lib.load()


# LDS per workgroup by flowsim_learn.h ppo_grad_lds = 4 (2 (32 D + 32 + 1056 L) + 4384 + round4(P + 2)) bytes; the cap is
# 256 x min(4, floor(163840 / LDS)): 146704 B -> 1, 118448 B -> 1, 57024 B -> 2, 45216 B -> 3, 27296 B -> 6, four at the most
@pytest.mark.parametrize("D,A,layers,cap", [(160, 32, 3, 256), (141, 20, 2, 256), (25, 5, 2, 512), (3, 1, 2, 768),
                                            (1, 1, 1, 1024)])
def test_workspace_pins_the_workgroups_of_the_gradient_on_every_branch_of_the_cap(lib, D, A, layers, cap):
    assert groups_of(lib, D, A, layers, 1) == 1 and groups_of(lib, D, A, layers, 64) == 1
    assert groups_of(lib, D, A, layers, 65) == 2
    assert groups_of(lib, D, A, layers, 64 * (cap - 1) + 1) == cap                  # the last tile below the cap, partial
    assert groups_of(lib, D, A, layers, 64 * cap) == cap
    assert groups_of(lib, D, A, layers, 64 * cap + 1) == cap                        # one tile more: still the cap
    assert groups_of(lib, D, A, layers, 64 * (2 * cap + 1) + 5) == cap              # (tests/test_device_ppo_scale_gpu.py)
    assert groups_of(lib, D, A, layers, 102400) == min(1600, cap)                   # 1024 replicas x 100 steps
    assert groups_of(lib, D, A, layers, 2 ** 31 - 1) == cap


def test_workspace_is_zero_outside_the_range_of_n_and_outside_the_model_class(lib):
    def floats(model, n):
        return int(lib.fs_ppo_workspace(ctypes.byref(model), n))
    good = ppo_model(3, 1, 2)
    assert floats(good, 1) == ppo_ref.packed(3, 1, 2) + 2 == 2437
    for n in (0, -1, 2 ** 31, 2 ** 40):
        assert floats(good, n) == 0, n
    for bad in (ppo_model(161, 1, 2), ppo_model(0, 1, 2), ppo_model(3, 33, 2), ppo_model(3, 0, 2), ppo_model(3, 1, 4),
                ppo_model(3, 1, 0), ppo_model(3, 1, 2, width=16), ppo_model(3, 1, 2, activation=1),
                ppo_model(3, 1, 2, value=None), ppo_model(3, 1, 2, struct_size=8)):
        assert floats(bad, 64) == 0
    assert int(lib.fs_ppo_workspace(None, 64)) == 0


# -------------------------------------------------------------------------------- compose_ref: the composition of tiles
def test_compose_ref_on_three_tiles_and_two_workgroups_worked_by_hand():
    """G = 2: workgroup 0 takes tiles 0 and 2, workgroup 1 tile 1; out = ((0 + T0) + T2) + (0 + T1).  With u = 2^-24, 1 + u
    rounds to 1 (a tie, to even) and 1 + 2 u is exact, so the order shows in the bits."""
    u = 2.0 ** -24
    #                 column 0    1    2     3
    T = torch.tensor([[1.0,      u,   u,   -0.0],          # tile 0
                      [u,        1.0, u,   -0.0],          # tile 1
                      [u,        u,   1.0, -0.0]], dtype=torch.float32)
    # column 0: (1 + u) + u: 1 + u = 1 twice                           column 1: (u + u) + 1 = 1 + 2 u
    # column 2: (u + 1) + u = 1 + u = 1                                column 3: 0 + -0 = +0, and +0 it stays
    out = ppo_ref.compose_ref(T, 2)
    assert out.dtype == torch.float32 and out.tolist() == [1.0, 1.0 + 2 * u, 1.0, 0.0]
    assert not bool(torch.signbit(out[3]))
    # the other counts on the same sums: G = 1 is tile after tile, G = 3 one tile per workgroup (the same adds here)
    assert ppo_ref.compose_ref(T, 1).tolist() == [1.0, 1.0, 1.0 + 2 * u, 0.0]
    assert ppo_ref.compose_ref(T, 3).tolist() == [1.0, 1.0, 1.0 + 2 * u, 0.0]
    assert T[0, 3].item() == 0.0 and bool(torch.signbit(T[0, 3]))                   # (the input is left as it was)


@pytest.mark.parametrize("tiles,G", [(37, 1), (37, 5), (37, 37), (515, 256)])
def test_compose_ref_against_float64(tiles, G):
    g = torch.Generator().manual_seed(tiles + G)
    T = torch.randn(tiles, 50, generator=g) * 10.0 ** torch.randint(-3, 3, (tiles, 50), generator=g).float()
    out = ppo_ref.compose_ref(T, G)
    exact = T.double().sum(0)
    # a float32 sum of m terms in ANY order: |error| <= (m - 1) u sum|x| to first order, u = 2^-24; m u covers the rest
    bound = tiles * 2.0 ** -24 * T.double().abs().sum(0)
    assert bool(((out.double() - exact).abs() <= bound).all())
    assert bool((out.double() != exact).any())                                      # (float32 adds: not the float64 sum)
    if 1 < G < tiles:
        assert not torch.equal(out, ppo_ref.compose_ref(T, 1))                      # the order is in the bits


# ------------------------------------------------------------------------------ adv_stats_ref: the order of k_adv_stats
def test_adv_groups_is_the_header_s():
    assert [ppo_ref.adv_groups(n) for n in (1, 1024, 1025, 262144, 262145, 524288, 524289, 525317, 2 ** 31 - 1)] \
        == [1, 1, 2, 256, 257, 512, 512, 512, 512]


def test_adv_stats_ref_on_orders_worked_by_hand():
    """n = 1025: G = 2, so lane t of workgroup b adds rows 256 b + t, + 512, + 1024.  With v = 2^-53, 1 + v rounds to 1 in
    double (a tie, to even) and v + v = 2^-52 is exact: where the two small terms meet before they meet the 1 is in the bits."""
    v, n = 2.0 ** -53, 1025
    present = np.ones(n, dtype=np.bool_)

    def total(rows):
        adv = np.zeros(n, dtype=np.float32)
        adv[0] = 1.0
        adv[list(rows)] = v
        out = ppo_ref.adv_stats_ref(adv, present)
        assert out.dtype == np.float64 and out.shape == (3,) and out[1] == 1.0 and out[2] == n
        return out[0]
    assert np.float32(v) == v
    assert total([512, 1024]) == 1.0                        # the same lane as the 1, k = 1 and 2: (1 + v) + v
    assert total([1, 129]) == 1.0 + 2 * v                   # lanes 1 and 129 meet at half = 128, lane 0 at half = 1
    assert total([1, 2]) == 1.0                             # lane 2 joins lane 0 at half = 2, lane 1 at half = 1
    assert total([256, 257]) == 1.0 + 2 * v                 # workgroup 1: its partial sum meets workgroup 0's as one term
    assert total([256, 768]) == 1.0 + 2 * v                 # (lane 0 of workgroup 1, k = 0 and 1)


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n", [1, 5, 1024, 1025, 4099, 262145, 525317])
def test_adv_stats_ref_against_fsum_and_whatever_absent_rows_hold(n, wide):
    """wide: magnitudes over 1e-8 .. 1e8, where the double adds do round (float32 values of like magnitude add exactly)."""
    g = torch.Generator().manual_seed(3 * n + 1)
    adv = torch.randn(n, generator=g) * 3 + 0.7
    adv = (adv * 10.0 ** (16 * torch.rand(n, generator=g) - 8) if wide else adv).numpy()
    absent = (torch.rand(n, generator=g) < 0.25).numpy()
    absent[n - 1] = False
    eps = 2.0 ** -52
    for present in (np.ones(n, dtype=np.bool_), ~absent):
        out = ppo_ref.adv_stats_ref(adv, present)
        terms = [float(x) for x in adv[present]]
        s0, s1 = math.fsum(terms), math.fsum(x * x for x in terms)                  # (x * x is exact: float32 values)
        assert out[2] == len(terms)
        assert abs(out[0] - s0) <= n * eps * math.fsum(abs(x) for x in terms)
        assert abs(out[1] - s1) <= n * eps * s1
    want = ppo_ref.adv_stats_ref(adv, ~absent)
    for junk in (np.float32("nan"), np.float32("inf"), np.float32(1e30), np.float32(-0.0)):
        holed = adv.copy()
        holed[absent] = junk
        assert ppo_ref.adv_stats_ref(holed, ~absent).tobytes() == want.tobytes()
    assert want.tobytes() == ppo_ref.adv_stats_ref(adv, ~absent).tobytes()
