"""MergePOEnv's fused policy kernel k_merge_policy (flow_amd/csrc/flowsim_queue.h; fs_last_kernel "k_merge_policy<PO>") and
the Python side of its action-vector head, without a GPU.

* code generation (hipcc -S): the kernel exists with and without noise, keeps nothing in scratch memory and stays within a
  workgroup's 64 KB of LDS.  Together with tests/test_queue_codegen.py -- which holds every k_merge_queue instantiation to
  its figures and allows none with both POLICY and PO -- this shows that the new kernel is a kernel of its own and that
  the step forms and the multi-agent policy forms are what they were;
* DevicePolicy(act_dim=A): the packed buffer is [W..., b...] per layer in order, the output layer's rows included, and
  reference() splits means and log stds the way RLlib's DiagGaussian does (the first A outputs, the last A outputs)."""
import re

import numpy as np
import pytest

from flow_amd import build


@pytest.fixture(scope="module")
def queue_asm(tmp_path_factory):
    try:
        build.find_hipcc()
    except RuntimeError:
        pytest.skip("hipcc not available")
    files = build.device_asm(str(tmp_path_factory.mktemp("asm")), names=["queue_f32"])
    with open(files["queue_f32"]) as f:
        return f.read()


def kernels(asm, family):
    """{mangled name: {num_vgpr, num_agpr, private_seg_size, lds_bytes}} of the kernels whose name starts with `family`."""
    out = {}
    for name, key, val in re.findall(r"\.set (_ZN2fs\d+%s\w+)\.(num_vgpr|num_agpr|private_seg_size), (\d+)" % family, asm):
        out.setdefault(name, {})[key] = int(val)
    lds = None
    for line in asm.splitlines():                       # the metadata lists a kernel's LDS size before its name
        m = re.match(r"\s*\.group_segment_fixed_size:\s*(\d+)", line)
        if m:
            lds = int(m.group(1))
            continue
        m = re.match(r"\s*\.name:\s+(\S+)\s*$", line)
        if m and m.group(1) in out:
            out[m.group(1)]["lds_bytes"] = lds
    return out


def test_fused_kernel_exists_in_both_noise_forms_without_scratch(queue_asm):
    table = kernels(queue_asm, "k_merge_policy")
    forms = {}
    for name, res in table.items():
        m = re.match(r"_ZN2fs14k_merge_policyILb([01])EEEv", name)
        assert m, name
        forms[int(m.group(1))] = res
    assert sorted(forms) == [0, 1], sorted(table)
    for noise, res in forms.items():
        print("k_merge_policy<NOISE=%d>: %s" % (noise, res))
        assert res["private_seg_size"] == 0, (noise, res)
        assert 0 < res["lds_bytes"] <= 64 * 1024, (noise, res)
        assert res["num_vgpr"] + res["num_agpr"] <= 512, (noise, res)


def test_eager_kernel_exists_without_scratch(queue_asm):
    table = kernels(queue_asm, "k_policy_act_vec")
    assert len(table) == 1, sorted(table)
    res = next(iter(table.values()))
    assert res["private_seg_size"] == 0 and res["lds_bytes"] <= 64 * 1024, res


def make_policy(act_dim, num_hidden, free):
    import torch
    from flow_amd.utils.device_policy import DevicePolicy
    g = torch.Generator().manual_seed(act_dim + 10 * num_hidden)
    dims = [5 * act_dim] + [32] * num_hidden
    hidden = [torch.nn.Linear(dims[i], dims[i + 1]) for i in range(num_hidden)]
    head = torch.nn.Linear(32, act_dim if free else 2 * act_dim)
    with torch.no_grad():
        for l in hidden + [head]:
            l.weight.copy_(torch.randn(l.weight.shape, generator=g) * 0.3)
            l.bias.copy_(torch.randn(l.bias.shape, generator=g) * 0.2)
    ls = torch.nn.Parameter(torch.linspace(-1.0, -0.2, act_dim)) if free else None
    return DevicePolicy(hidden, head, log_std=ls, seed=5, act_dim=act_dim), hidden, head, ls


@pytest.mark.parametrize("num_hidden,free", [(1, False), (2, True), (3, False)])
def test_device_policy_packs_an_action_vector_head(num_hidden, free):
    import torch
    A = 5
    pol, hidden, head, ls = make_policy(A, num_hidden, free)
    assert pol.act_dim == A and pol.struct.obs_dim == 5 * A and pol.struct.num_hidden == num_hidden
    # the documented order: per layer W [out][in] row-major, then b [out]; the output layer last
    want = []
    for l in hidden + [head]:
        want += [l.weight.detach().numpy().reshape(-1), l.bias.detach().numpy().reshape(-1)]
    want = np.concatenate(want)
    np.testing.assert_array_equal(pol.buf.numpy(), want)
    n_out = A if free else 2 * A
    np.testing.assert_array_equal(pol.buf.numpy()[-n_out:], head.bias.detach().numpy())
    np.testing.assert_array_equal(pol.buf.numpy()[-n_out - 32 * n_out:-n_out].reshape(n_out, 32), head.weight.detach().numpy())
    if free:
        assert pol.struct.log_std_dev == pol.ls.data_ptr() and pol.ls.numel() == A
        np.testing.assert_array_equal(pol.ls.numpy(), ls.detach().numpy())
    else:
        assert not pol.struct.log_std_dev
    # reference(): a forward pass written out by hand
    obs = torch.rand((7, 3, 5 * A), generator=torch.Generator().manual_seed(1)) * 2 - 1
    with torch.no_grad():
        mu, log_std = pol.reference(obs)
    h = obs.numpy().astype(np.float64)
    for l in hidden:
        h = np.tanh(h @ l.weight.detach().numpy().astype(np.float64).T + l.bias.detach().numpy())
    out = h @ head.weight.detach().numpy().astype(np.float64).T + head.bias.detach().numpy()
    assert tuple(mu.shape) == (7, 3, A) and tuple(log_std.shape) == (7, 3, A)
    np.testing.assert_allclose(mu.numpy(), out[..., :A], atol=1e-5, rtol=0)
    if free:
        np.testing.assert_array_equal(log_std.detach().numpy(), np.broadcast_to(ls.detach().numpy(), (7, 3, A)))
    else:
        np.testing.assert_allclose(log_std.numpy(), out[..., A:], atol=1e-5, rtol=0)


def test_device_policy_checks_the_head_width_and_keeps_its_default():
    import torch
    from flow_amd.utils.device_policy import DevicePolicy
    hidden = [torch.nn.Linear(25, 32)]
    with pytest.raises(NotImplementedError):
        DevicePolicy(hidden, torch.nn.Linear(32, 5))                       # (act_dim 1: two outputs)
    with pytest.raises(NotImplementedError):
        DevicePolicy(hidden, torch.nn.Linear(32, 7), act_dim=5)
    with pytest.raises(NotImplementedError):
        DevicePolicy(hidden, torch.nn.Linear(32, 5), log_std=torch.zeros(1), act_dim=5)
    one = DevicePolicy([torch.nn.Linear(3, 32)], torch.nn.Linear(32, 2))
    mu, ls = one.reference(torch.zeros(4, 3))
    assert one.act_dim == 1 and tuple(mu.shape) == (4,) and tuple(ls.shape) == (4,)
