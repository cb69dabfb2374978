"""The reference's PPO loss (KL penalty, clipped value loss, entropy; include/flowsim.h fs_ppo_loss), what can be checked
without a GPU: the five new names are declared, bound and exported together and the ABI version stays; the ctypes mirror of
fs_ppo_loss has the C layout; fs_ppo_loss_workspace is the workgroups of fs_ppo_workspace times P + 4; train_vec.ppo_update
with every term on computes the gradient of the loss as include/flowsim.h states it (written out again here, checked against
autograd and against central differences); the adaptive coefficient moves by RLlib's rule; the flags are off by default."""
import ctypes
import math
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import device_ppo_ref as ppo_ref  # noqa: E402

NEW_NAMES = ("fs_ppo_loss", "fs_ppo_eval_dist_dev", "fs_ppo_loss_workspace", "fs_ppo_grad_loss_dev", "fs_kl_adapt_dev")


@pytest.fixture(scope="module")
def lib():
    from flow_amd import _lib, build
    build.build()
    return _lib.load()


def test_header_binding_and_library_agree_on_the_new_names(lib):
    from flow_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flowsim.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fs_[a-z_0-9]+)\s*\(", text))
    for name in NEW_NAMES[1:]:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert hasattr(lib, name), name
    assert re.search(r"typedef struct fs_ppo_loss \{[^}]*\} fs_ppo_loss;", text)
    assert issubclass(_lib.fs_ppo_loss, ctypes.Structure)
    assert lib.fs_abi_version() == 8 and _lib.FS_ABI_VERSION == 8               # additive: the ABI version stays


def test_fs_ppo_loss_has_the_c_layout(tmp_path):
    from flow_amd import _lib
    fields = ["struct_size", "clip", "vf_coef", "vf_clip", "entropy_coef", "kl_state_dev"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "flowsim.h"\n'
                   'int main(void){printf("%zu' + " %zu" * len(fields) + '\\n", sizeof(fs_ppo_loss)'
                   + "".join(", offsetof(fs_ppo_loss, %s)" % f for f in fields) + "); return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    M = _lib.fs_ppo_loss
    assert [n for n, _ in M._fields_] == fields
    assert out == [ctypes.sizeof(M)] + [getattr(M, f).offset for f in fields]
    assert out[0] == 32 and out[-1] == 24


def ppo_model(D, A, layers, width=32, activation=0, value=64, struct_size=None):
    from flow_amd import _lib
    M = _lib.fs_ppo_model
    return M(struct_size=ctypes.sizeof(M) if struct_size is None else struct_size, obs_dim=D, act_dim=A, num_hidden=layers,
             hidden_width=width, activation=activation, policy_weights_dev=64, log_std_dev=64, value_weights_dev=value)


@pytest.mark.parametrize("D,A,layers", [(3, 1, 2), (25, 5, 2), (65, 13, 3), (141, 20, 2), (160, 32, 3)])
def test_loss_workspace_is_the_groups_of_the_plain_workspace_times_p_plus_4(lib, D, A, layers):
    P = ppo_ref.packed(D, A, layers)
    for n in (1, 64, 65, 259, 102400, 64 * 1024 + 1, 2 ** 31 - 1):
        plain = int(lib.fs_ppo_workspace(ctypes.byref(ppo_model(D, A, layers)), n))
        assert plain % (P + 2) == 0
        groups = plain // (P + 2)
        assert int(lib.fs_ppo_loss_workspace(ctypes.byref(ppo_model(D, A, layers)), n)) == groups * (P + 4)


def test_loss_workspace_is_zero_outside_the_range_of_n_and_outside_the_model_class(lib):
    def floats(model, n):
        return int(lib.fs_ppo_loss_workspace(ctypes.byref(model), n))
    good = ppo_model(3, 1, 2)
    assert floats(good, 1) == ppo_ref.packed(3, 1, 2) + 4 == 2439
    for n in (0, -1, 2 ** 31, 2 ** 40):
        assert floats(good, n) == 0, n
    for bad in (ppo_model(161, 1, 2), ppo_model(0, 1, 2), ppo_model(3, 33, 2), ppo_model(3, 0, 2), ppo_model(3, 1, 4),
                ppo_model(3, 1, 0), ppo_model(3, 1, 2, width=16), ppo_model(3, 1, 2, activation=1),
                ppo_model(3, 1, 2, value=None), ppo_model(3, 1, 2, struct_size=8)):
        assert floats(bad, 64) == 0
    assert int(lib.fs_ppo_loss_workspace(None, 64)) == 0


# ------------------------------------------------------------------------------------ ppo_update with every term on
class Prelude(object):
    """A policy for ppo_update whose no_grad pass is GIVEN -- (logp_old, val_old, mean_old, log_std_old) -- so that the old
    distribution differs from the new one in the first epoch already."""

    def __init__(self, net, logp_old, val_old, mean_old, log_std_old):
        self.net, self.old = net, (logp_old, val_old, mean_old, log_std_old)
        self.log_std = net.log_std

    def parameters(self):
        return self.net.parameters()

    def logp_value(self, obs, act):
        return self.net.logp_value(obs, act) if torch.is_grad_enabled() else self.old[:2]

    def logp_value_dist(self, obs, act):
        return self.net.logp_value_dist(obs, act) if torch.is_grad_enabled() else self.old

    def value(self, obs):
        return self.net.value(obs)


K, R, D, A = 6, 5, 3, 2
CLIP, KL_COEF, ENT, VF_CLIP, VF_COEF = 0.2, 0.3, 0.01, 0.5, 0.7


def fragment_problem(shift=0.3):
    import train_vec
    g = torch.Generator().manual_seed(11)
    torch.manual_seed(5)
    net = train_vec.GaussianPolicy(D, A).double()
    obs = torch.randn(K + 1, R, D, generator=g, dtype=torch.float64)
    o = obs[:K].reshape(K * R, D)
    with torch.no_grad():
        mu, v = net.mu(o), net.value(o).squeeze(-1)
        std = net.log_std.exp()
        act = mu + std * torch.randn(K * R, A, generator=g, dtype=torch.float64)
        mean_old = mu + shift * std * torch.randn(K * R, A, generator=g, dtype=torch.float64)
        ls_old = net.log_std.detach() + 0.1 * torch.randn(A, generator=g, dtype=torch.float64)
        val_old = v + 0.6 * torch.randn(K * R, generator=g, dtype=torch.float64)
        logp_old = net.logp_value(o, act)[0] + 0.3 * torch.randn(K * R, generator=g, dtype=torch.float64)
    rew = torch.randn(K, R, generator=g, dtype=torch.float64)
    done = (torch.rand(K, R, generator=g) < 0.15).to(torch.uint8)
    return net, (obs, act.view(K, R, A), rew, done), (logp_old, val_old, mean_old, ls_old)


def targets(net, shard, old):
    """(adv_n, ret) of the update: constants of the loss, taken once from the weights the update starts from."""
    import train_vec
    obs, act, rew, done = shard
    val_old = old[1]
    with torch.no_grad():
        adv, ret = train_vec.gae(rew, val_old.view(K, R), done, net.value(obs[K]).squeeze(-1))
        adv, ret, n = adv.reshape(-1), ret.reshape(-1), K * R
        mean = adv.sum() / n
        std = (((adv * adv).sum() - n * mean * mean) / (n - 1)).sqrt()
        adv_n = ((adv - mean) / (std + 1e-8)).float()       # (adv_n stays what it is: rounded to float32)
    return adv_n, ret


def written_out_loss(net, shard, old, fixed):
    """The loss of include/flowsim.h (fs_ppo_loss), from its formulas alone (nothing of ppo_update's body)."""
    obs, act, rew, done = shard
    logp_old, val_old, mean_old, ls_old = old
    (adv_n, ret), n = fixed, K * R
    o, a = obs[:K].reshape(K * R, D), act.reshape(K * R, A)
    mu, ls, v = net.mu(o), net.log_std, net.value(o).squeeze(-1)
    total = 0.0
    for i in range(n):                                      # sample by sample, column by column
        logp = sum(-0.5 * ((a[i, c] - mu[i, c]) / ls[c].exp()) ** 2 - ls[c] - 0.9189385 for c in range(A))
        ratio = (logp - logp_old[i]).exp()
        pg = torch.minimum(ratio * adv_n[i], ratio.clamp(1 - CLIP, 1 + CLIP) * adv_n[i])
        kl = sum(ls[c] - ls_old[c] + ((2 * ls_old[c]).exp() + (mean_old[i, c] - mu[i, c]) ** 2) / (2 * (2 * ls[c]).exp()) - 0.5
                 for c in range(A))
        ent = sum(ls[c] + 0.5 * math.log(2 * math.pi * math.e) for c in range(A))
        v_c = val_old[i] + (v[i] - val_old[i]).clamp(-VF_CLIP, VF_CLIP)
        vfl = torch.maximum((v[i] - ret[i]) ** 2, (v_c - ret[i]) ** 2)
        total = total + (-pg + KL_COEF * kl + VF_COEF * vfl - ENT * ent)
    return total / n


def test_ppo_update_with_every_term_on_has_the_gradient_of_the_written_out_loss():
    import train_vec
    net, shard, old = fragment_problem()
    # the conditions under which the comparison means something: both branches of the value clip and of the ratio clip taken
    with torch.no_grad():
        o = shard[0][:K].reshape(K * R, D)
        cut = ((net.value(o).squeeze(-1) - old[1]).abs() > VF_CLIP).double().mean()
    assert 0.1 <= float(cut) <= 0.9
    params = list(net.parameters())
    fixed = targets(net, shard, old)
    want = torch.autograd.grad(written_out_loss(net, shard, old, fixed), params)
    kl = train_vec.AdaptiveKL(target=0.02, coef=KL_COEF)
    train_vec.ppo_update(Prelude(net, *old), torch.optim.SGD(params, lr=0.0), [shard], epochs=1, clip=CLIP, kl=kl,
                         entropy_coef=ENT, vf_clip=VF_CLIP, vf_coef=VF_COEF)
    for p, w in zip(params, want):
        assert float(w.abs().max()) > 0
        assert float((p.grad - w).abs().max()) <= 1e-12 * float(w.abs().max()) + 1e-15
    # central differences of the written-out loss along random directions, 1e-6 relative
    g = torch.Generator().manual_seed(3)
    base = [p.detach().clone() for p in params]
    for _ in range(3):
        d = [torch.randn(p.shape, generator=g, dtype=torch.float64) for p in params]
        slope = sum(float((w * x).sum()) for w, x in zip(want, d))
        vals = []
        for sgn in (1.0, -1.0):
            with torch.no_grad():
                for p, b, x in zip(params, base, d):
                    p.copy_(b + sgn * 1e-5 * x)
                vals.append(float(written_out_loss(net, shard, old, fixed)))
        with torch.no_grad():
            for p, b in zip(params, base):
                p.copy_(b)
        fd = (vals[0] - vals[1]) / 2e-5
        assert abs(fd - slope) <= 1e-6 * abs(slope), (fd, slope)


def test_each_term_alone_changes_the_gradient_and_the_defaults_do_not():
    import train_vec
    net, shard, old = fragment_problem()
    params = list(net.parameters())

    def grads(**kw):
        train_vec.ppo_update(Prelude(net, *old), torch.optim.SGD(params, lr=0.0), [shard], epochs=1, clip=CLIP, **kw)
        return torch.cat([p.grad.reshape(-1).clone() for p in params])
    plain = grads()
    assert torch.equal(plain, grads(kl=None, entropy_coef=0.0, vf_clip=None, vf_coef=0.5))
    assert torch.equal(plain, grads(vf_clip=float("inf")))
    for kw in (dict(kl=train_vec.AdaptiveKL(0.02, 0.3)), dict(entropy_coef=0.01), dict(vf_clip=0.5), dict(vf_coef=1.0)):
        assert not torch.equal(plain, grads(**kw)), kw


# ------------------------------------------------------------------------------------------- the adaptation rule
@pytest.mark.parametrize("d,factor", [(0.3, 1.5), (0.2, 1.0), (0.1, 0.5)])
def test_the_coefficient_moves_by_rllibs_rule(d, factor):
    """A = 1, log_std unchanged, every old mean d standard deviations away: KL = d^2 / 2 per sample.  With the target
    0.02: 0.045 > 0.04 (x 1.5), 0.02 in between (unchanged), 0.005 < 0.01 (x 0.5)."""
    import train_vec
    torch.manual_seed(2)
    net = train_vec.GaussianPolicy(3, 1).double()
    g = torch.Generator().manual_seed(1)
    k, r = 4, 3
    obs = torch.randn(k + 1, r, 3, generator=g, dtype=torch.float64)
    o = obs[:k].reshape(k * r, 3)
    with torch.no_grad():
        mu, v = net.mu(o), net.value(o).squeeze(-1)
        act = mu + net.log_std.exp() * torch.randn(k * r, 1, generator=g, dtype=torch.float64)
        logp = net.logp_value(o, act)[0]
        old = (logp, v, mu + d * net.log_std.exp(), net.log_std.detach().clone())
    shard = (obs, act.view(k, r, 1), torch.randn(k, r, generator=g, dtype=torch.float64), torch.zeros(k, r, dtype=torch.uint8))
    kl = train_vec.AdaptiveKL(target=0.02, coef=0.2)
    train_vec.ppo_update(Prelude(net, *old), torch.optim.SGD(net.parameters(), lr=0.0), [shard], epochs=1, kl=kl)
    assert abs(kl.mean_kl - d * d / 2) <= 1e-12
    assert kl.coef == 0.2 * factor and kl.target == 0.02
    train_vec.ppo_update(Prelude(net, *old), torch.optim.SGD(net.parameters(), lr=0.0), [shard], epochs=2, kl=kl)
    assert kl.coef == 0.2 * factor * factor                  # once per update, not per epoch; and it keeps its state


def test_the_rule_itself_on_its_thresholds():
    import train_vec
    for mean_kl, factor in ((0.0401, 1.5), (0.04, 1.0), (0.01, 1.0), (0.0099, 0.5), (0.0, 0.5)):
        kl = train_vec.AdaptiveKL(target=0.02, coef=0.3)
        kl.adapt(mean_kl)
        assert kl.coef == 0.3 * factor and kl.mean_kl == mean_kl


# ------------------------------------------------------------------------------------------------------ the flags
def test_the_flags_are_off_by_default_in_both_parsers():
    import train
    import train_vec
    seen = {}

    def fake(flow_params, **kw):
        seen.clear()
        seen.update(kw)
        return []
    real, train_vec.train_on_device = train_vec.train_on_device, fake
    try:
        train_vec.main(["--iterations", "1"])
        assert seen["kl_target"] is None and seen["entropy_coeff"] == 0.0 and seen["vf_clip"] is None
        assert seen["kl_coeff"] == 0.2 and seen["epochs"] == 4
        train_vec.main(["--iterations", "1", "--kl_target", "0.02", "--kl_coeff", "0.3", "--entropy_coeff", "0.01",
                        "--vf_clip", "10"])
        assert (seen["kl_target"], seen["kl_coeff"], seen["entropy_coeff"], seen["vf_clip"]) == (0.02, 0.3, 0.01, 10.0)
    finally:
        train_vec.train_on_device = real
    a = train.parse_args(["singleagent_ring"])
    assert a.kl_target is None and a.vf_clip is None and a.entropy_coeff == 0.0 and a.kl_coeff == 0.2
    assert a.reference_ppo is False
    b = train.parse_args(["singleagent_ring", "--reference_ppo"])
    assert b.reference_ppo is True
    kw = train.ppo_loss_settings(b)
    assert (kw["kl_target"], kw["kl_coeff"], kw["vf_clip"], kw["epochs"]) == (0.02, 0.2, 10.0, 10)
    kw = train.ppo_loss_settings(a)
    assert kw["kl_target"] is None and kw["vf_clip"] is None and kw["entropy_coeff"] == 0.0 and kw["epochs"] == a.epochs
