"""Minibatch SGD in the PPO update (include/flowsim.h fs_ppo_minibatch; flow_amd/csrc/flowsim_learn.h perm_at), what can be
checked without a GPU:

* the permutation: fs_ppo_perm_host equals flow_amd.utils.device_ppo.epoch_permutation, both are bijections of [0, n), seeds
  and epochs give different permutations, and the shuffle is as good as the conditions below ask (sized so that a uniform
  shuffle passes with room: at n = 4096 at most 8 fixed points, mean |perm[i+1] - perm[i]| / n in [0.28, 0.39] where a
  uniform shuffle gives 1/3, and every minibatch of 128 holds 8 .. 56 rows of each quarter of the batch, where Binomial(128,
  1/4) has mean 32 and standard deviation 4.9);
* the new names are declared, bound and exported together, the ABI version stays, fs_ppo_minibatch has the C layout, the
  workspace is G (P + 4) + G words with G a function of (B, model) alone, and what must never launch is refused by name
  before a handle is looked at;
* train_vec.ppo_update(minibatch=B), the torch statement the kernels are held to, equals a loop written out here (the
  permutation, slices, the minibatch's own mean, one Adam step each, the KL sum of the last epoch), with the terms on and
  off; with B >= n and one epoch it is the full-batch update; a minibatch without a present row makes no step; with
  minibatch=None nothing new is called; the flag is off by default in both parsers."""
import ctypes
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
from test_device_ppo_loss_cpu import Prelude, ppo_model  # noqa: E402

NEW_NAMES = ("fs_ppo_perm_host", "fs_ppo_minibatch_workspace", "fs_ppo_minibatch_dev", "fs_ppo_mb_finish_dev")
SIZES = (1, 2, 3, 63, 64, 65, 259, 4096, 102400)


@pytest.fixture(scope="module")
def lib():
    from flow_amd import _lib, build
    build.build()
    return _lib.load()


def host_perm(lib, seed, epoch, n):
    out = np.full(n, -1, dtype=np.int64)
    assert lib.fs_ppo_perm_host(seed, epoch, n, out.ctypes.data) == 0
    return out


# ------------------------------------------------------------------------------------------------------ the permutation
@pytest.mark.parametrize("n", SIZES)
def test_host_permutation_equals_the_numpy_restatement_and_both_are_bijections(lib, n):
    from flow_amd.utils.device_ppo import epoch_permutation
    seen = []
    for seed, epoch in ((0, 0), (0, 1), (0, 2), (2 ** 40 + 12345, 0), (7, 2 ** 33 + 1)):
        p = epoch_permutation(seed, epoch, n)
        assert p.dtype == np.int64 and p.shape == (n,)
        assert np.array_equal(np.sort(p), np.arange(n))
        assert np.array_equal(host_perm(lib, seed, epoch, n), p)
        seen.append(p)
    if n >= 63:                                             # two epochs of one seed, two seeds of one epoch
        assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
        assert not np.array_equal(seen[0], seen[3]) and not np.array_equal(seen[0], seen[4])


def test_host_permutation_refuses_what_it_cannot_do(lib):
    out = np.zeros(4, dtype=np.int64)
    assert lib.fs_ppo_perm_host(0, 0, 0, out.ctypes.data) != 0 and b"fs_ppo_perm_host" in lib.fs_last_error()
    assert lib.fs_ppo_perm_host(0, 0, 2 ** 31, out.ctypes.data) != 0
    assert lib.fs_ppo_perm_host(0, 0, 4, None) != 0
    from flow_amd.utils.device_ppo import epoch_permutation
    with pytest.raises(ValueError):
        epoch_permutation(0, 0, 0)


@pytest.mark.parametrize("seed", [0, 7])
def test_shuffle_quality_at_4096(seed):
    from flow_amd.utils.device_ppo import epoch_permutation
    n, B = 4096, 128
    perms = [epoch_permutation(seed, e, n) for e in range(3)]
    for e, p in enumerate(perms):
        fixed = int((p == np.arange(n)).sum())
        walk = float(np.abs(np.diff(p)).mean()) / n
        quarters = (p // (n // 4)).reshape(n // B, B)
        counts = np.stack([(quarters == q).sum(1) for q in range(4)])
        print("seed %d epoch %d: %d fixed points, mean step %.4f, rows of a quarter per minibatch %d .. %d"
              % (seed, e, fixed, walk, counts.min(), counts.max()))
        assert fixed <= 8
        assert 0.28 <= walk <= 0.39
        assert counts.min() >= 8 and counts.max() <= 56
    assert int((perms[0] == perms[1]).sum()) <= 8 and int((perms[1] == perms[2]).sum()) <= 8


# ------------------------------------------------------------------------------------------------------------- the ABI
def test_header_binding_and_library_agree_on_the_new_names(lib):
    from flow_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flowsim.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fs_[a-z_0-9]+)\s*\(", text))
    for name in NEW_NAMES:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert hasattr(lib, name), name
    assert re.search(r"typedef struct fs_ppo_minibatch \{[^}]*\} fs_ppo_minibatch;", text)
    for name, val in (("FS_MB_STEP", 0), ("FS_MB_PARTIAL", 1), ("FS_MB_ACCUMULATE", 1), ("FS_MB_FIRST", 2), ("FS_MB_LAST", 4)):
        assert re.search(r"\b%s = %d\b" % (name, val), text) and getattr(_lib, name) == val, name
    assert lib.fs_abi_version() == 8 and _lib.FS_ABI_VERSION == 8               # additive: the ABI version stays


def test_fs_ppo_minibatch_has_the_c_layout(tmp_path):
    from flow_amd import _lib
    M = _lib.fs_ppo_minibatch
    fields = [n for n, _ in M._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "flowsim.h"\n'
                   'int main(void){printf("%zu' + " %zu" * len(fields) + '\\n", sizeof(fs_ppo_minibatch)'
                   + "".join(", offsetof(fs_ppo_minibatch, %s)" % f for f in fields) + "); return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert out == [ctypes.sizeof(M)] + [getattr(M, f).offset for f in fields]
    assert fields[:7] == ["struct_size", "mode", "flags", "reserved", "batch", "index", "seed"] and out[0] == 120


@pytest.mark.parametrize("D,A,layers", [(3, 1, 2), (25, 5, 2), (65, 13, 3), (141, 20, 2), (160, 32, 3)])
def test_minibatch_workspace_is_the_groups_of_a_batch_of_b_times_p_plus_5(lib, D, A, layers):
    P = ppo_ref.packed(D, A, layers)
    for B in (1, 5, 64, 65, 128, 1024, 4096, 102400, 2 ** 31 - 1):
        groups = int(lib.fs_ppo_workspace(ctypes.byref(ppo_model(D, A, layers)), B)) // (P + 2)
        assert groups == min(-(-B // 64), groups)
        assert int(lib.fs_ppo_minibatch_workspace(ctypes.byref(ppo_model(D, A, layers)), B)) == groups * (P + 4 + 1)
    for B in (0, -1, 2 ** 31):
        assert int(lib.fs_ppo_minibatch_workspace(ctypes.byref(ppo_model(D, A, layers)), B)) == 0
    assert int(lib.fs_ppo_minibatch_workspace(ctypes.byref(ppo_model(161, A, layers)), 128)) == 0
    assert int(lib.fs_ppo_minibatch_workspace(None, 128)) == 0


def mb_struct(**kw):
    from flow_amd import _lib
    M = _lib.fs_ppo_minibatch
    base = dict(struct_size=ctypes.sizeof(M), mode=_lib.FS_MB_STEP, flags=_lib.FS_MB_FIRST, batch=128, index=0, seed=0,
                epoch_dev=64, count_dev=64, weights_dev=64, m_dev=64, v_dev=64, state_dev=64, lr=3e-4, beta1=0.9, beta2=0.999,
                eps=1e-8)
    base.update(kw)
    return M(**base)


def test_what_must_never_launch_is_refused_by_name_before_a_handle_is_looked_at(lib):
    """No handle (NULL) and pointers that are never followed: every refusal below is made from the arguments alone."""
    from flow_amd import _lib
    loss = _lib.fs_ppo_loss(struct_size=ctypes.sizeof(_lib.fs_ppo_loss), clip=0.2, vf_coef=0.5)

    def call(model, mb, n=259):
        rc = lib.fs_ppo_minibatch_dev(None, ctypes.byref(model), ctypes.byref(loss), ctypes.byref(mb), n, 64, 64, 64, None,
                                      None, None, 64, 64, 64, 64, 64, 64, 1 << 30)
        return rc, lib.fs_last_error().decode()
    good = ppo_model(3, 1, 2)
    for bad, word in ((ppo_model(161, 1, 2), "obs_dim"), (ppo_model(3, 33, 2), "act_dim"), (ppo_model(3, 1, 4), "hidden layers"),
                      (ppo_model(3, 1, 2, width=16), "hidden"), (ppo_model(3, 1, 2, activation=1), "activation")):
        rc, msg = call(bad, mb_struct())
        assert rc == _lib.FS_ERR_UNSUPPORTED and "fs_ppo_model" in msg and word in msg, msg
    for kw, word in ((dict(batch=0), "batch"), (dict(batch=-5), "batch"), (dict(state_dev=None), "state_dev"),
                     (dict(m_dev=None), "m_dev"), (dict(v_dev=None), "v_dev"), (dict(weights_dev=None), "weights_dev"),
                     (dict(epoch_dev=None), "epoch_dev"), (dict(index=3), "index"), (dict(index=-1), "index"),
                     (dict(index=2 ** 62), "index"), (dict(index=2 ** 63 - 1, batch=2 ** 31 - 1), "index"),
                     (dict(mode=2), "mode"), (dict(flags=8), "flags"), (dict(struct_size=8), "struct_size"),
                     (dict(mode=_lib.FS_MB_PARTIAL, count_dev=None), "count_dev"),
                     (dict(flags=_lib.FS_MB_ACCUMULATE), "FS_MB_ACCUMULATE")):
        rc, msg = call(good, mb_struct(**kw))
        assert rc == _lib.FS_ERR_INVALID and "fs_ppo_minibatch" in msg and word in msg, (kw, msg)
    rc, msg = call(good, mb_struct(weights_dev=128))                               # not the buffer the model points into
    assert rc == _lib.FS_ERR_INVALID and "weights_dev" in msg
    rc, msg = call(good, mb_struct(), n=0)
    assert rc == _lib.FS_ERR_INVALID and "n must be" in msg
    # fs_ppo_mb_finish_dev: Adam's buffers by name
    for i, word in ((4, "m_dev"), (5, "v_dev"), (6, "state_dev")):
        args = [None, 10, 64, 64, 64, 64, 64, 64, 64, 0, 3e-4, 0.9, 0.999, 1e-8]
        args[i] = None
        assert lib.fs_ppo_mb_finish_dev(*args) == _lib.FS_ERR_INVALID and word in lib.fs_last_error().decode()


# --------------------------------------------------------------------------------- the torch statement: ppo_update(minibatch=)
K, R, D, A = 7, 37, 3, 2                                                            # n = 259
CLIP, KL_COEF, ENT, VF_CLIP, VF_COEF, LR = 0.2, 0.3, 0.01, 0.5, 0.7, 3e-3
TERMS_ON = dict(entropy_coef=ENT, vf_clip=VF_CLIP)


def problem(k=K, r=R, absent=None):
    import train_vec
    g = torch.Generator().manual_seed(19)
    torch.manual_seed(6)
    net = train_vec.GaussianPolicy(D, A).double()
    n = k * r
    obs = torch.randn(k + 1, r, D, generator=g, dtype=torch.float64)
    o = obs[:k].reshape(n, D)
    with torch.no_grad():
        mu, v = net.mu(o), net.value(o).squeeze(-1)
        std = net.log_std.exp()
        act = mu + std * torch.randn(n, A, generator=g, dtype=torch.float64)
        mean_old = mu + 0.3 * std * torch.randn(n, A, generator=g, dtype=torch.float64)
        ls_old = net.log_std.detach() + 0.1 * torch.randn(A, generator=g, dtype=torch.float64)
        val_old = v + 0.6 * torch.randn(n, generator=g, dtype=torch.float64)
        logp_old = net.logp_value(o, act)[0] + 0.3 * torch.randn(n, generator=g, dtype=torch.float64)
    if absent is not None:
        act[absent, 0] = float("nan")
    rew = torch.randn(k, r, generator=g, dtype=torch.float64)
    done = (torch.rand(k, r, generator=g) < 0.15).to(torch.uint8)
    return net, (obs, act.view(k, r, A), rew, done), (logp_old, val_old, mean_old, ls_old)


def written_out_loop(net, opt, shard, old, B, epochs, terms, seed, epoch0):
    """The semantics of minibatch=B from the issue's list alone (nothing of ppo_update's body): returns the mean KL that
    kl.adapt is to see."""
    import train_vec
    from flow_amd.utils.device_ppo import epoch_permutation
    obs, act, rew, done = shard
    logp_old, val_old, mean_old, ls_old = old
    k, r = rew.shape
    n = k * r
    o, a = obs[:k].reshape(n, -1), act.reshape(n, -1)
    present = ~torch.isnan(a).any(-1)
    a = torch.where(present[:, None], a, torch.zeros_like(a))
    with torch.no_grad():
        adv, ret = train_vec.gae(rew, val_old.view(k, r), done, net.value(obs[k]).squeeze(-1))
        adv, ret = adv.reshape(-1)[present], ret.reshape(-1)
        cnt = float(present.sum())
        mean = adv.sum() / cnt
        std = (((adv * adv).sum() - cnt * mean * mean) / (cnt - 1)).clamp_min(0).sqrt()
        adv_n = torch.zeros(n, dtype=torch.float64)
        adv_n[present] = ((adv - mean) / (std + 1e-8)).float().double()
    sum_kl = 0.0
    for e in range(epochs):
        perm = epoch_permutation(seed, epoch0 + e, n)
        sum_kl = 0.0
        for j in range(-(-n // B)):
            rows = [int(i) for i in perm[j * B:(j + 1) * B] if bool(present[int(i)])]
            if not rows:
                continue
            rows = torch.tensor(rows)
            mu, ls, v = net.mu(o[rows]), net.log_std, net.value(o[rows]).squeeze(-1)
            logp = (-0.5 * ((a[rows] - mu) / ls.exp()) ** 2 - ls - 0.9189385).sum(-1)
            ratio = (logp - logp_old[rows]).exp()
            per = -torch.minimum(ratio * adv_n[rows], ratio.clamp(1 - CLIP, 1 + CLIP) * adv_n[rows])
            kl = (ls - ls_old + ((2 * ls_old).exp() + (mean_old[rows] - mu) ** 2) / (2 * (2 * ls).exp()) - 0.5).sum(-1)
            if terms:
                v_c = val_old[rows] + (v - val_old[rows]).clamp(-VF_CLIP, VF_CLIP)
                per = per + VF_COEF * torch.maximum((v - ret[rows]) ** 2, (v_c - ret[rows]) ** 2)
                per = per + KL_COEF * kl - ENT * (ls + 0.5 * math.log(2 * math.pi * math.e)).sum()
                sum_kl += float(kl.detach().sum())
            else:
                per = per + VF_COEF * (v - ret[rows]) ** 2
            opt.zero_grad()
            (per.sum() / len(rows)).backward()
            opt.step()
    return sum_kl / cnt


def flat(net):
    return torch.cat([p.detach().reshape(-1) for p in net.parameters()])


@pytest.mark.parametrize("terms", [True, False])
@pytest.mark.parametrize("absent_rows", [False, True])
def test_ppo_update_with_minibatches_equals_the_loop_written_out_here(terms, absent_rows):
    import copy
    import train_vec
    absent = torch.rand(K * R, generator=torch.Generator().manual_seed(3)) < 0.2 if absent_rows else None
    net, shard, old = problem(absent=absent)
    w0 = flat(net).clone()
    twin = copy.deepcopy(net)
    kl = train_vec.AdaptiveKL(target=0.02, coef=KL_COEF) if terms else None
    train_vec.ppo_update(Prelude(net, *old), torch.optim.Adam(net.parameters(), lr=LR), [shard], epochs=2, clip=CLIP, kl=kl,
                         vf_coef=VF_COEF, minibatch=128, shuffle_seed=5, epoch0=3, **(TERMS_ON if terms else {}))
    mean_kl = written_out_loop(twin, torch.optim.Adam(twin.parameters(), lr=LR), shard, old, 128, 2, terms, 5, 3)
    moved = float((flat(twin) - w0).abs().max())
    err = float((flat(net) - flat(twin)).abs().max())
    print("terms %s, absent rows %s: moved %.3g, difference %.3g" % (terms, absent_rows, moved, err))
    assert moved > 4 * LR                       # (six Adam steps of at most LR each; two full-batch epochs move 2 LR at the most)
    assert err <= 1e-10 * moved
    if terms:
        assert abs(kl.mean_kl - mean_kl) <= 1e-12 * abs(mean_kl) and mean_kl > 0
        assert kl.coef in (KL_COEF * 1.5, KL_COEF, KL_COEF * 0.5)


@pytest.mark.parametrize("terms", [True, False])
def test_one_minibatch_of_everything_is_the_full_batch_update(terms):
    """B >= n, one epoch: the same mean over the same rows in a permuted order -- 1e-12 relative in float64."""
    import copy
    import train_vec
    net, shard, old = problem()
    twin = copy.deepcopy(net)
    kw = dict(epochs=1, clip=CLIP, vf_coef=VF_COEF, **(TERMS_ON if terms else {}))
    kls = [train_vec.AdaptiveKL(0.02, KL_COEF) if terms else None for _ in range(2)]
    train_vec.ppo_update(Prelude(net, *old), torch.optim.Adam(net.parameters(), lr=LR), [shard], kl=kls[0], minibatch=K * R + 41,
                         shuffle_seed=1, **kw)
    train_vec.ppo_update(Prelude(twin, *old), torch.optim.Adam(twin.parameters(), lr=LR), [shard], kl=kls[1], **kw)
    a, b = flat(net), flat(twin)
    assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())
    if terms:
        assert abs(kls[0].mean_kl - kls[1].mean_kl) <= 1e-12 * kls[1].mean_kl and kls[0].coef == kls[1].coef


def test_a_minibatch_without_a_present_row_makes_no_step():
    import train_vec
    from flow_amd.utils.device_ppo import epoch_permutation
    k, r, B = 4, 6, 6                                                               # n = 24: four minibatches of six
    perm = epoch_permutation(9, 0, k * r)
    absent = torch.zeros(k * r, dtype=torch.bool)
    absent[torch.as_tensor(perm[B:2 * B])] = True                                   # the whole of minibatch 1
    net, shard, old = problem(k, r, absent=absent)
    opt = torch.optim.Adam(net.parameters(), lr=LR)
    steps = []
    real = opt.step
    opt.step = lambda *a, **kw: (steps.append(1), real(*a, **kw))[1]
    train_vec.ppo_update(Prelude(net, *old), opt, [shard], epochs=1, clip=CLIP, minibatch=B, shuffle_seed=9)
    assert len(steps) == 3
    assert all(int(opt.state[p]["step"]) == 3 for p in net.parameters())
    assert bool(torch.isfinite(flat(net)).all())


def test_shards_of_unequal_size_and_a_learner_are_refused():
    import train_vec
    net, shard, old = problem()
    net2, shard2, _ = problem(4, 6)
    opt = torch.optim.Adam(net.parameters(), lr=LR)
    with pytest.raises(ValueError, match="same number of samples"):
        train_vec.ppo_update(net, opt, [shard, shard2], epochs=1, minibatch=128)
    with pytest.raises(NotImplementedError, match="--device_adam"):
        train_vec.ppo_update(net, opt, [shard], epochs=1, minibatch=128, learner=object())


def test_without_a_minibatch_size_nothing_new_is_called(monkeypatch):
    import copy
    import train_vec
    from flow_amd.utils import device_ppo

    def never(*a, **kw):
        raise AssertionError("the minibatch path was reached")
    monkeypatch.setattr(train_vec, "_ppo_epochs_minibatch", never)
    monkeypatch.setattr(device_ppo, "epoch_permutation", never)
    net, shard, old = problem()
    twin = copy.deepcopy(net)
    train_vec.ppo_update(Prelude(net, *old), torch.optim.Adam(net.parameters(), lr=LR), [shard], epochs=2, clip=CLIP)
    train_vec.ppo_update(Prelude(twin, *old), torch.optim.Adam(twin.parameters(), lr=LR), [shard], epochs=2, clip=CLIP,
                         minibatch=None, shuffle_seed=3, epoch0=9)
    assert torch.equal(flat(net), flat(twin))
    train_vec.ppo_update(Prelude(net, *old), torch.optim.Adam(net.parameters(), lr=LR), [shard], epochs=1, clip=CLIP,
                         kl=train_vec.AdaptiveKL(0.02, 0.2), **TERMS_ON)


def test_the_flag_is_off_by_default_in_both_parsers():
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
        assert seen["sgd_minibatch_size"] is None
        train_vec.main(["--iterations", "1", "--sgd_minibatch_size", "128", "--device_adam"])
        assert seen["sgd_minibatch_size"] == 128 and seen["device_adam"] is True
    finally:
        train_vec.train_on_device = real
    a = train.parse_args(["singleagent_ring"])
    assert a.sgd_minibatch_size is None and train.ppo_loss_settings(a)["sgd_minibatch_size"] is None
    b = train.parse_args(["singleagent_ring", "--reference_ppo"])
    kw = train.ppo_loss_settings(b)
    assert kw["sgd_minibatch_size"] is None and kw["epochs"] == 10                  # --reference_ppo keeps its meaning
    c = train.parse_args(["singleagent_ring", "--reference_ppo", "--sgd_minibatch_size", "128", "--device_adam"])
    assert train.ppo_loss_settings(c)["sgd_minibatch_size"] == 128 and c.device_adam is True
