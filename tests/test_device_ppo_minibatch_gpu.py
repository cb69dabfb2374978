"""Minibatch SGD in the device PPO update (flow_amd/csrc/flowsim_learn.h: the minibatch form of k_ppo_grad -- fs_last_kernel's
"k_ppo_minibatch" -- and k_mb_finish; DeviceLearner.minibatch_step / mb_finish / update(minibatch=)), on the float32 2-replica
ring handle of tests/test_device_ppo_gpu.py and the inputs of tests/test_device_ppo_loss_gpu.py (``loss_case``, n = 259).

* the gradient one step leaves in ``grad`` agrees with torch float64 autograd of the same minibatch's mean loss -- rows
  ``epoch_permutation(seed, epoch, n)[kB : (k + 1)B]``, divisor the minibatch's own count -- for B below a tile, exactly a
  tile, two tiles and four tiles with a ragged end, at the first and at the last (short) minibatch, terms on and off.  The
  bound is the project's: MARGIN = 10 times the shape's torch-float32 yardstick;
* Adam in the tail equals device_adam_ref.adam_ref applied to the kernel's own gradient, bit for bit, three steps running;
* the fused step gives the bits of the chain PARTIAL + fs_ppo_mb_finish_dev, two calls give the same bits, and two shards
  through PARTIAL, PARTIAL(accumulate), finish stay within the bound of the torch statement over both;
* absent rows: the divisor is the present count and nothing of an absent row reaches an output; a minibatch without a present
  row leaves weights, m, v, state as they are and adds exact zeros to the loss sums;
* the loss sums of a whole epoch are the float64 sums; kl_adapt after a minibatch update is the rule in Python floats;
* update(minibatch=128, epochs=2) equals its stages, stays within float32 torch of float64 ppo_update(minibatch=128), replays
  from a graph with the bits of eager calls (the epoch counter is device state); the defaults never reach the new kernels;
  train_on_device(sgd_minibatch_size=128) trains."""
import copy
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "examples"))
sys.path.insert(0, HERE)

import device_adam_ref as ref  # noqa: E402
from device_adam_ref import adam_ref  # noqa: E402
from helpers import ring_spec  # noqa: E402
from test_device_ppo_gpu import MARGIN, Net, case, learner_of, rel_err, split_grad, yardstick  # noqa: E402,F401
from test_device_ppo_loss_gpu import (ENT, KL_COEF, KL_TARGET, VF_CLIP, VF_COEF, NetDist, fragment, loss_case,  # noqa: E402
                                      loss_yardstick, msn_of, on_gpu, rule, sums_err)

pytestmark = pytest.mark.gpu

SHAPES = [(3, 1, 2), (65, 13, 3), (160, 32, 3)]
N, CLIP, SEED = 259, 0.2, 11
HALF_LOG_2PIE = 0.5 * math.log(2.0 * math.pi * math.e)
STATE_NAMES = ("weights", "m", "v", "state")


@pytest.fixture(scope="module")
def sim():
    from flow_amd.sim import FlowSim
    s = FlowSim(ring_spec(R=2, N=5, bunching=0), "f32")
    yield s
    s.close()


def perm_of(epoch, n=N, seed=SEED):
    from flow_amd.utils.device_ppo import epoch_permutation
    return epoch_permutation(seed, epoch, n)


def reference(shards, rows, terms, D, A, layers):
    """torch float64 on the CPU: the mean loss of the rows ``rows`` of every shard in ``shards`` (dicts like loss_case's)
    over THEIR present count, its gradient per parameter tensor, the four raw sums and the sums of |term|."""
    net = NetDist(D, A, layers, seed=1).double()
    total, count, sums, mags = 0.0, 0, torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.float64)
    for c in shards:
        idx = torch.as_tensor(rows)
        act = c["act"][idx]
        present = ~torch.isnan(act).any(-1)
        idx = idx[present]
        if idx.numel() == 0:
            continue
        obs, act = c["obs"][idx].double(), c["act"][idx].double()
        adv_n = ((c["adv"] - c["mean"]) / (c["std"] + 1e-8)).float().double()[idx]
        ret, logp_old = c["ret"][idx].double(), c["logp_old"][idx].double()
        logp, v, mu, ls = net.logp_value_dist(obs, act)
        ratio = (logp - logp_old).exp()
        pg = torch.min(ratio * adv_n, ratio.clamp(1 - CLIP, 1 + CLIP) * adv_n)
        vfl = (v - ret) ** 2
        kl = torch.zeros_like(pg)
        h = (ls + HALF_LOG_2PIE).sum().expand(idx.numel())
        per = -pg
        if terms:
            vo, mo, lso = c["val_old"][idx].double(), c["mean_old"][idx].double(), c["ls_old"].double()
            vfl = torch.max(vfl, (vo + (v - vo).clamp(-VF_CLIP, VF_CLIP) - ret) ** 2)
            kl = (ls - lso + ((2 * lso).exp() + (mo - mu) ** 2) / (2 * (2 * ls).exp()) - 0.5).sum(-1)
            per = per + KL_COEF * kl - ENT * h
        per = per + VF_COEF * vfl
        total = total + per.sum()
        count += int(idx.numel())
        terms4 = torch.stack([pg, vfl, kl, h]).detach()
        sums, mags = sums + terms4.sum(1), mags + terms4.abs().sum(1)
    (total / count).backward()
    return {k: p.grad.detach().clone() for k, p in net.tensors().items()}, sums, mags, count


def fresh(learner, w0):
    learner._adam_buffers()
    learner.weights.copy_(w0)
    learner.m.zero_()
    learner.v.zero_()
    learner.state.copy_(torch.tensor(ref.fresh_state(), dtype=torch.float64))


def step(learner, c, B, k, terms=True, epoch=None, **kw):
    """One minibatch_step on the inputs of ``c`` (overridable); returns (grad, loss_sums) on the CPU."""
    over = {name: kw.pop(name) for name in list(kw) if name in ("obs", "act", "logp_old", "adv", "ret", "mean_old", "ls_old",
                                                                 "val_old")}
    t = {name: (over[name] if name in over else c[name]).cuda() for name in ("obs", "act", "logp_old", "adv", "ret", "mean_old",
                                                                           "ls_old", "val_old")}
    if epoch is not None:
        learner.mb_epoch.fill_(epoch)
    learner.kl_state[0] = KL_COEF
    on = dict(mean_old=t["mean_old"], log_std_old=t["ls_old"], val_old=t["val_old"], vf_clip=VF_CLIP, entropy_coef=ENT,
              kl=True) if terms else {}
    on.update(kw)
    sums = learner.minibatch_step(t["obs"], t["act"], t["logp_old"], t["adv"], t["ret"], msn_of(c), B, k, shuffle_seed=SEED,
                                  clip=CLIP, vf_coef=VF_COEF, **on)
    torch.cuda.synchronize()
    return learner.grad.detach().cpu().clone(), sums.detach().cpu().clone()


def snapshot(learner, names=STATE_NAMES + ("grad", "loss_sums")):
    return {k: getattr(learner, k).detach().cpu().clone() for k in names}


# ------------------------------------------------------------------------------------------------- gradient of one step
@pytest.mark.parametrize("terms", [True, False])
@pytest.mark.parametrize("D,A,layers", SHAPES)
def test_gradient_of_one_step_agrees_with_float64_autograd_of_the_minibatch_mean(sim, D, A, layers, terms):
    c = loss_case(D, A, layers, N)
    y = loss_yardstick(D, A, layers) if terms else yardstick(D, A, layers)[1]
    learner, net = learner_of(sim, c["net"])
    w0 = learner.weights.clone()
    perm = perm_of(2)
    for B in (5, 64, 128, 200):
        last = -(-N // B) - 1
        for k in (0, last):
            rows = perm[k * B:(k + 1) * B]
            assert len(rows) == (B if k == 0 else N - last * B) and (k == 0 or len(rows) < B)
            fresh(learner, w0)
            learner.loss_sums.fill_(float("nan"))
            _, sums = step(learner, c, B, k, terms=terms, epoch=2, first=True, last=False)
            assert sim.last_kernel == "k_ppo_minibatch"
            want, sums64, mags64, count = reference([c], rows, terms, D, A, layers)
            got = split_grad(learner, net)
            kern = {name: rel_err(got[name], want[name]) for name in want}
            worst = max(kern, key=kern.get)
            e_sums = float(((sums.double() - sums64).abs() / mags64.clamp_min(1e-300))[:2 if not terms else 4].max())
            print("minibatch gradient (%d, %d, %d) terms %s B=%d k=%d (%d rows): kernel %.3g (%s), yardstick (n=259) %.3g, "
                  "ratio %.2f; loss sums %.3g" % (D, A, layers, terms, B, k, count, kern[worst], worst, y, kern[worst] / y, e_sums))
            for name, e in kern.items():
                assert e <= MARGIN * y, "%s: %.3g against 10 x %.3g (B=%d k=%d)" % (name, e, y, B, k)
            assert e_sums <= MARGIN * y
            assert int(learner.mb_epoch.item()) == 2 and learner.state[0].item() == 1.0


# ----------------------------------------------------------------------------------------------------- Adam in the tail
@pytest.mark.parametrize("D,A,layers", SHAPES)
def test_adam_in_the_tail_equals_adam_ref_on_the_kernels_own_gradient_bit_for_bit(sim, D, A, layers):
    c = loss_case(D, A, layers, N)
    learner, _ = learner_of(sim, c["net"])
    fresh(learner, learner.weights.clone())
    w, m, v, st = (getattr(learner, k).cpu().numpy().copy() for k in STATE_NAMES)
    for k in range(3):                                                              # B = 100: minibatches of 100, 100, 59
        g, _ = step(learner, c, 100, k, epoch=None)
        w, m, v, st = adam_ref(w, g.numpy(), m, v, st, lr=3e-4)
        for name, want in zip(STATE_NAMES, (w, m, v, st)):
            assert np.array_equal(getattr(learner, name).cpu().numpy(), want), (name, k)
    assert st[0] == 3.0 and int(learner.mb_epoch.item()) == 1                       # k = 2 was the epoch's last minibatch


# ---------------------------------------------------------------------------------------------------- fused equals chain
@pytest.mark.parametrize("D,A,layers", SHAPES)
def test_the_fused_step_gives_the_bits_of_partial_plus_finish_and_of_a_second_call(sim, D, A, layers):
    c = loss_case(D, A, layers, N)
    learner, _ = learner_of(sim, c["net"])
    w0 = learner.weights.clone()
    for B, k in ((128, 0), (128, 2), (200, 1)):
        out = []
        for mode in ("step", "step", "chain"):
            fresh(learner, w0)
            learner.grad.fill_(float("nan"))
            learner.loss_sums.fill_(float("nan"))
            learner.mb_count.fill_(float("nan"))
            step(learner, c, B, k, epoch=4, first=True, partial=mode == "chain")
            if mode == "chain":
                assert learner.mb_count.item() == len(perm_of(4)[k * B:(k + 1) * B])
                assert int(learner.mb_epoch.item()) == 4                            # (PARTIAL never advances the epoch)
                learner.mb_finish(last=k == -(-N // B) - 1)
                torch.cuda.synchronize()
                assert sim.last_kernel == "k_mb_finish"
            out.append(snapshot(learner, STATE_NAMES + ("grad", "loss_sums", "mb_epoch")))
        for name in out[0]:
            assert torch.equal(out[0][name], out[1][name]), (name, "second call")
            assert torch.equal(out[0][name], out[2][name]), (name, "chain")
        assert bool(torch.isfinite(out[0]["grad"]).all()) and not torch.equal(out[0]["weights"], w0.cpu())
        assert int(out[0]["mb_epoch"].item()) == (5 if k == -(-N // B) - 1 else 4)


def test_two_shards_through_partial_partial_finish_stay_within_the_bound_of_the_torch_statement(sim):
    D, A, layers, B, k = 65, 13, 3, 128, 1
    c1 = loss_case(D, A, layers, N)
    flip = torch.arange(N - 1, -1, -1)
    c2 = dict(c1, **{name: c1[name][flip] for name in ("obs", "act", "logp_old", "adv", "ret", "mean_old", "val_old")})
    learner, net = learner_of(sim, c1["net"])
    fresh(learner, learner.weights.clone())
    w0 = learner.weights.clone()
    _, s1 = step(learner, c1, B, k, epoch=1, partial=True, first=True)
    g1 = learner.grad.clone()
    _, s2 = step(learner, c2, B, k, epoch=1, partial=True, accumulate=True, first=True)
    assert learner.mb_count.item() == 256.0 and torch.equal(learner.weights, w0)
    alone, _ = step(learner, c2, B, k, epoch=1, partial=True, first=True)           # the second shard alone: the sum in call order
    assert learner.mb_count.item() == 128.0
    step(learner, c1, B, k, epoch=1, partial=True, first=True)
    raw, s12 = step(learner, c2, B, k, epoch=1, partial=True, accumulate=True, first=True)
    assert torch.equal(raw, (g1 + alone.cuda()).cpu()) and torch.equal(s12, s2)
    learner.mb_finish()
    torch.cuda.synchronize()
    want, _, _, count = reference([c1, c2], perm_of(1)[k * B:(k + 1) * B], True, D, A, layers)
    assert count == 256 and learner.state[0].item() == 1.0
    got, y = split_grad(learner, net), loss_yardstick(D, A, layers)
    kern = {name: rel_err(got[name], want[name]) for name in want}
    print("two shards: kernel %.3g, yardstick %.3g, ratio %.2f" % (max(kern.values()), y, max(kern.values()) / y))
    assert max(kern.values()) <= MARGIN * y


# ----------------------------------------------------------------------------------------------------------- absent rows
def test_absent_rows_the_present_count_divides_and_nothing_of_them_reaches_an_output(sim):
    D, A, layers, B, k = 65, 13, 3, 128, 1
    c = loss_case(D, A, layers, N)
    learner, net = learner_of(sim, c["net"])
    w0 = learner.weights.clone()
    rows = perm_of(3)[k * B:(k + 1) * B]
    g = torch.Generator().manual_seed(8)
    gone = torch.as_tensor(rows)[torch.rand(B, generator=g) < 0.3]                  # rows of THIS minibatch, found through the permutation
    assert 20 <= gone.numel() <= 60
    act = c["act"].clone()
    act[gone, torch.randint(0, A, (gone.numel(),), generator=g)] = float("nan")
    fresh(learner, w0)
    step(learner, c, B, k, epoch=3, act=act, first=True)
    a = snapshot(learner)
    want, sums64, mags64, count = reference([dict(c, act=act)], rows, True, D, A, layers)
    assert count == B - gone.numel()
    got, y = split_grad(learner, net), loss_yardstick(D, A, layers)
    kern = {name: rel_err(got[name], want[name]) for name in want}
    print("absent rows: %d of %d present; kernel %.3g, yardstick %.3g, ratio %.2f" % (count, B, max(kern.values()), y,
                                                                                       max(kern.values()) / y))
    assert max(kern.values()) <= MARGIN * y
    assert float(((a["loss_sums"].double() - sums64).abs() / mags64).max()) <= MARGIN * y
    held = {name: c[name].clone() for name in ("obs", "mean_old", "val_old", "logp_old", "adv", "ret")}
    for name in held:
        held[name][gone] = float("nan")
    held["mean_old"][gone[0]] = float("inf")
    held["val_old"][gone[1]] = float("-inf")
    act2 = act.clone()
    act2[gone] = float("nan")
    fresh(learner, w0)
    step(learner, c, B, k, epoch=3, act=act2, first=True, **held)
    b = snapshot(learner)
    for name in a:
        assert torch.equal(a[name], b[name]) and bool(torch.isfinite(a[name]).all()), name


def test_a_minibatch_without_a_present_row_makes_no_step_and_adds_exact_zeros(sim):
    D, A, layers, B, k = 65, 13, 3, 64, 2
    c = loss_case(D, A, layers, N)
    learner, _ = learner_of(sim, c["net"])
    fresh(learner, learner.weights.clone())
    step(learner, c, B, 0, epoch=6)                                                 # a real step first: m, v, state are not trivial
    before = snapshot(learner, STATE_NAMES + ("loss_sums",))
    act = c["act"].clone()
    act[torch.as_tensor(perm_of(6)[k * B:(k + 1) * B]), 0] = float("nan")
    for partial in (False, True):
        grad, sums = step(learner, c, B, k, act=act, partial=partial, first=False)
        if partial:
            assert learner.mb_count.item() == 0.0
            learner.mb_finish()
            torch.cuda.synchronize()
        after = snapshot(learner, STATE_NAMES + ("loss_sums",))
        for name in before:
            assert torch.equal(before[name], after[name]), (name, partial)
        assert not bool(grad.any())
    assert before["state"][0].item() == 1.0 and int(learner.mb_epoch.item()) == 6


# ------------------------------------------------------------------------------------------------------ loss sums and KL
@pytest.mark.parametrize("D,A,layers", SHAPES)
def test_loss_sums_of_a_whole_epoch_are_the_float64_sums(sim, D, A, layers):
    c = loss_case(D, A, layers, N)
    learner, _ = learner_of(sim, c["net"])
    w0 = learner.weights.clone()
    fresh(learner, w0)
    learner.loss_sums.fill_(float("nan"))
    for k in range(3):                                                              # lr = 0: the weights stay where float64 has them
        _, sums = step(learner, c, 128, k, epoch=9, lr=0.0)
    assert torch.equal(learner.weights, w0) and int(learner.mb_epoch.item()) == 10 and learner.state[0].item() == 3.0
    e, y = sums_err(sums, c), loss_yardstick(D, A, layers)
    print("epoch loss sums (%d, %d, %d): kernel %.3g, yardstick %.3g; sums %s" % (D, A, layers, e, y, sums.tolist()))
    assert e <= MARGIN * y
    assert rel_err(sums, c["sums"]["f64"]) <= MARGIN * y


TERMS = dict(kl_target=KL_TARGET, kl_coef_init=0.2, entropy_coef=ENT, vf_clip=VF_CLIP)
K_, R_ = 8, 37                                                                      # 296 samples: minibatches of 128, 128, 40


@functools.lru_cache(maxsize=None)
def update_problem(D, A, layers):
    """A fragment of 8 x 37 samples and train_vec.ppo_update(minibatch=128) on it after 2 epochs with the terms on, by torch
    on the CPU in float64 and in float32 (computed once), from the same weights and with the same permutations as the
    code under test."""
    import train_vec
    net = NetDist(D, A, layers, seed=3)
    shard = fragment(D, A, K_, R_, 17 * D + A, net)
    w0, out, kls = flat(net), {}, {}
    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        m = copy.deepcopy(net).to(dt)
        sh = (shard[0].to(dt), shard[1].to(dt), shard[2].to(dt), shard[3])
        kls[name] = train_vec.AdaptiveKL(KL_TARGET, 0.2)
        train_vec.ppo_update(m, torch.optim.Adam(m.parameters(), lr=ref.LR), [sh], epochs=2, clip=0.2, kl=kls[name],
                             entropy_coef=ENT, vf_clip=VF_CLIP, vf_coef=0.5, minibatch=128, shuffle_seed=SEED, epoch0=0)
        out[name] = flat(m)
    return net, shard, w0, out["f64"], ref.displacement_error(out["f32"], out["f64"], w0), kls["f64"]


def flat(net):
    return torch.cat([p.detach().reshape(-1) for p in net.tensors().values()]).double().numpy()


def test_kl_adapt_after_a_minibatch_update_equals_the_rule_in_python_floats(sim):
    net, shard, _, _, _, _ = update_problem(3, 1, 2)
    learner, _ = learner_of(sim, net)
    learner.adopt_parameters()
    coef = 0.2
    for _ in range(2):                                                              # the second update starts from the adapted value
        sums = learner.update([on_gpu(shard)], epochs=2, minibatch=128, shuffle_seed=SEED, **TERMS)
        torch.cuda.synchronize()
        assert sim.last_kernel == "k_kl_adapt" and sums is learner.loss_sums
        n = learner._mean_std_n[2].item()
        assert n == K_ * R_
        coef, mean_kl = rule(coef, sums[2].item(), n, KL_TARGET)
        assert learner.kl_state.tolist() == [coef, mean_kl]
    assert int(learner.mb_epoch.item()) == 4 and learner.state[0].item() == 12.0
    # no epoch: no step, and no adaptation either (no KL was seen) -- ppo_update's rule
    kept = {k: getattr(learner, k).clone() for k in STATE_NAMES + ("kl_state", "loss_sums", "mb_epoch")}
    learner.update([on_gpu(shard)], epochs=0, minibatch=128, shuffle_seed=SEED, **TERMS)
    torch.cuda.synchronize()
    assert sim.last_kernel != "k_kl_adapt"
    for k, want in kept.items():
        assert torch.equal(getattr(learner, k), want), k


# ------------------------------------------------------------------------------------------------------------ update()
@pytest.mark.parametrize("D,A,layers", [(3, 1, 2), (65, 13, 3)])
def test_update_with_minibatches_equals_its_stages_called_one_by_one(sim, D, A, layers):
    net, shard, _, _, _, _ = update_problem(D, A, layers)
    shard = list(shard)
    shard[1] = shard[1].clone()
    shard[1][2, 3, 0] = float("nan")                                                # an absent agent
    whole, _ = learner_of(sim, net)
    whole.adopt_parameters()
    out = whole.update([on_gpu(shard)], epochs=2, minibatch=128, shuffle_seed=SEED, **TERMS)
    torch.cuda.synchronize()
    assert sim.last_kernel == "k_kl_adapt" and out is whole.loss_sums
    steps, _ = learner_of(sim, net)
    steps.adopt_parameters()
    steps.kl_state[0] = 0.2
    obs, act, rew, done = on_gpu(shard)
    k, r = rew.shape
    n = k * r
    o, a = obs[:k].reshape(n, D), act.reshape(n, A)
    logp, val, mean_old = steps.evaluate_dist(o, a)
    ls_old = steps.weights[steps.n_policy:steps.n_policy + A].clone()
    last = steps.evaluate(obs[k], None)[1]
    adv, ret = steps.gae(rew, val.view(k, r), last, done)
    adv64, stats = steps.adv_stats(adv, a)
    msn = steps.adv_finish(stats)
    for _ in range(2):
        for j in range(3):
            steps.minibatch_step(o, a, logp, adv64, ret.reshape(-1), msn, 128, j, shuffle_seed=SEED, mean_old=mean_old,
                                 log_std_old=ls_old, val_old=val, clip=0.2, vf_coef=0.5, vf_clip=VF_CLIP, entropy_coef=ENT,
                                 kl=True)
            assert sim.last_kernel == "k_ppo_minibatch"
    steps.kl_adapt(KL_TARGET, msn)
    torch.cuda.synchronize()
    assert msn[2].item() == n - 1
    for name in STATE_NAMES + ("grad", "loss_sums", "kl_state", "mb_epoch"):
        assert torch.equal(getattr(whole, name), getattr(steps, name)), name
    assert whole.state[0].item() == 6 and int(whole.mb_epoch.item()) == 2


@pytest.mark.parametrize("D,A,layers", [(3, 1, 2), (65, 13, 3)])
def test_update_with_minibatches_stays_within_float32_torch_of_float64_ppo_update(sim, D, A, layers):
    net, shard, w0, w64, err32, kl64 = update_problem(D, A, layers)
    learner, _ = learner_of(sim, net)
    learner.adopt_parameters()
    learner.update([on_gpu(shard)], epochs=2, clip=0.2, lr=ref.LR, minibatch=128, shuffle_seed=SEED, **TERMS)
    torch.cuda.synchronize()
    err = ref.displacement_error(learner.weights.cpu().numpy(), w64, w0)
    coef, mean_kl = learner.kl_state.tolist()
    print("update, minibatches (%d, %d, %d): kernels %.3g, torch float32 %.3g (ratio %.2f); mean KL %.3g (float64 %.3g), "
          "coefficient %.3g (float64 %.3g)" % (D, A, layers, err, err32, err / err32, mean_kl, kl64.mean_kl, coef, kl64.coef))
    assert err <= MARGIN * err32
    assert coef == kl64.coef                                                        # the same branch of the rule


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("D,A,layers", [(3, 1, 2), (65, 13, 3)])
def test_update_with_minibatches_replays_from_a_graph_with_the_bits_of_eager_calls(sim, D, A, layers, fused):
    """``fused=True``: every step is the one launch whose tail resets the ticket and advances the epoch counter inside the
    kernel; ``fused=False``: the chain, where k_mb_finish advances it."""
    net, shard, _, _, _, _ = update_problem(D, A, layers)
    learner, _ = learner_of(sim, net)
    learner.adopt_parameters()
    shard = on_gpu(shard)
    start = learner.weights.clone()
    kw = dict(epochs=2, minibatch=128, shuffle_seed=SEED, fused=fused, **TERMS)

    def rewind():
        learner.weights.copy_(start)
        learner.m.zero_()
        learner.v.zero_()
        learner.state.copy_(torch.tensor(ref.fresh_state(), dtype=torch.float64))
        learner.kl_state.copy_(torch.tensor([0.2, 0.0], dtype=torch.float64))
        learner.mb_epoch.zero_()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        learner.update([shard], **kw)                       # the eager warm-up, on the capture stream: the handle is bound
        side.synchronize()                                  # to it and every buffer, the ticket included, exists
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        learner.update([shard], **kw)
    torch.cuda.synchronize()
    # an update at a larger batch size in between: the graph keeps the workspace it was captured with
    held = learner._mb_workspace(128).data_ptr()
    learner.update([shard], epochs=1, minibatch=4096, shuffle_seed=SEED, fused=fused, **TERMS)
    torch.cuda.synchronize()
    assert sim.last_kernel == "k_kl_adapt"
    assert learner._work_mb.numel() > learner._mb_workspace(128).numel() and learner._mb_workspace(128).data_ptr() == held
    rewind()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert learner.state[0].item() == 12 and int(learner.mb_epoch.item()) == 4
    names = STATE_NAMES + ("grad", "loss_sums", "kl_state", "mb_epoch")
    replayed = {k: getattr(learner, k).clone() for k in names}
    assert not torch.equal(replayed["weights"], start)
    # (the graph was captured with the counter at 2: a permutation fixed at capture time would have drawn epochs 2, 3 twice,
    # where the eager updates below draw 0, 1 and then 2, 3)
    rewind()
    learner.update([shard], **kw)
    learner.update([shard], **kw)
    torch.cuda.synchronize()
    for k, want in replayed.items():
        assert torch.equal(getattr(learner, k), want), k


NEW = ("minibatch_step", "_mb_step", "mb_finish", "_mb_workspace")


def test_update_with_the_defaults_never_reaches_the_new_kernels(sim, monkeypatch):
    from flow_amd.utils.device_ppo import DeviceLearner
    net, shard, _, _, _, _ = update_problem(3, 1, 2)
    learner, _ = learner_of(sim, net)
    learner.adopt_parameters()
    calls, kernels = [], []
    for name in NEW + ("_adv_stats", "_grad_n", "adam_step"):
        def counted(name=name, real=getattr(DeviceLearner, name)):
            def fn(self, *a, **kw):
                calls.append(name)
                out = real(self, *a, **kw)
                kernels.append(self.sim.last_kernel)
                return out
            return fn
        monkeypatch.setattr(DeviceLearner, name, counted())
    epoch0 = learner.mb_epoch.clone()
    out = learner.update([on_gpu(shard)], epochs=4)
    torch.cuda.synchronize()
    assert sim.last_kernel == "k_adam" and out is learner.loss
    assert calls == ["_adv_stats"] + ["_grad_n", "adam_step"] * 4
    assert kernels == ["k_adv_stats"] + ["k_ppo_grad", "k_adam"] * 4
    assert torch.equal(learner.mb_epoch, epoch0) and learner._work_mb is None
    calls.clear()
    learner.update([on_gpu(shard)], epochs=1, minibatch=128)                        # (and with a size it does reach them)
    torch.cuda.synchronize()
    assert calls.count("_mb_step") == 3 and "_grad_n" not in calls and "adam_step" not in calls
    fused = DeviceLearner.minibatch_fused(128, 3, 1, 2)                             # (the rule: one launch per step, or two)
    assert calls.count("mb_finish") == (0 if fused else 3)
    assert sim.last_kernel == ("k_ppo_minibatch" if fused else "k_mb_finish")
    calls.clear()
    learner.update([on_gpu(shard)], epochs=1, minibatch=128, fused=True)
    torch.cuda.synchronize()
    assert calls.count("_mb_step") == 3 and "mb_finish" not in calls and sim.last_kernel == "k_ppo_minibatch"
    with pytest.raises(ValueError, match="same number of samples"):
        learner.update([on_gpu(shard), on_gpu(fragment(3, 1, 5, 7, 2, net))], epochs=1, minibatch=128)


# ------------------------------------------------------------------------------------------------------------ trainer
def test_train_on_device_with_minibatches_on_the_device(monkeypatch):
    import train_vec
    from flow_amd.utils.device_ppo import DeviceLearner
    calls, lines = [], []
    real = DeviceLearner._mb_step

    def counted(self, *a, **kw):
        calls.append(self.sim.last_kernel)
        return real(self, *a, **kw)
    monkeypatch.setattr(DeviceLearner, "_mb_step", counted)
    hist = train_vec.train_on_device(train_vec.ring_flow_params(40), replicas=8, fragment=40, iterations=2, epochs=2,
                                     device_adam=True, device_update=True, sgd_minibatch_size=128,
                                     log=lambda s: lines.append(s))
    assert len(hist) == 2 and all(np.isfinite(h) for h in hist)
    assert len(calls) == 2 * 2 * 3                                                  # 320 samples: minibatches of 128, 128, 64
    assert len([s for s in lines if s.startswith("iteration")]) == 2
