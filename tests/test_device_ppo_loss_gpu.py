"""The reference's PPO loss on the device (flow_amd/csrc/flowsim_learn.h: k_ppo_eval with the old means, the full-loss form
of k_ppo_grad -- fs_last_kernel's "k_ppo_grad_loss" -- and k_kl_adapt; DeviceLearner.evaluate_dist / gradients_loss /
kl_adapt and update() with the terms on), on the float32 2-replica ring handle of tests/test_device_ppo_gpu.py.

* the packed gradient and the four loss sums {pg, vfl, KL, H} agree with torch float64 autograd of train_vec.ppo_update
  with the KL penalty, the clipped value loss and the entropy bonus on.  The measure is the project's: max|x - x64| /
  max|x64| per parameter tensor, against MARGIN = 10 times what torch FLOAT32 shows by the same measure on the shape's
  n = 259 inputs with the same terms on.  The inputs are those of tests/test_device_ppo_gpu.py ``case`` plus an old
  distribution and old values (``loss_case``); float64 decides, before anything runs on the GPU, that 10 % .. 60 % of the
  samples have their value gradient cut and that none lies within 1e-3 of a boundary of the value clip;
* evaluate_dist gives the bits of evaluate and the means within the forward bound; with every term off the full-loss form
  gives the bits of the plain one; two calls give the same bits, shards accumulate in call order, and nothing an absent
  row holds (NaN old means, old values, observations) reaches an output;
* k_kl_adapt equals the rule in Python floats bit for bit;
* update() with the terms on equals its stages, stays within MARGIN times torch float32 of float64 ppo_update, replays
  from a graph (kl_state included); with the defaults it never reaches the new kernels; train_on_device logs the KL."""
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
from helpers import ring_spec  # noqa: E402
from test_device_ppo_gpu import (CLIP, MARGIN, FixedPrelude, Net, case, learner_of, rel_err, split_grad, stats_of,  # noqa: E402
                                 yardstick)

pytestmark = pytest.mark.gpu

SHAPES = [(3, 1, 2), (65, 13, 3), (160, 32, 3)]
COUNTS = [5, 64, 259]
VF_CLIP, KL_COEF, ENT, VF_COEF, KL_TARGET = 0.5, 0.3, 0.01, 0.5, 0.02
GRID = 1.0 / 1024
HALF_LOG_2PIE = 0.5 * math.log(2.0 * math.pi * math.e)


@pytest.fixture(scope="module")
def sim():
    from flow_amd.sim import FlowSim
    s = FlowSim(ring_spec(R=2, N=5, bunching=0), "f32")
    yield s
    s.close()


class NetDist(Net):
    """Net with the method ppo_update's full loss asks of a policy."""

    def logp_value_dist(self, obs, act):
        mu = self.mu(obs)
        std = self.log_std.exp()
        logp = (-0.5 * ((act - mu) / std) ** 2 - self.log_std - 0.9189385).sum(-1)
        return logp, self.value(obs).squeeze(-1), mu, self.log_std


class FixedPreludeDist(FixedPrelude):
    """FixedPrelude that also hands over the old distribution: the no_grad pass is (logp_old, val_old, mean_old, log_std_old)."""

    def __init__(self, net, logp_old, val_old, mean_old, log_std_old):
        FixedPrelude.__init__(self, net, logp_old, val_old)
        self.mean_old, self.log_std_old = mean_old.to(self.dtype), log_std_old.to(self.dtype)
        self.log_std = net.log_std

    def logp_value_dist(self, obs, act):
        if torch.is_grad_enabled():
            return self.net.logp_value_dist(obs, act)
        return self.logp_old, self.val, self.mean_old, self.log_std_old


def loss_sums_of(net, obs, act, logp_old, mean_old, ls_old, val_old, adv_n, ret):
    """{sum pg, sum vfl, sum KL, sum H} by the formulas of include/flowsim.h (fs_ppo_loss) in the dtype of ``net``, and the
    sums of |term| beside them."""
    dt = net.log_std.dtype
    obs, act, logp_old, mean_old, ls_old, val_old, adv_n, ret = (t.to(dt) for t in (obs, act, logp_old, mean_old, ls_old,
                                                                                    val_old, adv_n, ret))
    with torch.no_grad():
        logp, v, mu, ls = net.logp_value_dist(obs, act)
        ratio = (logp - logp_old).exp()
        pg = torch.min(ratio * adv_n, ratio.clamp(1 - CLIP, 1 + CLIP) * adv_n)
        v_c = val_old + (v - val_old).clamp(-VF_CLIP, VF_CLIP)
        vfl = torch.max((v - ret) ** 2, (v_c - ret) ** 2)
        kl = (ls - ls_old + ((2 * ls_old).exp() + (mean_old - mu) ** 2) / (2 * (2 * ls).exp()) - 0.5).sum(-1)
        h = (ls + HALF_LOG_2PIE).sum().expand(obs.shape[0])
    terms = torch.stack([pg, vfl, kl, h])
    return terms.sum(1).double(), terms.double().abs().sum(1)


@functools.lru_cache(maxsize=None)
def loss_case(D, A, layers, n):
    """``case`` plus the old distribution and the old values, and ppo_update's float64 / float32 gradients with every term on
    (computed once on the CPU, never changed).  val_old lies on the 2^-10 grid like rew, so adv = rew - val_old and ret = rew
    are exact in float32: both precisions see the same advantages, statistics and returns."""
    import train_vec
    c = case(D, A, layers, n)
    # (the seed's offset: float64 alone picked it, so that every case, the five-sample ones included, meets the conditions
    # below -- cut shares of 0.16 .. 0.40, at most 0.4 % of the samples near a boundary)
    g = torch.Generator().manual_seed(31 * D + 7 * A + 3 * layers + 1000 * n + 25)
    net64 = NetDist(D, A, layers, seed=1).double()
    obs, act, rew = c["obs"], c["act"], c["ret"]
    with torch.no_grad():
        mu64, std64 = net64.mu(obs.double()), net64.log_std.exp()
    mean_old = (mu64 + 0.3 * std64 * torch.randn(n, A, generator=g, dtype=torch.float64)).float()
    ls_old = (net64.log_std.detach() + 0.1 * torch.randn(A, generator=g, dtype=torch.float64)).float()
    val_old = (torch.round((c["val64"] + 0.6 * torch.randn(n, generator=g, dtype=torch.float64)) / GRID) * GRID).float()
    v, r = c["val64"], rew.double()

    def bands(vo):
        dv = v - vo.double()
        e1, e2 = (v - r) ** 2, (vo.double() + dv.clamp(-VF_CLIP, VF_CLIP) - r) ** 2
        outside = dv.abs() > VF_CLIP
        near = ((dv.abs() - VF_CLIP).abs() < 1e-3) | (outside & ((e1 - e2).abs() < 1e-3))
        return near, outside & (e2 > e1)
    near, _ = bands(val_old)
    assert float(near.double().mean()) < 0.02, "the boundary shift moves %d of %d samples" % (int(near.sum()), n)
    val_old = torch.where(near, val_old + 51 * GRID, val_old)                       # 0.05, on the grid
    near, cut = bands(val_old)
    assert not bool(near.any())
    cut = float(cut.double().mean())
    assert 0.10 <= cut <= 0.60, "%.0f %% of the samples have their value gradient cut" % (100 * cut)
    adv = (rew - val_old).double()
    assert torch.equal(adv, rew.double() - val_old.double()) and torch.equal((rew - val_old) + val_old, rew)
    mean, std = stats_of(adv)
    adv_n = ((adv - mean) / (std + 1e-8)).float()
    done = torch.ones(1, n, dtype=torch.uint8)                                      # K = 1, every episode ends: adv = rew - val_old
    grads, sums, mags = {}, {}, {}
    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        m = NetDist(D, A, layers, seed=1).to(dt)
        shard = (torch.stack([obs, obs]).to(dt), act.to(dt).view(1, n, A), rew.to(dt).view(1, n), done)
        pi = FixedPreludeDist(m, c["logp_old"], val_old, mean_old, ls_old)
        train_vec.ppo_update(pi, torch.optim.SGD(m.parameters(), lr=0.0), [shard], epochs=1, clip=CLIP,
                             kl=train_vec.AdaptiveKL(KL_TARGET, KL_COEF), entropy_coef=ENT, vf_clip=VF_CLIP, vf_coef=VF_COEF)
        grads[name] = {k: p.grad.detach().double().clone() for k, p in m.tensors().items()}
        sums[name], mags[name] = loss_sums_of(m, obs, act, c["logp_old"], mean_old, ls_old, val_old, adv_n, rew)
    return dict(c, mean_old=mean_old, ls_old=ls_old, val_old=val_old, adv=adv, ret=rew, mean=mean, std=std, grads=grads,
                sums=sums, mags=mags, cut=cut)


def sums_err(x, c):
    """The largest of the four |x - x64| / sum|term64|: each sum's error over the size of what was added.  (The project's
    measure over the four as one tensor, max|x - x64| / max|x64|, lets sum H, the largest by far, hide the other three;
    the test asserts both.)"""
    return float(((x.double().cpu() - c["sums"]["f64"]).abs() / c["mags"]["f64"]).max())


@functools.lru_cache(maxsize=None)
def loss_yardstick(D, A, layers):
    """torch float32's own error on the shape's n = 259 inputs with the terms on, the largest over the parameter tensors:
    the bound of the gradient and of the loss sums is MARGIN times this."""
    c = loss_case(D, A, layers, 259)
    return max(rel_err(c["grads"]["f32"][k], c["grads"]["f64"][k]) for k in c["grads"]["f64"])


def msn_of(c, count=None):
    n = c["obs"].shape[0] if count is None else count
    return torch.tensor([float(c["mean"]), float(c["std"]), float(n)], dtype=torch.float64).cuda()


def run_loss(learner, c, msn=None, accumulate=False, terms=True, **over):
    t = {k: (over[k] if k in over else c[k]).cuda() for k in ("obs", "act", "logp_old", "adv", "ret", "mean_old", "ls_old",
                                                               "val_old")}
    learner.kl_state[0] = KL_COEF
    kw = dict(mean_old=t["mean_old"], log_std_old=t["ls_old"], val_old=t["val_old"], vf_clip=VF_CLIP, entropy_coef=ENT,
              kl=True) if terms else {}
    sums = learner.gradients_loss(t["obs"], t["act"], t["logp_old"], t["adv"], t["ret"], msn_of(c) if msn is None else msn,
                                  clip=CLIP, vf_coef=VF_COEF, accumulate=accumulate, **kw)
    torch.cuda.synchronize()
    return learner.grad.detach().cpu().clone(), sums.detach().cpu().clone()


# ----------------------------------------------------------------------------------------------------------- gradient
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("D,A,layers", SHAPES)
def test_gradient_and_loss_sums_agree_with_float64_ppo_update_with_the_terms_on(sim, D, A, layers, n):
    c = loss_case(D, A, layers, n)
    y_grad = loss_yardstick(D, A, layers)
    learner, net = learner_of(sim, c["net"])
    _, sums = run_loss(learner, c)
    assert sim.last_kernel == "k_ppo_grad_loss"
    got, want = split_grad(learner, net), c["grads"]["f64"]
    kern = {k: rel_err(got[k], want[k]) for k in want}
    f32 = max(rel_err(c["grads"]["f32"][k], want[k]) for k in want)
    worst = max(kern, key=kern.get)
    print("gradient, full loss (%d, %d, %d) n=%d: kernel %.3g (%s), torch float32 here %.3g, yardstick (n=259) %.3g, ratio %.2f"
          % (D, A, layers, n, kern[worst], worst, f32, y_grad, kern[worst] / y_grad))
    e_sums = sums_err(sums, c)
    print("loss sums (%d, %d, %d) n=%d: kernel %.3g, torch float32 here %.3g, yardstick (n=259) %.3g; cut %.0f %%; sums %s"
          % (D, A, layers, n, e_sums, sums_err(c["sums"]["f32"], c), y_grad, 100 * c["cut"], sums.tolist()))
    for k, e in kern.items():
        assert e <= MARGIN * y_grad, "%s: %.3g against 10 x %.3g" % (k, e, y_grad)
    assert e_sums <= MARGIN * y_grad, "%.3g against 10 x %.3g" % (e_sums, y_grad)
    assert rel_err(sums, c["sums"]["f64"]) <= MARGIN * y_grad                       # (the four as one tensor)
    assert float(sums[2]) > 0 and abs(float(sums[3]) - float(c["sums"]["f64"][3])) < 1e-3 * n * A


# ------------------------------------------------------------------------------------------------------ evaluate_dist
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("D,A,layers", SHAPES)
def test_evaluate_dist_gives_the_bits_of_evaluate_and_the_means(sim, D, A, layers, n):
    c = case(D, A, layers, n)
    learner, _ = learner_of(sim, c["net"])
    logp, val = learner.evaluate(c["obs"].cuda(), c["act"].cuda())
    logp2, val2, mean = learner.evaluate_dist(c["obs"].cuda(), c["act"].cuda())
    torch.cuda.synchronize()
    assert sim.last_kernel == "k_ppo_eval"
    assert torch.equal(logp, logp2) and torch.equal(val, val2)
    with torch.no_grad():
        mu64 = Net(D, A, layers, seed=1).double().mu(c["obs"].double())
    e, bound = rel_err(mean, mu64), MARGIN * yardstick(D, A, layers)[0]
    print("means (%d, %d, %d) n=%d: kernel %.3g, bound %.3g" % (D, A, layers, n, e, bound))
    assert mean.shape == (n, A) and e <= bound


# ------------------------------------------------------------------------------------------------------------ terms off
@pytest.mark.parametrize("absent_rows", [False, True])
def test_with_the_terms_off_the_full_loss_form_gives_the_bits_of_the_plain_one(sim, absent_rows):
    c = loss_case(65, 13, 3, 259)
    learner, _ = learner_of(sim, c["net"])
    act, count = c["act"].clone(), 259
    if absent_rows:
        absent = torch.rand(259, generator=torch.Generator().manual_seed(11)) < 0.3
        act[absent, 0] = float("nan")
        count = int((~absent).sum())
        assert 0 < count < 259
    msn = msn_of(c, count)
    t = [c["obs"].cuda(), act.cuda(), c["logp_old"].cuda(), c["adv"].cuda(), c["ret"].cuda()]
    loss = learner.gradients_n(*t, msn, clip=CLIP, vf_coef=VF_COEF)
    torch.cuda.synchronize()
    assert sim.last_kernel == "k_ppo_grad"
    g0, l0 = learner.grad.clone(), loss.clone()
    learner.grad.fill_(float("nan"))
    g1, s1 = run_loss(learner, c, msn=msn, terms=False, act=act)
    assert sim.last_kernel == "k_ppo_grad_loss"
    assert bool(torch.isfinite(g0).all()) and float(g0.abs().max()) > 0
    assert torch.equal(g1, g0.cpu()) and torch.equal(s1[:2], l0.cpu())
    assert float(s1[2]) == 0.0 and torch.equal(learner.loss, l0)                    # no KL term: no KL sum; loss left alone
    g2, _ = run_loss(learner, c, msn=msn, act=act)                                  # (and the terms do change the gradient)
    assert not torch.equal(g2, g1)


# ------------------------------------------------------------------------------------------ determinism, shards, absence
def test_the_same_bits_twice_shards_in_call_order_and_nothing_of_an_absent_row(sim):
    c1, c2 = loss_case(65, 13, 3, 259), loss_case(65, 13, 3, 64)
    learner, _ = learner_of(sim, c1["net"])
    msn = msn_of(c1, 323)
    a, sa = run_loss(learner, c1, msn=msn)
    learner.grad.fill_(float("nan"))
    learner.loss_sums.fill_(float("nan"))                                           # (accumulate=False overwrites)
    b, sb = run_loss(learner, c1, msn=msn)
    assert torch.equal(a, b) and torch.equal(sa, sb) and bool(torch.isfinite(a).all())
    s2, ss2 = run_loss(learner, c2, msn=msn)
    run_loss(learner, c1, msn=msn)
    acc, sacc = run_loss(learner, c2, msn=msn, accumulate=True)
    assert torch.equal(acc, (a.cuda() + s2.cuda()).cpu()) and torch.equal(sacc, (sa.cuda() + ss2.cuda()).cpu())
    # absent rows: the same bits whatever they hold, NaN old means, old values and observations included
    g = torch.Generator().manual_seed(5)
    absent = torch.rand(259, generator=g) < 0.2
    absent[64:128] = True                                                           # one whole 64-sample tile
    act = c1["act"].clone()
    act[absent, torch.randint(0, 13, (259,), generator=g)[absent]] = float("nan")
    msn = msn_of(c1, int((~absent).sum()))
    p, sp = run_loss(learner, c1, msn=msn, act=act)
    assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(sp).all()) and not torch.equal(p, a)
    nan = float("nan")
    held = {k: c1[k].clone() for k in ("obs", "logp_old", "adv", "ret", "mean_old", "val_old")}
    for k in held:
        held[k][absent] = nan
    held["mean_old"][absent.nonzero()[0]] = float("inf")
    act2 = act.clone()
    act2[absent] = nan
    q, sq = run_loss(learner, c1, msn=msn, act=act2, **held)
    assert torch.equal(p, q) and torch.equal(sp, sq)


# ------------------------------------------------------------------------------------------------------------ kl_adapt
def rule(coef, sum_kl, n, target):
    mean_kl = float(np.float32(sum_kl)) / float(n)
    if mean_kl > 2.0 * target:
        coef = coef * 1.5
    elif mean_kl < 0.5 * target:
        coef = coef * 0.5
    return coef, mean_kl


@pytest.mark.parametrize("sum_kl,n,factor", [(259 * 0.045, 259, 1.5), (259 * 0.02, 259, 1.0), (259 * 0.005, 259, 0.5),
                                              (0.041, 1, 1.5), (0.0, 1, 0.5)])
def test_kl_adapt_equals_the_rule_in_python_floats_bit_for_bit(sim, sum_kl, n, factor):
    learner, _ = learner_of(sim, Net(3, 1, 1, seed=0))
    sums = torch.tensor([1.0, 2.0, sum_kl, 3.0], dtype=torch.float32).cuda()
    msn = torch.tensor([0.5, 2.0, float(n)], dtype=torch.float64).cuda()
    learner.kl_state.copy_(torch.tensor([0.3, -1.0], dtype=torch.float64))
    coef, mean_kl = 0.3, None
    for _ in range(3):                                                              # a second and a third call advance it again
        learner.kl_adapt(KL_TARGET, msn, sums)
        torch.cuda.synchronize()
        assert sim.last_kernel == "k_kl_adapt"
        coef, mean_kl = rule(coef, sum_kl, n, KL_TARGET)
        assert learner.kl_state.tolist() == [coef, mean_kl]
    assert coef == {1.5: ((0.3 * 1.5) * 1.5) * 1.5, 1.0: 0.3, 0.5: 0.3 * 0.125}[factor]


# ------------------------------------------------------------------------------------------------------------ update()
TERMS = dict(kl_target=KL_TARGET, kl_coef_init=0.2, entropy_coef=ENT, vf_clip=VF_CLIP)


def fragment(D, A, K, R, seed, net):
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn(K + 1, R, D, generator=g)
    with torch.no_grad():
        mu = net.mu(obs[:K].reshape(K * R, D))
        act = (mu + net.log_std.exp() * torch.randn(K * R, A, generator=g)).view(K, R, A)
    rew = torch.randn(K, R, generator=g)
    done = (torch.rand(K, R, generator=g) < 0.1).to(torch.uint8)
    done[K // 2, 0] = 2
    return obs, act, rew, done


def on_gpu(shard):
    return tuple(t.cuda() for t in shard)


def test_update_with_the_terms_on_equals_its_stages_called_one_by_one(sim):
    D, A, layers, K, R = 65, 13, 3, 8, 16
    net = Net(D, A, layers, seed=2)
    shards = [fragment(D, A, K, R, 1, net), fragment(D, A, 5, 7, 2, net)]
    shards[1][1][2, 3, 1] = float("nan")                                            # an absent agent in the second shard
    whole, _ = learner_of(sim, net)
    whole.adopt_parameters()
    out = whole.update([on_gpu(s) for s in shards], epochs=4, **TERMS)
    torch.cuda.synchronize()
    assert sim.last_kernel == "k_kl_adapt" and out is whole.loss_sums
    steps, _ = learner_of(sim, net)
    steps.adopt_parameters()
    steps.kl_state[0] = 0.2
    prepared, stats = [], torch.zeros(3, dtype=torch.float64).cuda()
    for j, (obs, act, rew, done) in enumerate(on_gpu(s) for s in shards):
        k, r = rew.shape
        o, a = obs[:k].reshape(k * r, D), act.reshape(k * r, A)
        logp, val, mean_old = steps.evaluate_dist(o, a)
        ls_old = steps.weights[steps.n_policy:steps.n_policy + A].clone()
        last = steps.evaluate(obs[k], None)[1]
        adv, ret = steps.gae(rew, val.view(k, r), last, done)
        adv64, _ = steps.adv_stats(adv, a, accumulate=j > 0, stats=stats)
        prepared.append((o, a, logp, adv64, ret.reshape(-1), mean_old, ls_old, val))
    msn = steps.adv_finish(stats)
    for _ in range(4):
        for j, (o, a, logp, adv64, ret, mean_old, ls_old, val) in enumerate(prepared):
            steps.gradients_loss(o, a, logp, adv64, ret, msn, mean_old=mean_old, log_std_old=ls_old, val_old=val, clip=0.2,
                                 vf_coef=0.5, vf_clip=VF_CLIP, entropy_coef=ENT, kl=True, accumulate=j > 0)
        steps.adam_step(lr=3e-4, betas=(0.9, 0.999), eps=1e-8)
    steps.kl_adapt(KL_TARGET, msn)
    torch.cuda.synchronize()
    assert msn[2].item() == 8 * 16 + 5 * 7 - 1
    for name in ("weights", "grad", "loss_sums", "m", "v", "state", "kl_state"):
        assert torch.equal(getattr(whole, name), getattr(steps, name)), name
    assert whole.state[0].item() == 4 and whole.kl_state[0].item() in (0.1, 0.2, 0.2 * 1.5)
    assert whole.kl_state[1].item() == float(whole.loss_sums[2].item()) / msn[2].item()


def flat(net):
    return torch.cat([p.detach().reshape(-1) for p in net.tensors().values()]).double().numpy()


@functools.lru_cache(maxsize=None)
def update_problem(D, A, layers):
    """A fragment of 8 x 16 samples and train_vec.ppo_update's result on it after 4 epochs with the terms on, by torch on
    the CPU in float64 and in float32 (computed once); the float64 coefficient after the update beside them."""
    import train_vec
    K, R = 8, 16
    net = NetDist(D, A, layers, seed=3)
    shard = fragment(D, A, K, R, 17 * D + A, net)
    w0, out, kls = flat(net), {}, {}
    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        m = copy.deepcopy(net).to(dt)
        sh = (shard[0].to(dt), shard[1].to(dt), shard[2].to(dt), shard[3])
        kls[name] = train_vec.AdaptiveKL(KL_TARGET, 0.2)
        train_vec.ppo_update(m, torch.optim.Adam(m.parameters(), lr=ref.LR), [sh], epochs=4, clip=0.2, kl=kls[name],
                             entropy_coef=ENT, vf_clip=VF_CLIP, vf_coef=0.5)
        out[name] = flat(m)
    return net, shard, w0, out["f64"], ref.displacement_error(out["f32"], out["f64"], w0), kls["f64"]


@pytest.mark.parametrize("D,A,layers", [(3, 1, 2), (65, 13, 3)])
def test_update_with_the_terms_on_stays_within_float32_torch_of_float64_ppo_update(sim, D, A, layers):
    net, shard, w0, w64, err32, kl64 = update_problem(D, A, layers)
    learner, _ = learner_of(sim, net)
    learner.adopt_parameters()
    learner.update([on_gpu(shard)], epochs=4, clip=0.2, lr=ref.LR, **TERMS)
    torch.cuda.synchronize()
    err = ref.displacement_error(learner.weights.cpu().numpy(), w64, w0)
    coef, mean_kl = learner.kl_state.tolist()
    print("update, full loss (%d, %d, %d): kernels %.3g, torch float32 %.3g (ratio %.2f); mean KL %.3g (float64 %.3g), "
          "coefficient %.3g (float64 %.3g)" % (D, A, layers, err, err32, err / err32, mean_kl, kl64.mean_kl, coef, kl64.coef))
    assert err <= MARGIN * err32
    assert coef == kl64.coef                                                        # the same branch of the rule


def test_update_with_the_terms_on_replays_from_a_graph_with_the_bits_of_eager_calls(sim):
    D, A, layers = 3, 1, 2
    net, shard, _, _, _, _ = update_problem(D, A, layers)
    learner, _ = learner_of(sim, net)
    learner.adopt_parameters()
    shard = on_gpu(shard)
    start = learner.weights.clone()

    def rewind():
        learner.weights.copy_(start)
        learner.m.zero_()
        learner.v.zero_()
        learner.state.copy_(torch.tensor(ref.fresh_state(), dtype=torch.float64))
        learner.kl_state.copy_(torch.tensor([0.2, 0.0], dtype=torch.float64))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        learner.update([shard], epochs=4, **TERMS)          # the eager warm-up, on the capture stream: the handle is bound
        side.synchronize()                                  # to it (fs_set_stream synchronises) and every buffer exists
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        learner.update([shard], epochs=4, **TERMS)
    torch.cuda.synchronize()
    rewind()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert learner.state[0].item() == 8
    names = ("weights", "m", "v", "state", "grad", "loss_sums", "kl_state")
    replayed = {k: getattr(learner, k).clone() for k in names}
    assert not torch.equal(replayed["weights"], start)
    assert replayed["kl_state"][0].item() != 0.2            # the replays advanced the coefficient
    rewind()
    learner.update([shard], epochs=4, **TERMS)
    learner.update([shard], epochs=4, **TERMS)
    torch.cuda.synchronize()
    assert learner.state[0].item() == 8
    for k, want in replayed.items():
        assert torch.equal(getattr(learner, k), want), k


NEW = ("evaluate_dist", "_eval_dist", "gradients_loss", "_grad_loss", "kl_adapt")
STAGES = ("_adv_stats", "_grad_n", "adam_step")


def watch(monkeypatch, calls, kernels=None):
    from flow_amd.utils.device_ppo import DeviceLearner

    def counted(name):
        real = getattr(DeviceLearner, name)

        def fn(self, *a, **kw):
            calls.append(name)
            out = real(self, *a, **kw)
            if kernels is not None:
                kernels.append(self.sim.last_kernel)
            return out
        monkeypatch.setattr(DeviceLearner, name, fn)
    for name in NEW + STAGES:
        counted(name)


def test_update_with_the_defaults_never_reaches_the_new_kernels(sim, monkeypatch):
    net, shard, _, _, _, _ = update_problem(3, 1, 2)
    learner, _ = learner_of(sim, net)
    learner.adopt_parameters()
    calls, kernels = [], []
    watch(monkeypatch, calls, kernels)
    kl0 = learner.kl_state.clone()
    out = learner.update([on_gpu(shard)], epochs=4)
    torch.cuda.synchronize()
    assert sim.last_kernel == "k_adam" and out is learner.loss
    assert calls == ["_adv_stats"] + ["_grad_n", "adam_step"] * 4
    assert kernels == ["k_adv_stats"] + ["k_ppo_grad", "k_adam"] * 4
    assert torch.equal(learner.kl_state, kl0) and not bool(learner.loss_sums.any())


# ------------------------------------------------------------------------------------------------------------ trainer
@pytest.mark.parametrize("kl_target,path", [(KL_TARGET, "device_adam"), (None, "device_adam"), (KL_TARGET, "device_update"),
                                            (KL_TARGET, "torch")])
def test_train_on_device_with_and_without_the_kl_target(monkeypatch, kl_target, path):
    """device_adam: update() on the device; device_update: ppo_update(learner=, kl=) -- the kernels' gradient, the rule in
    Python; torch: ppo_update(kl=) alone."""
    import train_vec
    calls, lines = [], []
    watch(monkeypatch, calls)
    hist = train_vec.train_on_device(train_vec.ring_flow_params(20), replicas=8, fragment=10, iterations=2,
                                     device_adam=path == "device_adam", device_update=path != "torch", kl_target=kl_target,
                                     log=lambda s: lines.append(s))
    assert len(hist) == 2 and all(np.isfinite(h) for h in hist)
    its = [s for s in lines if s.startswith("iteration")]
    assert len(its) == 2
    if kl_target is None:
        assert not any(name in calls for name in NEW) and calls.count("_grad_n") == 2 * 4
        assert not any("KL" in s or "kl_coeff" in s for s in its)
    else:
        if path == "device_adam":
            assert calls.count("_eval_dist") == 2 and calls.count("_grad_loss") == 2 * 4 and calls.count("kl_adapt") == 2
        elif path == "device_update":
            assert calls.count("evaluate_dist") == 2 and calls.count("gradients_loss") == 2 * 4 and "kl_adapt" not in calls
        else:
            assert calls == []
        assert "_grad_n" not in calls
        for s in its:
            kl, coef = float(s.split("KL")[1].split()[0]), float(s.split("kl_coeff")[1].split()[0])
            assert np.isfinite(kl) and round(coef, 6) in (0.3, 0.2, 0.1, 0.45, 0.15, 0.05)    # 0.2 after one or two steps of the rule
