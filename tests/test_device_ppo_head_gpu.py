"""The head of 2 act_dim outputs (log stds from the network) in the device PPO update: the NET_LS forms of k_ppo_eval and
k_ppo_grad (flow_amd/csrc/flowsim_learn.h; fs_last_kernel's "k_ppo_eval_ls", "k_ppo_grad_ls", "k_ppo_grad_loss_ls",
"k_ppo_minibatch_ls") through DeviceLearner(net_log_std=True), on the float32 2-replica ring handle of
tests/test_device_ppo_gpu.py.

* the degenerate head, bit for bit: log-std rows with zero weights and bias b are the free form with log_std = b, so every
  output the two forms share must hold the same values -- logp, val, the gradient of the trunk, of the mean rows and of the
  value network, the loss sums, and the log-std bias gradient against the free form's log_std gradient;
* a general head (random log-std rows, ls in about [-1.5, 0.5]) against torch float64 autograd of train_vec.ppo_update with
  the terms on and off, by the project's measure (max|x - x64| / max|x64| per parameter tensor; each loss sum's error over
  the sum of |term|) and bound: MARGIN = 10 times what torch FLOAT32 shows on the shape's n = 259 inputs with this head.
  Float64 decides on the CPU, before anything runs on the GPU, that 10 % .. 60 % of the samples are clipped by the
  surrogate and by the value clip and that none lies within 1e-3 of a boundary;
* two calls give the same bits, shards accumulate in call order, nothing an absent row holds reaches an output;
* above the workgroup cap the gradient is the stated composition of its tile sums, bit for bit, and stays within MARGIN
  times torch float32's error on the same inputs;
* a minibatch step in one launch gives the bits of PARTIAL + mb_finish; update() equals its stages, stays within the bound
  of float64 ppo_update(minibatch=128), replays from a graph; without the keyword no "_ls" kernel is ever launched;
* a DevicePolicy sharing the learner's buffer acts with the bits of a synced copy; train_on_device(net_log_std=True)."""
import copy
import ctypes
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
import device_ppo_ref as ppo_ref  # noqa: E402
from helpers import ring_spec  # noqa: E402
from test_device_ppo_gpu import CLIP, MARGIN, Net, case, learner_of, rel_err, split_grad, stats_of, yardstick  # noqa: E402,F401
from test_device_ppo_loss_gpu import (ENT, GRID, KL_COEF, KL_TARGET, VF_CLIP, VF_COEF, loss_case, msn_of, on_gpu,  # noqa: E402
                                      run_loss)

pytestmark = pytest.mark.gpu

SHAPES = [(3, 1, 2), (65, 13, 3), (160, 32, 3)]
COUNTS = [5, 64, 259]
HALF_LOG_2PIE = 0.5 * math.log(2.0 * math.pi * math.e)
TILE, SEED = 64, 11
CAP_3_1_2 = 768                                              # tests/test_device_ppo_head_cpu.py derives and pins it
SCALE_N = TILE * (2 * CAP_3_1_2 + 1) + 5
TERMS = dict(kl_target=KL_TARGET, kl_coef_init=0.2, entropy_coef=ENT, vf_clip=VF_CLIP)


@pytest.fixture(scope="module")
def sim():
    from flow_amd.sim import FlowSim
    s = FlowSim(ring_spec(R=2, N=5, bunching=0), "f32")
    yield s
    s.close()


class NetLS(Net):
    """Net whose policy head has 2 A rows, the means (Net's own head) and then the log stds, and no free log_std:
    train_vec.GaussianPolicy(net_log_std=True) with the trunk depth as a parameter.  ``ls_rows``: (weights [A, 32], bias [A])
    of the log-std rows; default: random, scaled so that ls stays in about [-1.5, 0.5] (the hidden units lie in [-1, 1]:
    the weighted sum has a standard deviation below 0.3, the bias is -0.5 +- 0.2)."""

    def __init__(self, D, A, layers, seed, ls_rows=None):
        Net.__init__(self, D, A, layers, seed)
        self.A = A
        old = self.linears(self.mu)[-1]
        head = torch.nn.Linear(32, 2 * A)
        if ls_rows is None:
            g = torch.Generator().manual_seed(77 * seed + 3 * D + A + layers)
            ls_rows = (torch.randn(A, 32, generator=g) * 0.3 / 32 ** 0.5, torch.randn(A, generator=g) * 0.2 - 0.5)
        with torch.no_grad():
            head.weight[:A].copy_(old.weight)
            head.bias[:A].copy_(old.bias)
            head.weight[A:].copy_(ls_rows[0])
            head.bias[A:].copy_(ls_rows[1])
        self.mu[len(self.mu) - 1] = head
        del self.log_std

    def dist(self, obs):
        out = self.mu(obs)
        return out[..., :self.A], out[..., self.A:]

    def logp_value_dist(self, obs, act):
        mu, ls = self.dist(obs)
        logp = (-0.5 * ((act - mu) / ls.exp()) ** 2 - ls - 0.9189385).sum(-1)
        return logp, self.value(obs).squeeze(-1), mu, ls

    def logp_value(self, obs, act):
        return self.logp_value_dist(obs, act)[:2]

    def tensors(self):
        """{name: parameter} in the packed order [policy with its 2A-row head][value]."""
        out = {}
        for i, l in enumerate(self.linears(self.mu)):
            out["pi.W%d" % i], out["pi.b%d" % i] = l.weight, l.bias
        for i, l in enumerate(self.linears(self.value)):
            out["v.W%d" % i], out["v.b%d" % i] = l.weight, l.bias
        return out


def learner_ls(sim, net):
    from flow_amd.utils.device_ppo import DeviceLearner
    g = copy.deepcopy(net).float().cuda()
    pl, vl = g.linears(g.mu), g.linears(g.value)
    return DeviceLearner(sim, pl[:-1], pl[-1], None, vl[:-1], vl[-1], net_log_std=True), g


class Prelude(object):
    """A policy for ppo_update whose no_grad pass is GIVEN (logp_old, val_old and the old distribution, per sample):
    ppo_update itself then builds the loss and autograd its gradient, in the dtype of ``net``."""

    def __init__(self, net, logp_old, val_old, mean_old, ls_old):
        self.net, dt = net, next(net.parameters()).dtype
        self.old = tuple(t.to(dt) for t in (logp_old, val_old, mean_old, ls_old))
        self.dtype = dt

    def parameters(self):
        return self.net.parameters()

    def logp_value(self, obs, act):
        return self.net.logp_value(obs, act) if torch.is_grad_enabled() else self.old[:2]

    def logp_value_dist(self, obs, act):
        return self.net.logp_value_dist(obs, act) if torch.is_grad_enabled() else self.old

    def value(self, obs):
        return torch.zeros(obs.shape[0], 1, dtype=self.dtype)


def sums_of(net, c, adv_n):
    """{sum pg, sum vfl, sum KL, sum H} by the formulas of include/flowsim.h (fs_ppo_loss) with ls and ls_o per sample, in
    the dtype of ``net``, and the sums of |term| beside them."""
    dt = next(net.parameters()).dtype
    obs, act, logp_old, mean_old, ls_old, val_old, adv_n, ret = (t.to(dt) for t in (
        c["obs"], c["act"], c["logp_old"], c["mean_old"], c["ls_old"], c["val_old"], adv_n, c["ret"]))
    with torch.no_grad():
        logp, v, mu, ls = net.logp_value_dist(obs, act)
        ratio = (logp - logp_old).exp()
        pg = torch.min(ratio * adv_n, ratio.clamp(1 - CLIP, 1 + CLIP) * adv_n)
        v_c = val_old + (v - val_old).clamp(-VF_CLIP, VF_CLIP)
        vfl = torch.max((v - ret) ** 2, (v_c - ret) ** 2)
        kl = (ls - ls_old + ((2 * ls_old).exp() + (mean_old - mu) ** 2) / (2 * (2 * ls).exp()) - 0.5).sum(-1)
        h = (ls + HALF_LOG_2PIE).sum(-1)
    terms = torch.stack([pg, vfl, kl, h])
    return terms.sum(1).double(), terms.double().abs().sum(1)


# (the seed's offset per case: float64 alone picked it, on the CPU, so that every case -- the five-sample ones included --
# meets the conditions head_case asserts; 0 where none is listed)
OFFSETS = {(65, 13, 3, 64): 1}


@functools.lru_cache(maxsize=None)
def head_case(D, A, layers, n, offset=None):
    """Inputs of one case with a general network head, drawn on the CPU, and train_vec.ppo_update's float64 / float32
    gradients on them with every term on ("on") and off ("off"), computed once and never changed.  val_old and rew lie on
    the 2^-10 grid, so adv = rew - val_old and ret = rew are exact in float32: both precisions see the same advantages,
    statistics and returns."""
    import train_vec
    offset = OFFSETS.get((D, A, layers, n), 0) if offset is None else offset
    g = torch.Generator().manual_seed(53 * D + 11 * A + 7 * layers + 1000 * n + offset)
    net, net64 = NetLS(D, A, layers, seed=1), NetLS(D, A, layers, seed=1).double()
    obs = torch.randn(n, D, generator=g)
    with torch.no_grad():
        mu64, ls64 = net64.dist(obs.double())
        act = (mu64 + ls64.exp() * torch.randn(n, A, generator=g, dtype=torch.float64)).float()
        logp64, val64, _, _ = net64.logp_value_dist(obs.double(), act.double())
        logp32, val32, mu32, ls32 = net.logp_value_dist(obs, act)
    assert -2.0 < float(ls64.min()) and float(ls64.max()) < 1.0 and float(ls64.std()) > 0.05, (float(ls64.min()), float(ls64.max()))
    val0 = torch.round(val64.float() / GRID) * GRID
    rew = val0 + torch.round(torch.randn(n, generator=g) * 1.5 / GRID) * GRID
    logp_old = (logp64 + 0.3 * torch.randn(n, generator=g, dtype=torch.float64)).float()
    mean_old = (mu64 + 0.3 * ls64.exp() * torch.randn(n, A, generator=g, dtype=torch.float64)).float()
    ls_old = (ls64 + 0.1 * torch.randn(n, A, generator=g, dtype=torch.float64)).float()
    val_old = (torch.round((val64 + 0.6 * torch.randn(n, generator=g, dtype=torch.float64)) / GRID) * GRID).float()
    # ---- the surrogate's clip: no sample within 1e-3 of a boundary (float64 alone decides)
    ratio = (logp64 - logp_old.double()).exp()
    near = ((ratio - (1 - CLIP)).abs() < 1e-3) | ((ratio - (1 + CLIP)).abs() < 1e-3)
    assert float(near.double().mean()) < 0.02
    logp_old = torch.where(near, logp_old + 0.05, logp_old)
    ratio = (logp64 - logp_old.double()).exp()
    assert not bool((((ratio - (1 - CLIP)).abs() < 1e-3) | ((ratio - (1 + CLIP)).abs() < 1e-3)).any())
    # ---- the value clip: the same (loss_case's bands)
    v, r = val64, rew.double()

    def bands(vo):
        dv = v - vo.double()
        e1, e2 = (v - r) ** 2, (vo.double() + dv.clamp(-VF_CLIP, VF_CLIP) - r) ** 2
        outside = dv.abs() > VF_CLIP
        return ((dv.abs() - VF_CLIP).abs() < 1e-3) | (outside & ((e1 - e2).abs() < 1e-3)), outside & (e2 > e1)
    near, _ = bands(val_old)
    assert float(near.double().mean()) < 0.02
    for _ in range(4):                                       # (0.05, on the grid; among 1e5 samples a shifted one can land near again)
        val_old = torch.where(near, val_old + 51 * GRID, val_old)
        near, cut = bands(val_old)
        if not bool(near.any()):
            break
    assert not bool(near.any())
    cut = float(cut.double().mean())
    adv = (rew - val_old).double()
    assert torch.equal(adv, rew.double() - val_old.double()) and torch.equal((rew - val_old) + val_old, rew)
    mean, std = stats_of(adv)
    adv_n = ((adv - mean) / (std + 1e-8)).float()
    clipped = float((ratio.clamp(1 - CLIP, 1 + CLIP) * adv_n.double() < ratio * adv_n.double()).double().mean())
    assert 0.10 <= cut <= 0.60, "%.0f %% of the samples have their value gradient cut" % (100 * cut)
    assert 0.10 <= clipped <= 0.60, "%.0f %% of the samples are clipped" % (100 * clipped)
    c = dict(net=net, obs=obs, act=act, logp_old=logp_old, mean_old=mean_old, ls_old=ls_old, val_old=val_old, adv=adv, ret=rew,
             mean=mean, std=std, dist_old=torch.cat([mean_old, ls_old], 1).contiguous(), cut=cut, clipped=clipped,
             logp64=logp64, val64=val64, logp32=logp32, val32=val32, dist64=torch.cat([mu64, ls64], 1),
             dist32=torch.cat([mu32, ls32], 1))
    done = torch.ones(1, n, dtype=torch.uint8)                                      # K = 1, every episode ends: adv = rew - val_old
    grads, sums, mags = {"on": {}, "off": {}}, {}, {}
    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        for mode, kw in (("on", dict(kl=train_vec.AdaptiveKL(KL_TARGET, KL_COEF), entropy_coef=ENT, vf_clip=VF_CLIP)),
                         ("off", dict())):
            m = NetLS(D, A, layers, seed=1).to(dt)
            shard = (torch.stack([obs, obs]).to(dt), act.to(dt).view(1, n, A), rew.to(dt).view(1, n), done)
            pi = Prelude(m, logp_old, val_old, mean_old, ls_old)
            train_vec.ppo_update(pi, torch.optim.SGD(m.parameters(), lr=0.0), [shard], epochs=1, clip=CLIP, vf_coef=VF_COEF, **kw)
            grads[mode][name] = {k: p.grad.detach().double().clone() for k, p in m.tensors().items()}
        sums[name], mags[name] = sums_of(m, c, adv_n)
    return dict(c, grads=grads, sums=sums, mags=mags)


@functools.lru_cache(maxsize=None)
def head_yardstick(D, A, layers):
    """torch float32's own error on the shape's n = 259 inputs with this head: (forward, gradient with the terms on,
    gradient with the terms off), each the largest over its tensors."""
    c = head_case(D, A, layers, 259)
    fwd = max(rel_err(c["logp32"], c["logp64"]), rel_err(c["val32"], c["val64"]), rel_err(c["dist32"], c["dist64"]))
    on, off = (max(rel_err(c["grads"][m]["f32"][k], c["grads"][m]["f64"][k]) for k in c["grads"][m]["f64"]) for m in ("on", "off"))
    return fwd, on, off


def sums_err(x, c):
    return float(((x.double().cpu() - c["sums"]["f64"]).abs() / c["mags"]["f64"]).max())


def run_head(learner, c, msn=None, accumulate=False, terms=True, **over):
    """gradients_loss (terms on) or gradients_n (off) on the case's inputs (overridable): (grad, sums) on the CPU."""
    t = {k: (over[k] if k in over else c[k]).cuda() for k in ("obs", "act", "logp_old", "adv", "ret", "dist_old", "val_old")}
    msn = msn_of(c) if msn is None else msn
    if terms:
        learner.kl_state[0] = KL_COEF
        sums = learner.gradients_loss(t["obs"], t["act"], t["logp_old"], t["adv"], t["ret"], msn, mean_old=t["dist_old"],
                                      val_old=t["val_old"], clip=CLIP, vf_coef=VF_COEF, vf_clip=VF_CLIP, entropy_coef=ENT,
                                      kl=True, accumulate=accumulate)
    else:
        sums = learner.gradients_n(t["obs"], t["act"], t["logp_old"], t["adv"], t["ret"], msn, clip=CLIP, vf_coef=VF_COEF,
                                   accumulate=accumulate)
    torch.cuda.synchronize()
    return learner.grad.detach().cpu().clone(), sums.detach().cpu().clone()


# -------------------------------------------------------------------------------------- 1. the degenerate head, bit for bit
def degenerate_of(free):
    """The network head that IS the free-head Net ``free``: log-std rows with zero weights and bias log_std."""
    D, A, layers = free.linears(free.mu)[0].in_features, free.log_std.numel(), len(free.linears(free.mu)) - 1
    net = NetLS(D, A, layers, seed=1, ls_rows=(torch.zeros(A, 32), free.log_std.detach().clone()))
    with torch.no_grad():
        for a, b in zip(net.linears(net.mu)[:-1] + net.linears(net.value), free.linears(free.mu)[:-1] + free.linears(free.value)):
            a.load_state_dict(b.state_dict())
        net.linears(net.mu)[-1].weight[:A].copy_(free.linears(free.mu)[-1].weight)
        net.linears(net.mu)[-1].bias[:A].copy_(free.linears(free.mu)[-1].bias)
    return net


def shared_tensors(got_free, got_ls, A):
    """[(name, free form's tensor, network form's tensor)] of everything the two forms share."""
    out = []
    head_w, head_b = [k for k in got_ls if k.startswith("pi.W")][-1], [k for k in got_ls if k.startswith("pi.b")][-1]
    for k in got_ls:
        if k == head_w or k == head_b:
            out.append((k + "[:A]", got_free[k], got_ls[k][:A]))
        else:
            out.append((k, got_free[k], got_ls[k]))
    out.append(("log_std / " + head_b + "[A:]", got_free["log_std"], got_ls[head_b][A:]))
    return out


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("D,A,layers", SHAPES)
def test_a_head_with_zero_log_std_weights_is_the_free_form_bit_for_bit(sim, D, A, layers, n):
    c = loss_case(D, A, layers, n)
    free, fnet = learner_of(sim, c["net"])
    ls, lnet = learner_ls(sim, degenerate_of(c["net"]))
    assert ls.P == free.P + 32 * A                           # A rows of 32 weights more; the A biases take log_std's place
    for fn in ("fs_ppo_workspace", "fs_ppo_loss_workspace"):                        # G is the tile count in both forms
        per = 2 if fn == "fs_ppo_workspace" else 4
        for lr in (free, ls):
            assert int(getattr(sim.lib, fn)(ctypes.byref(lr.struct), n)) == -(-n // TILE) * (lr.P + per)
    obs, act = c["obs"].cuda(), c["act"].cuda()
    lp0, v0 = free.evaluate(obs, act)
    assert sim.last_kernel == "k_ppo_eval"
    lp1, v1 = ls.evaluate(obs, act)
    torch.cuda.synchronize()
    assert sim.last_kernel == "k_ppo_eval_ls"
    assert torch.equal(lp0, lp1) and torch.equal(v0, v1) and bool(torch.isfinite(lp0).all())
    assert torch.equal(ls.evaluate(obs, None)[1], v0) and sim.last_kernel == "k_ppo_eval"
    # ---- the plain form
    t = [obs, act, c["logp_old"].cuda(), c["adv"].cuda(), c["ret"].cuda()]
    l0 = free.gradients_n(*t, msn_of(c), clip=CLIP, vf_coef=VF_COEF).clone()
    assert sim.last_kernel == "k_ppo_grad"
    l1 = ls.gradients_n(*t, msn_of(c), clip=CLIP, vf_coef=VF_COEF).clone()
    torch.cuda.synchronize()
    assert sim.last_kernel == "k_ppo_grad_ls"
    assert torch.equal(l0, l1)
    for name, a, b in shared_tensors(split_grad(free, fnet), split_grad(ls, lnet), A):
        assert torch.equal(a, b), ("plain", name)
    assert float(ls.grad.abs().max()) > 0
    # ---- the full loss, every term on: the old log stds of every row are the free form's log_std_old
    _, s0 = run_loss(free, c)
    assert sim.last_kernel == "k_ppo_grad_loss"
    dist_old = torch.cat([c["mean_old"], c["ls_old"].expand(n, A)], 1).contiguous()
    ls.kl_state[0] = KL_COEF
    s1 = ls.gradients_loss(*t, msn_of(c), mean_old=dist_old.cuda(), val_old=c["val_old"].cuda(), clip=CLIP, vf_coef=VF_COEF,
                           vf_clip=VF_CLIP, entropy_coef=ENT, kl=True)
    torch.cuda.synchronize()
    assert sim.last_kernel == "k_ppo_grad_loss_ls"
    assert torch.equal(s0, s1.cpu()) and float(s0[2]) > 0
    for name, a, b in shared_tensors(split_grad(free, fnet), split_grad(ls, lnet), A):
        assert torch.equal(a, b), ("full loss", name)
    got = split_grad(ls, lnet)
    head_w = [k for k in got if k.startswith("pi.W")][-1]
    assert float(got[head_w][A:].abs().max()) > 0            # (the log-std rows' weights do get a gradient)


# --------------------------------------------------------------------------------- 2. a general head against float64
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("D,A,layers", SHAPES)
def test_gradient_and_loss_sums_of_a_general_head_agree_with_float64_ppo_update(sim, D, A, layers, n):
    c = head_case(D, A, layers, n)
    y_fwd, y_on, y_off = head_yardstick(D, A, layers)
    learner, net = learner_ls(sim, c["net"])
    _, sums = run_head(learner, c)
    assert sim.last_kernel == "k_ppo_grad_loss_ls"
    got, want = split_grad(learner, net), c["grads"]["on"]["f64"]
    kern = {k: rel_err(got[k], want[k]) for k in want}
    worst = max(kern, key=kern.get)
    e_sums = sums_err(sums, c)
    print("network head, full loss (%d, %d, %d) n=%d: kernel %.3g (%s), yardstick (n=259) %.3g, ratio %.2f; loss sums %.3g "
          "(torch float32 here %.3g); clipped %.0f %%, cut %.0f %%"
          % (D, A, layers, n, kern[worst], worst, y_on, kern[worst] / y_on, e_sums, sums_err(c["sums"]["f32"], c),
             100 * c["clipped"], 100 * c["cut"]))
    for k, e in kern.items():
        assert e <= MARGIN * y_on, "%s: %.3g against 10 x %.3g" % (k, e, y_on)
    assert e_sums <= MARGIN * y_on, "%.3g against 10 x %.3g" % (e_sums, y_on)
    assert rel_err(sums, c["sums"]["f64"]) <= MARGIN * y_on                         # (the four as one tensor)
    # ---- the terms off: the plain form
    _, loss = run_head(learner, c, terms=False)
    assert sim.last_kernel == "k_ppo_grad_ls"
    got, want = split_grad(learner, net), c["grads"]["off"]["f64"]
    kern = {k: rel_err(got[k], want[k]) for k in want}
    worst = max(kern, key=kern.get)
    print("network head, plain (%d, %d, %d) n=%d: kernel %.3g (%s), yardstick (n=259) %.3g, ratio %.2f"
          % (D, A, layers, n, kern[worst], worst, y_off, kern[worst] / y_off))
    for k, e in kern.items():
        assert e <= MARGIN * y_off, "%s: %.3g against 10 x %.3g" % (k, e, y_off)
    assert abs(float(loss[0]) - float(c["sums"]["f64"][0])) <= MARGIN * y_on * float(c["mags"]["f64"][0])


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("D,A,layers", SHAPES)
def test_evaluate_dist_gives_the_bits_of_evaluate_and_the_whole_distribution(sim, D, A, layers, n):
    c = head_case(D, A, layers, n)
    learner, _ = learner_ls(sim, c["net"])
    logp, val = learner.evaluate(c["obs"].cuda(), c["act"].cuda())
    logp2, val2, dist = learner.evaluate_dist(c["obs"].cuda(), c["act"].cuda())
    torch.cuda.synchronize()
    assert sim.last_kernel == "k_ppo_eval_ls"
    assert torch.equal(logp, logp2) and torch.equal(val, val2) and dist.shape == (n, 2 * A)
    bound = MARGIN * head_yardstick(D, A, layers)[0]
    e = (rel_err(dist, c["dist64"]), rel_err(dist[:, A:], c["dist64"][:, A:]), rel_err(logp, c["logp64"]), rel_err(val, c["val64"]))
    print("forward, network head (%d, %d, %d) n=%d: dist %.3g, log stds %.3g, logp %.3g, val %.3g; bound %.3g" % ((D, A, layers, n) + e + (bound,)))
    assert max(e) <= bound


# ------------------------------------------------------------------------------------------ 3. determinism, shards, absence
def test_the_same_bits_twice_shards_in_call_order_and_nothing_of_an_absent_row(sim):
    c1, c2 = head_case(65, 13, 3, 259), head_case(65, 13, 3, 64)
    learner, _ = learner_ls(sim, c1["net"])
    msn = msn_of(c1, 323)
    for terms in (True, False):
        a, sa = run_head(learner, c1, msn=msn, terms=terms)
        learner.grad.fill_(float("nan"))
        learner.loss_sums.fill_(float("nan"))
        learner.loss.fill_(float("nan"))                                            # (accumulate=False overwrites)
        b, sb = run_head(learner, c1, msn=msn, terms=terms)
        assert torch.equal(a, b) and torch.equal(sa, sb) and bool(torch.isfinite(a).all())
        s2, ss2 = run_head(learner, c2, msn=msn, terms=terms)
        run_head(learner, c1, msn=msn, terms=terms)
        acc, sacc = run_head(learner, c2, msn=msn, terms=terms, accumulate=True)
        assert torch.equal(acc, (a.cuda() + s2.cuda()).cpu()) and torch.equal(sacc, (sa.cuda() + ss2.cuda()).cpu())
        # absent rows: the same bits whatever they hold -- NaN observations, NaN old means and log stds, a NaN old value
        g = torch.Generator().manual_seed(5)
        absent = torch.rand(259, generator=g) < 0.2
        absent[64:128] = True                                                       # one whole 64-sample tile
        act = c1["act"].clone()
        act[absent, torch.randint(0, 13, (259,), generator=g)[absent]] = float("nan")
        msn_p = msn_of(c1, int((~absent).sum()))
        p, sp = run_head(learner, c1, msn=msn_p, terms=terms, act=act)
        assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(sp).all()) and not torch.equal(p, a)
        nan = float("nan")
        held = {k: c1[k].clone() for k in ("obs", "logp_old", "adv", "ret", "dist_old", "val_old")}
        for k in held:
            held[k][absent] = nan
        held["dist_old"][absent.nonzero()[0]] = float("inf")
        act2 = act.clone()
        act2[absent] = nan
        q, sq = run_head(learner, c1, msn=msn_p, terms=terms, act=act2, **held)
        assert torch.equal(p, q) and torch.equal(sp, sq)
    lp_a, v_a, d_a = learner.evaluate_dist(c1["obs"].cuda(), act.cuda())
    lp_0, v_0, d_0 = learner.evaluate_dist(c1["obs"].cuda(), c1["act"].cuda())
    keep = (~absent).cuda()
    assert torch.equal(lp_a[keep], lp_0[keep]) and torch.equal(v_a, v_0) and torch.equal(d_a, d_0)


# ------------------------------------------------------------------------------------------------- 4. above the cap
def test_above_the_cap_the_gradient_is_the_stated_composition_and_agrees_with_float64(sim):
    from test_device_ppo_scale_gpu import absent_rows, holed_actions
    D, A, layers, G, n = 3, 1, 2, CAP_3_1_2, SCALE_N
    assert n == 98373
    c = head_case(D, A, layers, n)
    learner, net = learner_ls(sim, c["net"])
    P, tiles = learner.P, (n + TILE - 1) // TILE
    assert int(sim.lib.fs_ppo_loss_workspace(ctypes.byref(learner.struct), n)) == G * (P + 4) and tiles == 2 * G + 2
    # ---- float64, every row present: torch float32's error on THESE inputs is the yardstick
    _, sums = run_head(learner, c)
    assert sim.last_kernel == "k_ppo_grad_loss_ls"
    got, want, f32 = split_grad(learner, net), c["grads"]["on"]["f64"], c["grads"]["on"]["f32"]
    y = max(rel_err(f32[k], want[k]) for k in want)
    kern = {k: rel_err(got[k], want[k]) for k in want}
    worst = max(kern, key=kern.get)
    print("network head (%d, %d, %d) n=%d: kernel %.3g (%s), torch float32 on the same inputs %.3g, ratio %.2f; loss sums %.3g"
          % (D, A, layers, n, kern[worst], worst, y, kern[worst] / y, sums_err(sums, c)))
    for k, e in kern.items():
        assert e <= MARGIN * y, "%s: %.3g against 10 x %.3g" % (k, e, y)
    assert sums_err(sums, c) <= MARGIN * y
    # ---- the composition of tile sums, a fifth of the rows absent (a whole tile of the second round among them)
    absent = absent_rows(n, G, last_row=True)
    act = holed_actions(c, absent)
    msn = msn_of(c, int((~absent).sum()))
    dev = [c["obs"].cuda(), act.cuda(), c["logp_old"].cuda(), c["adv"].cuda(), c["ret"].cuda()]
    dist_old, val_old = c["dist_old"].cuda(), c["val_old"].cuda()
    kw = dict(clip=CLIP, vf_coef=VF_COEF, vf_clip=VF_CLIP, entropy_coef=ENT, kl=True)
    learner.kl_state[0] = KL_COEF
    stack = torch.empty(tiles, P + 4, dtype=torch.float32, device=learner.device)
    for t in range(tiles):                                   # (a call on one tile's rows alone has G = 1: its own block sums)
        lo, hi = TILE * t, min(TILE * t + TILE, n)
        learner.gradients_loss(*(x[lo:hi] for x in dev), msn, mean_old=dist_old[lo:hi], val_old=val_old[lo:hi], **kw)
        stack[t, :P] = learner.grad
        stack[t, P:] = learner.loss_sums
    learner.gradients_loss(*dev, msn, mean_old=dist_old, val_old=val_old, **kw)
    torch.cuda.synchronize()
    whole, stack = torch.cat([learner.grad, learner.loss_sums]).cpu(), stack.cpu()
    assert bool(torch.isfinite(whole).all()) and bool(torch.isfinite(stack).all()) and float(whole[:P].abs().max()) > 0
    assert not bool(stack[G + 3].any()) and bool(stack[tiles - 1].any())
    want = ppo_ref.compose_ref(stack, G)
    assert torch.equal(whole, want), "%d of %d elements differ from the stated order" % (int((whole != want).sum()), whole.numel())
    assert not torch.equal(whole, ppo_ref.compose_ref(stack, 1))                    # (another order is other bits)


# ------------------------------------------------------------------------------------------------------ 5. minibatches
def mb_step(learner, c, B, k, epoch, **kw):
    t = {name: c[name].cuda() for name in ("obs", "act", "logp_old", "adv", "ret", "dist_old", "val_old")}
    learner.mb_epoch.fill_(epoch)
    learner.kl_state[0] = KL_COEF
    sums = learner.minibatch_step(t["obs"], t["act"], t["logp_old"], t["adv"], t["ret"], msn_of(c), B, k, shuffle_seed=SEED,
                                  mean_old=t["dist_old"], val_old=t["val_old"], clip=CLIP, vf_coef=VF_COEF, vf_clip=VF_CLIP,
                                  entropy_coef=ENT, kl=True, **kw)
    torch.cuda.synchronize()
    return sums


def fresh(learner, w0):
    learner._adam_buffers()
    learner.weights.copy_(w0)
    learner.m.zero_()
    learner.v.zero_()
    learner.state.copy_(torch.tensor(ref.fresh_state(), dtype=torch.float64))


STATE_NAMES = ("weights", "m", "v", "state")


@pytest.mark.parametrize("D,A,layers", [(3, 1, 2), (65, 13, 3)])
def test_the_fused_step_gives_the_bits_of_partial_plus_finish(sim, D, A, layers):
    from flow_amd.utils.device_ppo import epoch_permutation
    c, N, B = head_case(D, A, layers, 259), 259, 128
    learner, net = learner_ls(sim, c["net"])
    w0 = learner.weights.clone()
    for k in (0, 2):
        out = []
        for mode in ("step", "step", "chain"):
            fresh(learner, w0)
            for name in ("grad", "loss_sums", "mb_count"):
                getattr(learner, name).fill_(float("nan"))
            mb_step(learner, c, B, k, 4, first=True, partial=mode == "chain")
            assert sim.last_kernel == "k_ppo_minibatch_ls"
            if mode == "chain":
                assert learner.mb_count.item() == len(epoch_permutation(SEED, 4, N)[k * B:(k + 1) * B])
                assert int(learner.mb_epoch.item()) == 4                            # (PARTIAL never advances the epoch)
                learner.mb_finish(last=k == 2)
                torch.cuda.synchronize()
                assert sim.last_kernel == "k_mb_finish"
            out.append({name: getattr(learner, name).detach().cpu().clone()
                        for name in STATE_NAMES + ("grad", "loss_sums", "mb_epoch")})
        for name in out[0]:
            assert torch.equal(out[0][name], out[1][name]), (name, "second call")
            assert torch.equal(out[0][name], out[2][name]), (name, "chain")
        assert bool(torch.isfinite(out[0]["grad"]).all()) and not torch.equal(out[0]["weights"], w0.cpu())
        assert int(out[0]["mb_epoch"].item()) == (5 if k == 2 else 4)
        got = split_grad(learner, net)
        head_w = [name for name in got if name.startswith("pi.W")][-1]
        assert float(got[head_w][A:].abs().max()) > 0


def fragment_ls(D, A, K, R, seed, net):
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn(K + 1, R, D, generator=g)
    with torch.no_grad():
        mu, ls = net.dist(obs[:K].reshape(K * R, D))
        act = (mu + ls.exp() * torch.randn(K * R, A, generator=g)).view(K, R, A)
    rew = torch.randn(K, R, generator=g)
    done = (torch.rand(K, R, generator=g) < 0.1).to(torch.uint8)
    done[K // 2, 0] = 2
    return obs, act, rew, done


def flat(net):
    return torch.cat([p.detach().reshape(-1) for p in net.tensors().values()]).double().numpy()


@functools.lru_cache(maxsize=None)
def update_problem(D, A, layers, minibatch):
    """A fragment of 8 x 37 samples and train_vec.ppo_update on it with the terms on -- 2 epochs of minibatches of 128, or 4
    whole-batch epochs -- by torch on the CPU in float64 and in float32 (computed once), from the same weights and with the
    same permutations as the code under test."""
    import train_vec
    net = NetLS(D, A, layers, seed=3)
    shard = fragment_ls(D, A, 8, 37, 17 * D + A, net)
    w0, out, kls = flat(net), {}, {}
    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        m = copy.deepcopy(net).to(dt)
        sh = (shard[0].to(dt), shard[1].to(dt), shard[2].to(dt), shard[3])
        kls[name] = train_vec.AdaptiveKL(KL_TARGET, 0.2)
        train_vec.ppo_update(m, torch.optim.Adam(m.parameters(), lr=ref.LR), [sh], epochs=2 if minibatch else 4, clip=0.2,
                             kl=kls[name], entropy_coef=ENT, vf_clip=VF_CLIP, vf_coef=0.5, minibatch=minibatch,
                             shuffle_seed=SEED, epoch0=0)
        out[name] = flat(m)
    return net, shard, w0, out["f64"], ref.displacement_error(out["f32"], out["f64"], w0), kls["f64"]


@pytest.mark.parametrize("minibatch", [128, None])
@pytest.mark.parametrize("D,A,layers", [(3, 1, 2), (65, 13, 3)])
def test_update_stays_within_float32_torch_of_float64_ppo_update(sim, D, A, layers, minibatch):
    net, shard, w0, w64, err32, kl64 = update_problem(D, A, layers, minibatch)
    learner, _ = learner_ls(sim, net)
    learner.adopt_parameters()
    learner.update([on_gpu(shard)], epochs=2 if minibatch else 4, clip=0.2, lr=ref.LR, minibatch=minibatch, shuffle_seed=SEED,
                   **TERMS)
    torch.cuda.synchronize()
    assert sim.last_kernel == "k_kl_adapt"
    err = ref.displacement_error(learner.weights.cpu().numpy(), w64, w0)
    coef, mean_kl = learner.kl_state.tolist()
    print("update, network head (%d, %d, %d) minibatch %s: kernels %.3g, torch float32 %.3g (ratio %.2f); mean KL %.3g "
          "(float64 %.3g), coefficient %.3g (float64 %.3g)"
          % (D, A, layers, minibatch, err, err32, err / err32, mean_kl, kl64.mean_kl, coef, kl64.coef))
    assert err <= MARGIN * err32
    assert coef == kl64.coef                                                        # the same branch of the rule


# ------------------------------------------------------------------------------------------------------------ 6. update()
def test_update_with_the_terms_on_equals_its_stages_called_one_by_one(sim):
    D, A, layers = 65, 13, 3
    net = NetLS(D, A, layers, seed=2)
    shards = [fragment_ls(D, A, 8, 16, 1, net), fragment_ls(D, A, 5, 7, 2, net)]
    shards[1][1][2, 3, 1] = float("nan")                                            # an absent agent in the second shard
    whole, _ = learner_ls(sim, net)
    whole.adopt_parameters()
    out = whole.update([on_gpu(s) for s in shards], epochs=4, **TERMS)
    torch.cuda.synchronize()
    assert sim.last_kernel == "k_kl_adapt" and out is whole.loss_sums
    steps, _ = learner_ls(sim, net)
    steps.adopt_parameters()
    steps.kl_state[0] = 0.2
    prepared, stats = [], torch.zeros(3, dtype=torch.float64).cuda()
    for j, (obs, act, rew, done) in enumerate(on_gpu(s) for s in shards):
        k, r = rew.shape
        o, a = obs[:k].reshape(k * r, D), act.reshape(k * r, A)
        logp, val, dist_old = steps.evaluate_dist(o, a)
        assert sim.last_kernel == "k_ppo_eval_ls" and dist_old.shape == (k * r, 2 * A)
        last = steps.evaluate(obs[k], None)[1]
        adv, ret = steps.gae(rew, val.view(k, r), last, done)
        adv64, _ = steps.adv_stats(adv, a, accumulate=j > 0, stats=stats)
        prepared.append((o, a, logp, adv64, ret.reshape(-1), dist_old, val))
    msn = steps.adv_finish(stats)
    for _ in range(4):
        for j, (o, a, logp, adv64, ret, dist_old, val) in enumerate(prepared):
            steps.gradients_loss(o, a, logp, adv64, ret, msn, mean_old=dist_old, val_old=val, clip=0.2, vf_coef=0.5,
                                 vf_clip=VF_CLIP, entropy_coef=ENT, kl=True, accumulate=j > 0)
            assert sim.last_kernel == "k_ppo_grad_loss_ls"
        steps.adam_step(lr=3e-4, betas=(0.9, 0.999), eps=1e-8)
    steps.kl_adapt(KL_TARGET, msn)
    torch.cuda.synchronize()
    assert msn[2].item() == 8 * 16 + 5 * 7 - 1
    for name in ("weights", "grad", "loss_sums", "m", "v", "state", "kl_state"):
        assert torch.equal(getattr(whole, name), getattr(steps, name)), name
    assert whole.state[0].item() == 4 and bool(torch.isfinite(whole.weights).all())
    # ---- the defaults: the plain form, launch for launch
    plain, _ = learner_ls(sim, net)
    plain.adopt_parameters()
    w0 = plain.weights.clone()
    assert plain.update([on_gpu(shards[0])], epochs=1) is plain.loss
    torch.cuda.synchronize()
    assert sim.last_kernel == "k_adam" and not torch.equal(plain.weights, w0) and bool(torch.isfinite(plain.weights).all())


@pytest.mark.parametrize("minibatch", [None, 128])
def test_update_replays_from_a_graph_with_the_bits_of_eager_calls(sim, minibatch):
    net, shard, _, _, _, _ = update_problem(3, 1, 2, minibatch)
    learner, _ = learner_ls(sim, net)
    learner.adopt_parameters()
    shard = on_gpu(shard)
    start = learner.weights.clone()
    kw = dict(epochs=2, minibatch=minibatch, shuffle_seed=SEED, **TERMS)

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
        side.synchronize()                                  # to it (fs_set_stream synchronises) and every buffer exists
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        learner.update([shard], **kw)
    torch.cuda.synchronize()
    rewind()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    steps = 2 * (2 * 3 if minibatch else 2)
    assert learner.state[0].item() == steps
    names = ("weights", "m", "v", "state", "grad", "loss_sums", "kl_state", "mb_epoch")
    replayed = {k: getattr(learner, k).clone() for k in names}
    assert not torch.equal(replayed["weights"], start) and int(replayed["mb_epoch"].item()) == (4 if minibatch else 0)
    rewind()
    learner.update([shard], **kw)
    learner.update([shard], **kw)
    torch.cuda.synchronize()
    assert learner.state[0].item() == steps
    for k, want in replayed.items():
        assert torch.equal(getattr(learner, k), want), k


WATCHED = ("evaluate", "evaluate_dist", "_eval_dist", "gradients_n", "_grad_n", "gradients_loss", "_grad_loss", "minibatch_step",
           "_mb_step", "mb_finish", "adam_step", "kl_adapt", "_adv_stats")


def watch(monkeypatch, kernels):
    from flow_amd.utils.device_ppo import DeviceLearner

    def counted(name):
        real = getattr(DeviceLearner, name)

        def fn(self, *a, **kw):
            out = real(self, *a, **kw)
            kernels.append(self.sim.last_kernel)
            return out
        monkeypatch.setattr(DeviceLearner, name, fn)
    for name in WATCHED:
        counted(name)


def test_without_the_keyword_no_ls_kernel_is_ever_launched(sim, monkeypatch):
    from test_device_ppo_loss_gpu import update_problem as free_problem
    net, shard, _, _, _, _ = free_problem(3, 1, 2)
    kernels = []
    watch(monkeypatch, kernels)
    for kw in (dict(), dict(TERMS), dict(TERMS, minibatch=128, shuffle_seed=SEED), dict(TERMS, minibatch=128, fused=True)):
        learner, _ = learner_of(sim, net)
        learner.adopt_parameters()
        learner.update([on_gpu(shard)], epochs=2, **kw)
    c = loss_case(3, 1, 2, 64)
    learner, _ = learner_of(sim, c["net"])
    learner.evaluate(c["obs"].cuda(), c["act"].cuda())
    learner.evaluate_dist(c["obs"].cuda(), c["act"].cuda())
    run_loss(learner, c)
    torch.cuda.synchronize()
    assert len(kernels) > 20 and not any(k.endswith("_ls") for k in kernels), sorted(set(kernels))
    assert {"k_ppo_eval", "k_ppo_grad", "k_ppo_grad_loss", "k_ppo_minibatch", "k_mb_finish", "k_adam"} <= set(kernels)
    # (and with it, the same calls do)
    kernels.clear()
    net_ls, shard_ls, _, _, _, _ = update_problem(3, 1, 2, 128)
    for kw in (dict(), dict(TERMS), dict(TERMS, minibatch=128, shuffle_seed=SEED, fused=True)):
        learner, _ = learner_ls(sim, net_ls)
        learner.adopt_parameters()
        learner.update([on_gpu(shard_ls)], epochs=2, **kw)
    torch.cuda.synchronize()
    assert {"k_ppo_eval_ls", "k_ppo_grad_ls", "k_ppo_grad_loss_ls", "k_ppo_minibatch_ls"} <= set(kernels)
    assert not {"k_ppo_grad", "k_ppo_grad_loss", "k_ppo_minibatch"} & set(kernels)


def test_the_host_n_gradient_refuses_the_head_by_name(sim):
    c = head_case(3, 1, 2, 64)
    learner, _ = learner_ls(sim, c["net"])
    with pytest.raises(NotImplementedError, match="net_log_std") as e:
        learner.gradients(c["obs"].cuda(), c["act"].cuda(), c["logp_old"].cuda(), c["adv"].cuda(), c["ret"].cuda(), c["mean"],
                          c["std"])
    assert "fs_ppo_grad_dev" in str(e.value)
    with pytest.raises(ValueError, match="log_std_old_dev"):                        # the old log stds travel in mean_old
        learner.gradients_loss(c["obs"].cuda(), c["act"].cuda(), c["logp_old"].cuda(), c["adv"].cuda(), c["ret"].cuda(), msn_of(c),
                               mean_old=c["dist_old"].cuda(), log_std_old=torch.zeros(1).cuda(), kl=True)


# --------------------------------------------------------------------------------------------------------------- 7. share
def ring_handle():
    import train_vec
    from flow_amd.envs import VecFlowEnv
    vec = VecFlowEnv(train_vec.ring_flow_params(20), num_replicas=64, device=0)
    return vec, vec.close, "k_policy_act"


def wide_handle():
    from helpers import bottleneck_spec, bottleneck_tables, segment_cells
    from test_open_gpu import make
    tb = bottleneck_tables()
    oc, ac = segment_cells(tb, [("1", 4)]), segment_cells(tb, [("1", 3), ("5", 1)])  # 4 x 16 + 1 observations, 12 + 1 actions
    s = make(bottleneck_spec(R=64, cap_human=40, cap_rl=8, obs_cells=oc, action_cells=ac, num_rl=13), "f32")
    return s, s.close, "k_policy_act_wide"


@pytest.mark.parametrize("D,A,layers,handle", [(3, 1, 2, ring_handle), (65, 13, 3, wide_handle)])
def test_a_sharing_policy_acts_with_the_bits_of_a_synced_one_after_an_update(D, A, layers, handle):
    """policy_act draws from the replicas' Philox streams, keyed by the policy's seed and the handle's draw counter: two
    handles in the same state, one per policy, see the same draws."""
    from flow_amd.utils.device_policy import DevicePolicy
    net = NetLS(D, A, layers, seed=4)
    shard = fragment_ls(D, A, 4, 16, 9, net)
    obs = torch.rand(64, D, generator=torch.Generator().manual_seed(2)) * 2 - 1
    outs = []
    for share in (True, False):
        h, close, kernel = handle()
        try:
            s = h.sim if hasattr(h, "sim") else h
            if s is not h:
                h.reset()
            assert s.obs_dim == D and s.policy_action_dim == A
            learner, g = learner_ls(h, net)
            learner.adopt_parameters()
            pl = g.linears(g.mu)
            if share:
                pol = DevicePolicy(pl[:-1], pl[-1], log_std=None, seed=5, act_dim=A).share(learner)
                assert pol.struct.weights_dev == learner.weights.data_ptr() and not pol.struct.log_std_dev
            w0 = learner.weights.clone()
            learner.update([on_gpu(shard)], epochs=2, lr=1e-2, **TERMS)
            torch.cuda.synchronize()
            assert not torch.equal(learner.weights, w0)
            if not share:                                    # a fresh policy, synced from the adopted parameters
                pol = DevicePolicy(pl[:-1], pl[-1], log_std=None, seed=5, act_dim=A)
                assert pol.struct.weights_dev != learner.weights.data_ptr()
                assert torch.equal(pol.buf, learner.weights[:learner.n_policy])
            act, logp = torch.zeros(64, A).cuda(), torch.zeros(64).cuda()
            torch.cuda.synchronize()
            s.policy_act_dev(pol.struct, obs.cuda(), act, logp)
            s.sync()
            assert s.last_kernel == kernel
            outs.append((act.cpu().clone(), logp.cpu().clone(), learner.weights.cpu().clone()))
        finally:
            close()
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(outs[0][0]).all()) and bool(torch.isfinite(outs[0][1]).all())


# ---------------------------------------------------------------------------------------------------------- 8. end to end
@pytest.mark.parametrize("fuse_policy", [False, True])
def test_train_on_device_with_the_network_head(monkeypatch, fuse_policy):
    import train
    import train_vec
    from flow_amd.utils.device_ppo import DeviceLearner
    singleagent_ring, multiagent = train.load_experiment("singleagent_ring")
    assert not multiagent
    made, lines = [], []
    init = DeviceLearner.__init__

    def recording(self, *a, **kw):
        init(self, *a, **kw)
        made.append(self)
    monkeypatch.setattr(DeviceLearner, "__init__", recording)
    fp = singleagent_ring.flow_params
    fp["sim"].render = False
    hist = train_vec.train_on_device(fp, replicas=8, fragment=10, iterations=2, device_adam=True, net_log_std=True,
                                     fuse_action_vector=fuse_policy, kl_target=KL_TARGET, log=lambda s: lines.append(s))
    assert len(hist) == 2 and all(np.isfinite(h) for h in hist)
    assert len(made) == 1 and made[0].net_log_std and made[0].A == 1
    its = [s for s in lines if s.startswith("iteration")]
    assert len(its) == 2 and all(np.isfinite(float(s.split("KL")[1].split()[0])) for s in its)
    assert any(s.startswith("rollout: fused policy + step kernel") for s in lines), lines   # (through share: the learner's buffer)
    head = made[0].p_head
    w, b = head.weight.detach().cpu(), head.bias.detach().cpu()
    assert w.shape == (2, 32) and bool(torch.isfinite(w).all()) and bool(torch.isfinite(b).all())
    assert float(w[1].abs().max()) > 0 and float(b[1]) != -0.5                      # the log-std row has moved
    with pytest.raises(NotImplementedError, match="device_adam"):
        train_vec.train_on_device(fp, replicas=8, fragment=10, iterations=1, device_update=True, net_log_std=True,
                                  log=lambda s: None)
