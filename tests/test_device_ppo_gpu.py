"""The PPO update on the device (flow_amd/csrc/flowsim_learn.h; fs_ppo_eval_dev, fs_gae_dev, fs_ppo_grad_dev through
flow_amd.utils.device_ppo.DeviceLearner), on a float32 handle of a 2-replica ring.

* k_gae equals train_vec.gae, evaluated by torch on the CPU, bit for bit;
* k_ppo_eval agrees with the same networks in torch float64, and the packed gradient of k_ppo_grad, per parameter tensor,
  with torch float64 autograd of ppo_update's own loss.  The error measure is max|x - x64| / max|x64| per tensor; the
  yardstick is what torch FLOAT32 shows by the same measure on the same inputs, and the kernels may be 10 times that (their
  tanh is hardware exp2 and rcp, their sample sum runs in another order).  The yardstick of a shape (D, A, layers) is taken
  ONCE, on its n = 259 inputs, as the largest error over its tensors, and holds for every tensor and every n of the shape: a
  one-element tensor or a five-sample batch is one draw of that error and can land near zero by chance.  The reference
  networks are evaluated by torch on the CPU (the same bits on every machine);
* absent agents (NaN action rows) add nothing and nothing of their rows reaches an output; two calls give the same bits;
  accumulation over shards is the sum in call order;
* train_on_device(device_update=True) trains on k_ppo_grad, and without the flag never launches it.

What "the gradient of the present samples alone, bit for bit" means here: the sum over samples has ONE order, fixed by
(n, D, A, layers) -- a 64-sample tile per workgroup, the tiles' partial sums added in ascending order.  Removing scattered
rows from the batch moves the others to other tiles, which is another order of the same sum, so that comparison is made
where the order survives: a batch with a whole absent tile inserted equals the batch without it, bit for bit (absent rows
add exact zeros).  For scattered absences the test holds the kernel to (a) the same bits whatever the absent rows contain,
NaN observations included, and (b) torch float64 on the present rows alone, within the bound above."""
import copy
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "examples"))

from helpers import ring_spec  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(3, 1, 2), (28, 1, 1), (65, 13, 3), (141, 20, 2), (160, 32, 3)]
COUNTS = [5, 64, 259]
CLIP = 0.2
MARGIN = 10.0


@pytest.fixture(scope="module")
def sim():
    from flow_amd.sim import FlowSim
    s = FlowSim(ring_spec(R=2, N=5, bunching=0), "f32")
    yield s
    s.close()


class Net(torch.nn.Module):
    """train_vec.GaussianPolicy with the trunk depth as a parameter."""

    def __init__(self, D, A, layers, seed):
        super().__init__()
        g = torch.Generator().manual_seed(1000 * seed + 7 * D + A + layers)

        def trunk(n_out):
            dims = [D] + [32] * layers
            mods = []
            for i in range(layers):
                mods += [torch.nn.Linear(dims[i], dims[i + 1]), torch.nn.Tanh()]
            mods.append(torch.nn.Linear(32, n_out))
            for m in mods:
                if isinstance(m, torch.nn.Linear):
                    with torch.no_grad():
                        m.weight.copy_(torch.randn(m.weight.shape, generator=g) / m.in_features ** 0.5)
                        m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)
            return torch.nn.Sequential(*mods)
        self.mu, self.value = trunk(A), trunk(1)
        self.log_std = torch.nn.Parameter(torch.randn(A, generator=g) * 0.2 - 0.5)

    def linears(self, seq):
        return [m for m in seq if isinstance(m, torch.nn.Linear)]

    def logp_value(self, obs, act):
        mu = self.mu(obs)
        std = self.log_std.exp()
        logp = (-0.5 * ((act - mu) / std) ** 2 - self.log_std - 0.9189385).sum(-1)
        return logp, self.value(obs).squeeze(-1)

    def tensors(self):
        """{name: parameter} in the packed order [policy][log_std][value]."""
        out = {}
        for i, l in enumerate(self.linears(self.mu)):
            out["pi.W%d" % i], out["pi.b%d" % i] = l.weight, l.bias
        out["log_std"] = self.log_std
        for i, l in enumerate(self.linears(self.value)):
            out["v.W%d" % i], out["v.b%d" % i] = l.weight, l.bias
        return out


def learner_of(sim, net):
    from flow_amd.utils.device_ppo import DeviceLearner
    g = copy.deepcopy(net).float().cuda()
    pl, vl = g.linears(g.mu), g.linears(g.value)
    return DeviceLearner(sim, pl[:-1], pl[-1], g.log_std, vl[:-1], vl[-1]), g


class FixedPrelude(object):
    """A policy for ppo_update whose no_grad pass is GIVEN (logp_old, val): ppo_update itself then builds the loss and
    autograd its gradient, in the dtype of ``net``."""

    def __init__(self, net, logp_old, val):
        self.net, self.dtype = net, net.log_std.dtype
        self.logp_old, self.val = logp_old.to(self.dtype), val.to(self.dtype)

    def parameters(self):
        return self.net.parameters()

    def logp_value(self, obs, act):
        if torch.is_grad_enabled():
            return self.net.logp_value(obs, act)
        return self.logp_old, self.val

    def value(self, obs):
        return torch.zeros(obs.shape[0], 1, dtype=self.dtype)


def stats_of(adv):
    """(mean, std) of the float64 advantages as ppo_update takes them from its three sums."""
    n = torch.tensor(float(adv.numel()), dtype=torch.float64)
    mean = adv.sum() / n
    return mean, ((((adv * adv).sum() - n * mean * mean) / (n - 1)).clamp_min(0).sqrt() if adv.numel() > 1 else mean * 0)


@functools.lru_cache(maxsize=None)
def case(D, A, layers, n):
    """Inputs of one case, drawn on the CPU, and torch's float64 / float32 results on them (computed once, never changed).
    val and rew lie on a grid of 2^-10, so adv = rew - val and ret = adv + val are exact in float32 and the float32 and the
    float64 run of ppo_update see the same advantages, statistics and returns."""
    import train_vec
    g = torch.Generator().manual_seed(97 * D + 13 * A + 5 * layers + n)
    net = Net(D, A, layers, seed=1)
    obs = torch.randn(n, D, generator=g)
    net64 = Net(D, A, layers, seed=1).double()
    with torch.no_grad():
        mu64 = net64.mu(obs.double())
        act = (mu64 + net64.log_std.exp() * torch.randn(n, A, generator=g, dtype=torch.float64)).float()
        logp64, val64 = net64.logp_value(obs.double(), act.double())
        logp32, val32 = net.logp_value(obs, act)
    grid = 1.0 / 1024
    val0 = torch.round(val64.float() / grid) * grid
    rew = val0 + torch.round(torch.randn(n, generator=g) * 1.5 / grid) * grid
    logp_old = (logp64 + 0.3 * torch.randn(n, generator=g, dtype=torch.float64)).float()
    # no sample within 1e-3 of a clipping boundary (float64 alone decides): it would flip the branch of min between precisions
    ratio = (logp64 - logp_old.double()).exp()
    near = ((ratio - (1 - CLIP)).abs() < 1e-3) | ((ratio - (1 + CLIP)).abs() < 1e-3)
    assert float(near.double().mean()) < 0.02, "the boundary shift moves %d of %d samples" % (int(near.sum()), n)
    logp_old = torch.where(near, logp_old + 0.05, logp_old)
    ratio = (logp64 - logp_old.double()).exp()
    assert not bool((((ratio - (1 - CLIP)).abs() < 1e-3) | ((ratio - (1 + CLIP)).abs() < 1e-3)).any())
    adv = (rew - val0).double()
    mean, std = stats_of(adv)
    adv_n = ((adv - mean) / (std + 1e-8)).float().double()
    clipped = ratio.clamp(1 - CLIP, 1 + CLIP) * adv_n < ratio * adv_n            # min takes the clamped branch: no gradient
    # ---- ppo_update itself (epochs=1, SGD with lr 0) in float64 and in float32
    done = torch.ones(1, n, dtype=torch.uint8)                                      # K = 1, every episode ends: adv = rew - val
    grads = {}
    for name, m in (("f64", net64), ("f32", net)):
        dt = m.log_std.dtype
        shard = (torch.stack([obs, obs]).to(dt), act.to(dt).view(1, n, A), rew.to(dt).view(1, n), done)
        pi = FixedPrelude(m, logp_old, val0)
        train_vec.ppo_update(pi, torch.optim.SGD(m.parameters(), lr=0.0), [shard], epochs=1, clip=CLIP)
        grads[name] = {k: p.grad.detach().double().clone() for k, p in m.tensors().items()}
    return dict(net=net, obs=obs, act=act, logp_old=logp_old, adv=adv, ret=(rew - val0) + val0, mean=mean, std=std,
                logp64=logp64, val64=val64, logp32=logp32, val32=val32, grads=grads, clipped=float(clipped.double().mean()))


def rel_err(x, ref):
    return float((x.double().cpu() - ref).abs().max() / ref.abs().max())


@functools.lru_cache(maxsize=None)
def yardstick(D, A, layers):
    """torch float32's own error on the shape's n = 259 inputs: (forward, gradient), each the largest over its tensors."""
    c = case(D, A, layers, 259)
    fwd = max(rel_err(c["logp32"], c["logp64"]), rel_err(c["val32"], c["val64"]))
    grad = max(rel_err(c["grads"]["f32"][k], c["grads"]["f64"][k]) for k in c["grads"]["f64"])
    return fwd, grad


def split_grad(learner, net):
    out, off = {}, 0
    flat = learner.grad.detach().cpu()
    for k, p in net.tensors().items():
        out[k] = flat[off:off + p.numel()].view_as(p).clone()
        off += p.numel()
    assert off == flat.numel()
    return out


def run_gradients(learner, c, n_total=None, accumulate=False, **over):
    t = {k: (over[k] if k in over else c[k]) for k in ("obs", "act", "logp_old", "adv", "ret")}
    loss = learner.gradients(t["obs"].cuda(), t["act"].cuda(), t["logp_old"].cuda(), t["adv"].cuda(), t["ret"].cuda(),
                             over.get("mean", c["mean"]), over.get("std", c["std"]), clip=CLIP, vf_coef=0.5,
                             n_total=t["obs"].shape[0] if n_total is None else n_total, accumulate=accumulate)
    torch.cuda.synchronize()
    return learner.grad.detach().cpu().clone(), loss.detach().cpu().clone()


# ---------------------------------------------------------------------------------------------------------------- GAE
@pytest.mark.parametrize("K,R", [(1, 1), (7, 37), (100, 130)])
def test_gae_equals_torch_on_the_cpu_bit_for_bit(sim, K, R):
    import train_vec
    learner, _ = learner_of(sim, Net(3, 1, 1, seed=0))
    g = torch.Generator().manual_seed(K * 1000 + R)
    rew, val, last = torch.randn(K, R, generator=g), torch.randn(K, R, generator=g) * 3, torch.randn(R, generator=g) * 3
    done = torch.randint(0, 4, (K, R), generator=g).to(torch.uint8) * (torch.rand(K, R, generator=g) < 0.3).to(torch.uint8)
    done[0, 0], done[K - 1, R // 2] = 1, 2                                          # episodes ending at t = 0 and at t = K - 1
    if R > 1:
        done[K - 1, R - 1], done[0, 1] = 0, 3
    assert set(done.unique().tolist()) <= {0, 1, 2, 3} and (R < 37 or set(done.unique().tolist()) == {0, 1, 2, 3})
    adv_ref, ret_ref = train_vec.gae(rew, val, done, last)
    adv, ret = learner.gae(rew.cuda(), val.cuda(), last.cuda(), done.cuda())
    torch.cuda.synchronize()
    assert sim.last_kernel == "k_gae"
    assert torch.equal(adv.cpu(), adv_ref) and torch.equal(ret.cpu(), ret_ref)


# ------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("D,A,layers", SHAPES)
def test_forward_agrees_with_torch_float64(sim, D, A, layers, n):
    c = case(D, A, layers, n)
    learner, _ = learner_of(sim, c["net"])
    logp, val = learner.evaluate(c["obs"].cuda(), c["act"].cuda())
    val_only = learner.evaluate(c["obs"].cuda(), None)[1]
    torch.cuda.synchronize()
    assert sim.last_kernel == "k_ppo_eval"
    assert torch.equal(val, val_only)                                               # act=None: the same values
    e_logp, e_val, bound = rel_err(logp, c["logp64"]), rel_err(val, c["val64"]), MARGIN * yardstick(D, A, layers)[0]
    print("forward (%d, %d, %d) n=%d: kernel logp %.3g val %.3g; torch float32 (n=259) %.3g"
          % (D, A, layers, n, e_logp, e_val, yardstick(D, A, layers)[0]))
    assert e_logp <= bound and e_val <= bound


# ----------------------------------------------------------------------------------------------------------- gradient
def gradient_errors(sim, D, A, layers, n):
    c = case(D, A, layers, n)
    learner, net = learner_of(sim, c["net"])
    run_gradients(learner, c)
    got, ref = split_grad(learner, net), c["grads"]["f64"]
    return ({k: rel_err(got[k], ref[k]) for k in ref}, {k: rel_err(c["grads"]["f32"][k], ref[k]) for k in ref}, c)


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("D,A,layers", SHAPES)
def test_gradient_agrees_with_float64_autograd_of_ppo_update(sim, D, A, layers, n):
    kern, f32, c = gradient_errors(sim, D, A, layers, n)
    assert sim.last_kernel == "k_ppo_grad"
    assert 0.10 <= c["clipped"] <= 0.60, "%.0f %% of the samples are clipped" % (100 * c["clipped"])
    y = yardstick(D, A, layers)[1]
    worst = max(kern, key=kern.get)
    print("gradient (%d, %d, %d) n=%d: kernel %.3g (%s), torch float32 here %.3g, yardstick (n=259) %.3g, ratio %.2f"
          % (D, A, layers, n, kern[worst], worst, max(f32.values()), y, kern[worst] / y))
    for k, e in kern.items():
        assert e <= MARGIN * y, "%s: %.3g against 10 x %.3g" % (k, e, y)


def test_loss_sums_are_those_of_ppo_update(sim):
    c = case(65, 13, 3, 259)
    learner, _ = learner_of(sim, c["net"])
    _, loss = run_gradients(learner, c)
    net64 = Net(65, 13, 3, seed=1).double()
    with torch.no_grad():
        logp, v = net64.logp_value(c["obs"].double(), c["act"].double())
        adv_n = ((c["adv"] - c["mean"]) / (c["std"] + 1e-8)).float()
        ratio = (logp - c["logp_old"]).exp()
        pg = torch.min(ratio * adv_n, ratio.clamp(1 - CLIP, 1 + CLIP) * adv_n).sum()
        vf = (v - c["ret"]).pow(2).sum()
    assert abs(float(loss[0]) - float(pg)) <= 1e-4 * 259 and abs(float(loss[1]) - float(vf)) <= 1e-5 * float(vf)


# ------------------------------------------------------------------------------------------------------ absent agents
def test_absent_agents_add_nothing_and_nan_reaches_no_output(sim):
    D, A, layers, n = 65, 13, 3, 259
    c = case(D, A, layers, n)
    learner, net = learner_of(sim, c["net"])
    g = torch.Generator().manual_seed(5)
    absent = torch.rand(n, generator=g) < 0.2
    absent[64:128] = True                                                           # one whole 64-sample tile
    assert 0.25 <= float(absent.double().mean()) <= 0.5
    act = c["act"].clone()
    col = torch.randint(0, A, (n,), generator=g)
    act[absent, col[absent]] = float("nan")                                         # one NaN in the row is enough
    n_present = int((~absent).sum())
    a, la = run_gradients(learner, c, n_total=n_present, act=act)
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(la).all())
    # (a) the same bits whatever else the absent rows hold: NaN observations, NaN advantages, other numbers
    nan = float("nan")
    obs2, lp2, adv2, ret2 = c["obs"].clone(), c["logp_old"].clone(), c["adv"].clone(), c["ret"].clone()
    obs2[absent], lp2[absent], adv2[absent], ret2[absent] = nan, nan, nan, 7.0
    act2 = act.clone()
    act2[absent] = nan
    b, lb = run_gradients(learner, c, n_total=n_present, act=act2, obs=obs2, logp_old=lp2, adv=adv2, ret=ret2)
    assert torch.equal(a, b) and torch.equal(la, lb)
    # (b) torch float64 on the present rows alone
    import train_vec
    keep = ~absent
    net64 = Net(D, A, layers, seed=1).double()
    shard = (torch.stack([c["obs"][keep], c["obs"][keep]]).double(), c["act"][keep].double().view(1, n_present, A),
             c["ret"][keep].double().view(1, n_present), torch.ones(1, n_present, dtype=torch.uint8))
    # (ret = rew on these inputs, val = ret - adv; ppo_update takes its statistics from the present rows: the kernel gets them)
    pi = FixedPrelude(net64, c["logp_old"][keep], (c["ret"].double() - c["adv"])[keep])
    ref_mean, ref_std = stats_of(c["adv"][keep])
    a2, _ = run_gradients(learner, c, n_total=n_present, act=act, mean=ref_mean, std=ref_std)
    train_vec.ppo_update(pi, torch.optim.SGD(net64.parameters(), lr=0.0), [shard], epochs=1, clip=CLIP)
    learner.grad.copy_(a2.cuda())
    got, y = split_grad(learner, net), yardstick(D, A, layers)[1]
    for k, p in net64.tensors().items():
        e = rel_err(got[k], p.grad.detach())
        assert e <= MARGIN * y, "%s: %.3g against 10 x %.3g" % (k, e, y)
    # (c) a whole absent tile inserted into a batch changes no bit of its gradient (the order of the sum survives)
    small = {k: c[k][keep][:192] for k in ("obs", "act", "logp_old", "adv", "ret")}
    ins = {k: torch.cat([v[:64], torch.full_like(v[:64], nan if k == "act" else 3.0), v[64:]]) for k, v in small.items()}
    s0, ls0 = run_gradients(learner, c, n_total=192, **small)
    s1, ls1 = run_gradients(learner, c, n_total=192, **ins)
    assert torch.equal(s0, s1) and torch.equal(ls0, ls1)
    # the forward pass: the present rows' outputs do not depend on the absent ones
    lp_a, v_a = learner.evaluate(c["obs"].cuda(), act.cuda())
    lp_0, v_0 = learner.evaluate(c["obs"].cuda(), c["act"].cuda())
    assert torch.equal(lp_a[keep.cuda()], lp_0[keep.cuda()]) and torch.equal(v_a, v_0)


# -------------------------------------------------------------------------------------------------------- determinism
def test_the_same_inputs_give_the_same_bits_and_shards_accumulate_in_call_order(sim):
    c1, c2 = case(141, 20, 2, 259), case(141, 20, 2, 64)
    learner, _ = learner_of(sim, c1["net"])
    a, la = run_gradients(learner, c1, n_total=323)
    learner.grad.fill_(float("nan"))                                                # (accumulate=False overwrites)
    b, lb = run_gradients(learner, c1, n_total=323)
    assert torch.equal(a, b) and torch.equal(la, lb)
    s2, l2 = run_gradients(learner, c2, n_total=323)
    run_gradients(learner, c1, n_total=323)
    acc, lacc = run_gradients(learner, c2, n_total=323, accumulate=True)
    assert torch.equal(acc, (a.cuda() + s2.cuda()).cpu()) and torch.equal(lacc, (la.cuda() + l2.cuda()).cpu())
    fresh, _ = learner_of(sim, c1["net"])                                           # the same two calls on a zeroed buffer
    run_gradients(fresh, c1, n_total=323, accumulate=True)
    acc2, lacc2 = run_gradients(fresh, c2, n_total=323, accumulate=True)
    assert torch.equal(acc, acc2) and torch.equal(lacc, lacc2)


def test_grad_views_feed_the_torch_optimiser(sim):
    c = case(28, 1, 1, 64)
    learner, net = learner_of(sim, c["net"])
    run_gradients(learner, c)
    learner.attach_grads()
    for p in learner.params:
        assert p.grad.data_ptr() >= learner.grad.data_ptr() and p.grad.shape == p.shape
    before = learner.weights.clone()
    torch.optim.SGD(learner.params, lr=0.5).step()
    learner.sync()
    torch.cuda.synchronize()
    assert torch.equal(learner.weights, before - 0.5 * learner.grad)


# ------------------------------------------------------------------------------------------------------------ trainer
@pytest.mark.parametrize("device_update", [True, False])
def test_train_on_device_with_and_without_the_device_update(monkeypatch, device_update):
    import train_vec
    from flow_amd.envs import VecFlowEnv
    from flow_amd.utils.device_ppo import DeviceLearner
    seen, calls = [], []
    close, gradients = VecFlowEnv.close, DeviceLearner.gradients

    def closing(self):
        seen.append(self.sim.last_kernel)            # nothing launches on the handle after the last update
        return close(self)

    def counting(self, *a, **kw):
        calls.append(1)
        return gradients(self, *a, **kw)
    monkeypatch.setattr(VecFlowEnv, "close", closing)
    monkeypatch.setattr(DeviceLearner, "gradients", counting)
    hist = train_vec.train_on_device(train_vec.ring_flow_params(20), replicas=64, fragment=8, iterations=2,
                                     device_update=device_update, log=lambda *a: None)
    assert len(hist) == 2 and all(np.isfinite(h) for h in hist)
    if device_update:
        assert seen == ["k_ppo_grad"] and len(calls) == 2 * 4
    else:
        assert len(calls) == 0 and len(seen) == 1 and not seen[0].startswith("k_ppo") and seen[0] != "k_gae"
