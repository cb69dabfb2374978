"""The rest of the PPO update on the device (flow_amd/csrc/flowsim_learn.h: k_adv_stats, k_adv_finish, k_ppo_grad with the
sample count on the device, k_adam; DeviceLearner.adopt_parameters / adam_step / update, DevicePolicy.share), on the
float32 2-replica ring handle of tests/test_device_ppo_gpu.py.

* fs_adam_dev equals the numpy restatement of its operation sequence (tests/device_adam_ref.py) bit for bit, and is as
  close to torch float64 Adam as torch float32 is (error over displacement, MARGIN = 10 times torch float32's own);
* fs_adv_stats_dev: exact count, each sum within n 2^-52 sum|term| of the CPU float64 sum (the bound for a double sum of n
  float32-valued terms in any order), adv64 the exact copy, the same bits on every call, shards accumulated in call order,
  absent rows (NaN action rows) selected out whatever they hold; fs_adv_finish_dev equals numpy bit for bit;
* fs_ppo_grad_n_dev equals fs_ppo_grad_dev with inv_n_total = 1 / n bit for bit;
* adopted parameters live in learner.weights, a sharing DevicePolicy acts with the same bits as a synced one;
* update() equals its stages called one by one, stays within MARGIN times float32 torch ppo_update's own error of float64
  ppo_update, and replays from a captured graph with the bits of eager calls;
* train_on_device(device_adam=True) trains without torch's Adam and without ppo_update."""
import copy
import functools
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
from test_device_ppo_gpu import CLIP, MARGIN, Net, case, learner_of  # noqa: E402

pytestmark = pytest.mark.gpu

assert MARGIN == ref.MARGIN


@pytest.fixture(scope="module")
def sim():
    from flow_amd.sim import FlowSim
    s = FlowSim(ring_spec(R=2, N=5, bunching=0), "f32")
    yield s
    s.close()


def bind(sim):
    """The raw entry points launch on the handle's stream: torch's current one, where their tensors are produced."""
    sim.set_stream(torch.cuda.current_stream().cuda_stream)


def packed(D, A, layers):
    net = 32 * D + 32 + (layers - 1) * 1056
    return (net + 33 * A) + A + (net + 33)


# --------------------------------------------------------------------------------------------------------------- Adam
def device_adam(sim, w0, grads, snapshots):
    """fs_adam_dev over the gradients from a fresh state: {step: (w, m, v, state)} as numpy, for the steps asked for."""
    from flow_amd import _lib as L
    P = int(w0.size)
    w = torch.from_numpy(w0.copy()).cuda()
    m, v = torch.zeros_like(w), torch.zeros_like(w)
    state = torch.tensor(ref.fresh_state(), dtype=torch.float64).cuda()
    gs = [torch.from_numpy(x).cuda() for x in grads]
    bind(sim)
    out = {}
    for k, g in enumerate(gs, 1):
        L.check(sim.lib.fs_adam_dev(sim._h, P, w.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), state.data_ptr(),
                                    ref.LR, ref.BETAS[0], ref.BETAS[1], ref.EPS), sim.lib)
        if k in snapshots:
            torch.cuda.synchronize()
            out[k] = tuple(t.cpu().numpy().copy() for t in (w, m, v, state))
    assert sim.last_kernel == "k_adam"
    return out


@pytest.mark.parametrize("P", [1, 259, packed(3, 1, 2), packed(160, 32, 3)])
def test_adam_equals_the_numpy_restatement_bit_for_bit(sim, P):
    assert packed(3, 1, 2) == 2435 and packed(160, 32, 3) == 15649
    g = torch.Generator().manual_seed(P)
    w0 = torch.randn(P, generator=g).numpy()
    grads = [x.numpy() for x in ref.draw_gradients(P, 10, seed=P + 1)]
    if P == 1:
        grads[0][0], grads[1][0] = 0.0, 3e-4                # (element 0 of every seventh is zero throughout: move this one)
        for x in grads[2:]:
            x[0] = -0.02
    assert (grads[0] == 0).any()
    want, got = ref.run_adam_ref(w0, grads), device_adam(sim, w0, grads, (1, 2, 10))
    for k in (1, 2, 10):
        for name, a, b in zip(("w", "m", "v", "state"), got[k], want[k - 1]):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), \
                "step %d, %s: %d of %d elements differ" % (k, name, int((a != b).sum()), a.size)
    assert got[10][3][0] == 10.0
    assert P == 1 or not np.array_equal(got[10][0], w0)


@pytest.mark.parametrize("P", [7, 259, 4000])
def test_adam_is_as_close_to_float64_adam_as_torch_float32(sim, P):
    c = ref.adam_problem(P)
    w = device_adam(sim, c["w0"], c["grads"], (10,))[10][0]
    err = ref.displacement_error(w, c["w64"], c["w0"])
    print("Adam P=%d: kernel %.3g, torch float32 %.3g (ratio %.2f)" % (P, err, c["err32"], err / c["err32"]))
    assert err <= MARGIN * c["err32"]


# --------------------------------------------------------------------------------------------------------- statistics
COUNTS = [5, 64, 259, 4099]


@functools.lru_cache(maxsize=None)
def adv_case(n, A=3):
    g = torch.Generator().manual_seed(7 * n + A)
    adv = torch.randn(n, generator=g) * 3 + 0.7
    act = torch.randn(n, A, generator=g)
    absent = torch.rand(n, generator=g) < 0.25
    absent[0], absent[n - 1], absent[n // 2] = True, False, True
    holed = act.clone()
    holed[absent, torch.randint(0, A, (n,), generator=g)[absent]] = float("nan")       # one NaN in the row is enough
    return adv, act, holed, absent


def cpu_sums(adv, keep=None):
    a = adv.double() if keep is None else adv.double()[keep]
    return a.sum().item(), (a * a).sum().item(), float(a.numel()), a.abs().sum().item(), (a * a).sum().item()


def stats_of(learner, adv, act=None, **kw):
    adv64, stats = learner.adv_stats(adv.cuda(), None if act is None else act.cuda(), **kw)
    torch.cuda.synchronize()
    return adv64.cpu(), stats.cpu()


def check_sums(stats, adv, keep, n):
    s0, s1, cnt, abs0, abs1 = cpu_sums(adv, keep)
    eps = 2.0 ** -52
    assert stats[2].item() == cnt
    print("n=%d: sum %.17g (cpu %.17g, bound %.3g), squares %.17g (cpu %.17g, bound %.3g)"
          % (n, stats[0].item(), s0, n * eps * abs0, stats[1].item(), s1, n * eps * abs1))
    assert abs(stats[0].item() - s0) <= n * eps * abs0
    assert abs(stats[1].item() - s1) <= n * eps * abs1


# (4099: five workgroups; 300001: 293 of them, past the 256 lanes of the workgroup that adds the partial sums)
@pytest.mark.parametrize("n", COUNTS + [300001])
def test_adv_stats_against_float64_on_the_cpu(sim, n):
    learner, _ = learner_of(sim, Net(3, 3, 1, seed=0))
    adv, act, holed, absent = adv_case(n)
    for a in (None, act):                                                           # every row present, both forms
        adv64, stats = stats_of(learner, adv, a)
        assert sim.last_kernel == "k_adv_stats"
        assert adv64.dtype == torch.float64 and torch.equal(adv64, adv.double())
        check_sums(stats, adv, None, n)
    again64, again = stats_of(learner, adv, act)                                    # the same inputs, the same bits
    assert torch.equal(again, stats) and torch.equal(again64, adv64)
    # ---- absent rows: selected out, whatever they hold
    keep = ~absent
    a64, st = stats_of(learner, adv, holed)
    check_sums(st, adv, keep, n)
    assert torch.equal(a64[keep], adv.double()[keep]) and bool(torch.isfinite(a64).all())
    adv2, act2 = adv.clone(), holed.clone()
    adv2[absent] = float("nan")
    adv2[0] = float("inf")
    act2[absent] = float("nan")
    b64, st2 = stats_of(learner, adv2, act2)
    assert torch.equal(st2, st) and torch.equal(b64, a64)
    adv3 = adv.clone()
    adv3[absent] = 1e30
    c64, st3 = stats_of(learner, adv3, holed)
    assert torch.equal(st3, st) and torch.equal(c64, a64)


def test_adv_stats_accumulate_over_shards_in_call_order(sim):
    learner, _ = learner_of(sim, Net(3, 3, 1, seed=0))
    (adv1, _, holed1, _), (adv2, act2, _, _) = adv_case(259), adv_case(4099)
    _, s1 = stats_of(learner, adv1, holed1)
    _, s2 = stats_of(learner, adv2, act2)
    stats = torch.full((3,), float("nan"), dtype=torch.float64).cuda()              # (accumulate=False overwrites)
    stats_of(learner, adv1, holed1, stats=stats)
    _, both = stats_of(learner, adv2, act2, accumulate=True, stats=stats)
    assert torch.equal(both, s1 + s2)
    assert both[2].item() == s1[2].item() + 4099


@pytest.mark.parametrize("n", COUNTS)
def test_adv_finish_equals_numpy_bit_for_bit(sim, n):
    learner, _ = learner_of(sim, Net(3, 3, 1, seed=0))
    adv, _, holed, _ = adv_case(n)
    for a in (None, holed):
        _, stats = learner.adv_stats(adv.cuda(), None if a is None else a.cuda())
        out = learner.adv_finish(stats)
        torch.cuda.synchronize()
        assert sim.last_kernel == "k_adv_finish"
        want = ref.finish_ref(stats.cpu().numpy())
        assert out.cpu().numpy().tobytes() == want.tobytes(), (out.cpu().numpy(), want)
        assert want[1] > 0 and want[2] == stats[2].item()


# ----------------------------------------------------------------------------------------- the gradient, n on the device
@pytest.mark.parametrize("absent_rows", [False, True])
@pytest.mark.parametrize("D,A,layers", [(3, 1, 2), (141, 20, 2)])
def test_grad_n_equals_grad_bit_for_bit(sim, D, A, layers, absent_rows):
    n = 259
    c = case(D, A, layers, n)
    learner, _ = learner_of(sim, c["net"])
    act = c["act"].clone()
    count = n
    if absent_rows:
        g = torch.Generator().manual_seed(11)
        absent = torch.rand(n, generator=g) < 0.3
        act[absent, 0] = float("nan")
        count = int((~absent).sum())
        assert 0 < count < n
    t = [c[k].cuda() for k in ("obs",)] + [act.cuda()] + [c[k].cuda() for k in ("logp_old", "adv", "ret")]
    loss = learner.gradients(*t, c["mean"], c["std"], clip=CLIP, vf_coef=0.5, n_total=count)
    torch.cuda.synchronize()
    g0, l0 = learner.grad.clone(), loss.clone()
    learner.grad.fill_(float("nan"))
    learner.loss.fill_(float("nan"))
    msn = torch.tensor([float(c["mean"]), float(c["std"]), float(count)], dtype=torch.float64).cuda()
    loss = learner.gradients_n(*t, msn, clip=CLIP, vf_coef=0.5)
    torch.cuda.synchronize()
    assert sim.last_kernel == "k_ppo_grad"
    assert bool(torch.isfinite(g0).all()) and float(g0.abs().max()) > 0
    assert torch.equal(learner.grad, g0) and torch.equal(loss, l0)


# ----------------------------------------------------------------------------------------------------------- adoption
def test_adopted_parameters_live_in_the_packed_weights_and_torch_reads_them(sim):
    c = case(3, 1, 2, 64)
    learner, net = learner_of(sim, c["net"])
    obs = c["obs"].cuda()
    with torch.no_grad():
        y_old = net.mu(obs).clone()
    learner.adopt_parameters()
    before = learner.weights.clone()
    with torch.no_grad():
        assert torch.equal(net.mu(obs), y_old)              # adoption itself moves no value
    learner.grad.copy_(torch.randn(learner.P, generator=torch.Generator().manual_seed(1)).cuda())
    learner.adam_step(lr=1e-2)
    torch.cuda.synchronize()
    assert sim.last_kernel == "k_adam" and not torch.equal(learner.weights, before)
    lo, off = learner.weights.data_ptr(), 0
    for p in learner.params:
        assert p.data_ptr() == lo + 4 * off and lo <= p.data_ptr() < lo + 4 * learner.P
        assert torch.equal(p.detach().reshape(-1), learner.weights[off:off + p.numel()])
        off += p.numel()
    assert off == learner.P and [id(p) for p in learner.params] == [id(p) for p in net.tensors().values()]
    # a torch forward pass uses the new values: those of a module built from a host copy of the packed weights
    fresh = Net(3, 1, 2, seed=9).cuda()
    host, off = learner.weights.cpu(), 0
    with torch.no_grad():
        for q in fresh.tensors().values():
            q.copy_(host[off:off + q.numel()].view_as(q))
            off += q.numel()
        y_new = net.mu(obs)
        assert torch.equal(y_new, fresh.mu(obs)) and not torch.equal(y_new, y_old)
        assert torch.equal(net.value(obs), fresh.value(obs))
    learner.sync()                                          # (nothing to move)
    assert torch.equal(learner.weights.cpu(), host)


def test_a_sharing_policy_gives_the_bits_of_a_synced_one():
    """policy_act draws from the replicas' Philox streams, keyed by the policy's seed and the handle's draw counter: two
    handles in the same state, one per policy, see the same draws."""
    import train_vec
    from flow_amd.envs import VecFlowEnv
    from flow_amd.utils.device_policy import DevicePolicy
    from flow_amd.utils.device_ppo import DeviceLearner
    outs = []
    for share in (True, False):
        torch.manual_seed(3)
        vec = VecFlowEnv(train_vec.ring_flow_params(20), num_replicas=64, device=0)
        try:
            pi = train_vec.GaussianPolicy(vec.obs_dim, vec.act_dim).cuda()
            learner = DeviceLearner(vec, [pi.mu[0], pi.mu[2]], pi.mu[4], pi.log_std, [pi.value[0], pi.value[2]], pi.value[4])
            learner.adopt_parameters()
            learner.grad.copy_(torch.randn(learner.P, generator=torch.Generator().manual_seed(1)).cuda())
            learner.adam_step(lr=1e-2)
            pol = DevicePolicy([pi.mu[0], pi.mu[2]], pi.mu[4], log_std=pi.log_std, seed=5)
            if share:
                pol.share(learner)
                assert pol.struct.weights_dev == learner.weights.data_ptr()
            else:
                assert pol.struct.weights_dev != learner.weights.data_ptr()
            obs = vec.reset()
            act, logp = vec.policy_act(pol, obs)
            torch.cuda.synchronize()
            outs.append((obs.cpu().clone(), act.cpu().clone(), logp.cpu().clone(), learner.weights.cpu().clone()))
        finally:
            vec.close()
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(outs[0][1]).all())


# ------------------------------------------------------------------------------------------------------------ update()
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


def test_update_equals_its_stages_called_one_by_one(sim):
    D, A, layers, K, R = 65, 13, 3, 8, 16
    net = Net(D, A, layers, seed=2)
    shards = [fragment(D, A, K, R, 1, net), fragment(D, A, 5, 7, 2, net)]
    shards[1][1][2, 3, 1] = float("nan")                                            # an absent agent in the second shard
    whole, _ = learner_of(sim, net)
    whole.adopt_parameters()
    whole.update([on_gpu(s) for s in shards], epochs=4)
    torch.cuda.synchronize()
    assert sim.last_kernel == "k_adam"
    steps, _ = learner_of(sim, net)
    steps.adopt_parameters()
    prepared, stats = [], torch.zeros(3, dtype=torch.float64).cuda()
    for j, (obs, act, rew, done) in enumerate(on_gpu(s) for s in shards):
        k, r = rew.shape
        o, a = obs[:k].reshape(k * r, D), act.reshape(k * r, A)
        logp, val = steps.evaluate(o, a)
        last = steps.evaluate(obs[k], None)[1]
        adv, ret = steps.gae(rew, val.view(k, r), last, done)
        adv64, _ = steps.adv_stats(adv, a, accumulate=j > 0, stats=stats)
        prepared.append((o, a, logp, adv64, ret.reshape(-1)))
    msn = steps.adv_finish(stats)
    for _ in range(4):
        for j, p in enumerate(prepared):
            steps.gradients_n(*p, msn, clip=0.2, vf_coef=0.5, accumulate=j > 0)
        steps.adam_step(lr=3e-4, betas=(0.9, 0.999), eps=1e-8)
    torch.cuda.synchronize()
    assert msn[2].item() == 8 * 16 + 5 * 7 - 1
    for name in ("weights", "grad", "loss", "m", "v", "state"):
        assert torch.equal(getattr(whole, name), getattr(steps, name)), name
    assert whole.state[0].item() == 4 and not torch.equal(whole.weights, learner_of(sim, net)[0].weights)


def flat(net):
    return torch.cat([p.detach().reshape(-1) for p in net.tensors().values()]).double().numpy()


@functools.lru_cache(maxsize=None)
def update_problem(D, A, layers):
    """A fragment of 8 x 16 samples and train_vec.ppo_update's result on it after 4 epochs, by torch on the CPU in float64
    and in float32 (computed once)."""
    import train_vec
    K, R = 8, 16
    net = Net(D, A, layers, seed=3)
    shard = fragment(D, A, K, R, 17 * D + A, net)
    w0, out = flat(net), {}
    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        m = copy.deepcopy(net).to(dt)
        sh = (shard[0].to(dt), shard[1].to(dt), shard[2].to(dt), shard[3])
        train_vec.ppo_update(m, torch.optim.Adam(m.parameters(), lr=ref.LR), [sh], epochs=4, clip=0.2)
        out[name] = flat(m)
    return net, shard, w0, out["f64"], ref.displacement_error(out["f32"], out["f64"], w0)


@pytest.mark.parametrize("D,A,layers", [(3, 1, 2), (65, 13, 3)])
def test_update_stays_within_float32_torch_of_float64_ppo_update(sim, D, A, layers):
    net, shard, w0, w64, err32 = update_problem(D, A, layers)
    learner, _ = learner_of(sim, net)
    learner.adopt_parameters()
    learner.update([on_gpu(shard)], epochs=4, clip=0.2, lr=ref.LR)
    torch.cuda.synchronize()
    err = ref.displacement_error(learner.weights.cpu().numpy(), w64, w0)
    print("update (%d, %d, %d): kernels %.3g, torch float32 %.3g (ratio %.2f), displacement %.3g"
          % (D, A, layers, err, err32, err / err32, float(np.abs(w64 - w0).max())))
    assert err <= MARGIN * err32


# ------------------------------------------------------------------------------------------------------------- capture
def test_update_replays_from_a_graph_with_the_bits_of_eager_calls(sim):
    D, A, layers = 3, 1, 2
    net, shard, _, _, _ = update_problem(D, A, layers)
    learner, _ = learner_of(sim, net)
    learner.adopt_parameters()
    shard = on_gpu(shard)
    start = learner.weights.clone()

    def rewind():
        learner.weights.copy_(start)
        learner.m.zero_()
        learner.v.zero_()
        learner.state.copy_(torch.tensor(ref.fresh_state(), dtype=torch.float64))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        learner.update([shard], epochs=4)                   # the eager warm-up, on the capture stream: the handle is bound
        side.synchronize()                                  # to it (fs_set_stream synchronises) and every buffer exists
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        learner.update([shard], epochs=4)
    torch.cuda.synchronize()
    rewind()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert learner.state[0].item() == 8
    replayed = {k: getattr(learner, k).clone() for k in ("weights", "m", "v", "state", "grad", "loss")}
    assert not torch.equal(replayed["weights"], start)
    rewind()
    learner.update([shard], epochs=4)
    learner.update([shard], epochs=4)
    torch.cuda.synchronize()
    assert learner.state[0].item() == 8
    for k, want in replayed.items():
        assert torch.equal(getattr(learner, k), want), k


# ------------------------------------------------------------------------------------------------------------ trainer
NEW = ("update", "adam_step", "_adv_stats", "adv_finish", "_grad_n", "adopt_parameters")


@pytest.mark.parametrize("device_adam", [True, False])
def test_train_on_device_with_and_without_device_adam(monkeypatch, device_adam):
    import train_vec
    from flow_amd.utils.device_policy import DevicePolicy
    from flow_amd.utils.device_ppo import DeviceLearner
    calls = []

    def counted(cls, name):
        real = getattr(cls, name)

        def fn(self, *a, **kw):
            calls.append(name)
            return real(self, *a, **kw)
        monkeypatch.setattr(cls, name, fn)
    for name in NEW:
        counted(DeviceLearner, name)
    counted(DevicePolicy, "share")
    if device_adam:
        def refuse(*a, **kw):
            raise AssertionError("the torch update ran under device_adam")
        monkeypatch.setattr(torch.optim.Adam, "step", refuse)
        monkeypatch.setattr(train_vec, "ppo_update", refuse)
    hist = train_vec.train_on_device(train_vec.ring_flow_params(20), replicas=64, fragment=20, iterations=2,
                                     device_update=True, device_adam=device_adam, log=lambda *a: None)
    assert len(hist) == 2 and all(np.isfinite(h) for h in hist)
    if device_adam:
        assert calls.count("update") == 2 and calls.count("adam_step") == 2 * 4 and calls.count("_grad_n") == 2 * 4
        assert calls.count("adopt_parameters") == 1 and calls.count("share") == 1
    else:
        assert calls == []                                  # none of the new entry points without the flag
