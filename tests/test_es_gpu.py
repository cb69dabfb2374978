"""Evolution strategies on the device (include/flowsim.h fs_es_*; flow_amd/csrc/flowsim_es.h; flow_amd/utils/device_es.py).

* k_es_perturb equals numpy float32 built from oracle.refsim.gaussian_noise(exact=True), bit for bit;
* k_es_fitness equals a float64 numpy loop bit for bit (done at k = 0, never, in the second of two accumulated fragments);
* k_es_weights equals the numpy restatements (centered ranks with exact ties, ARS with top < N, ARS with equal returns);
* k_es_grad is within the float32 summation bound (N + 2) 2^-24 sum_p |u_p eps(p, e)| of the float64 sum and repeats
  its bits;
* DeviceES: two generations on a 128-replica singleagent_ring equal a numpy restatement fed with the device's fit_dev,
  and a state_dict round trip taken in the middle reproduces the second generation."""
import os
import sys

import numpy as np
import pytest

from oracle import refsim as S
from device_adam_ref import adam_ref
from test_ringrl_gpu import make, rl_ring_spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SEED = 0x123456789ABCDEF
COLUMN = 0x60000000


def eps_ref(N, P, generation, seed=SEED):
    """eps [N, P] float32: gauss<float>(seed, replica = p, vehicle = 0x60000000 | generation, step = e, exact)."""
    p = np.broadcast_to(np.arange(N, dtype=np.uint32)[:, None], (N, P)).copy()
    e = np.broadcast_to(np.arange(P, dtype=np.uint32)[None, :], (N, P)).copy()
    col = np.full((N, P), COLUMN | generation, np.uint32)
    return S.gaussian_noise(seed, p, col, e, np.float32, exact=True).astype(np.float32)


@pytest.fixture(scope="module")
def sim():
    s = make(rl_ring_spec(R=64, N=22, seed=1), "f32")
    s.reset()
    yield s
    s.close()


def dev_tensor(x):
    import torch
    t = torch.as_tensor(np.ascontiguousarray(x)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def check(sim, rc):
    from flow_amd import _lib as L
    L.check(rc, sim.lib)


@pytest.mark.parametrize("P", [2306, 7])
def test_perturb_equals_numpy_bit_for_bit(sim, P):
    import torch
    N, E, sigma = 3, 2, np.float32(0.02)
    M, stride = 2 * N + E, P + 3
    theta = np.random.default_rng(P).normal(0, 0.5, P).astype(np.float32)
    th = dev_tensor(theta)
    got = []
    for gen in (0, 1):
        w = torch.full((M, stride), -7.0, device="cuda:0")
        torch.cuda.synchronize()
        check(sim, sim.lib.fs_es_perturb_dev(sim._h, P, N, E, stride, th.data_ptr(), float(sigma), SEED, gen, w.data_ptr()))
        sim.sync()
        assert sim.last_kernel == "k_es_perturb"
        w = w.cpu().numpy()
        t = (sigma * eps_ref(N, P, gen)).astype(np.float32)
        np.testing.assert_array_equal(w[0:2 * N:2, :P], theta[None, :] + t)
        np.testing.assert_array_equal(w[1:2 * N:2, :P], theta[None, :] - t)
        np.testing.assert_array_equal(w[2 * N:, :P], np.tile(theta, (E, 1)))       # the evaluation rows are theta
        assert (w[:, P:] == -7.0).all()                                              # the padding is left alone
        # the pairs are antithetic: their midpoint is theta up to the two additions' roundings
        mid = (w[0:2 * N:2, :P].astype(np.float64) + w[1:2 * N:2, :P]) / 2
        assert (np.abs(mid - theta[None, :]) <= 2.0 ** -23 * (np.abs(theta[None, :]) + np.abs(t))).all()
        got.append(w)
    assert not np.array_equal(got[0][:2 * N], got[1][:2 * N])                       # the generations differ
    for a in range(N):
        for b in range(a + 1, N):
            assert not np.array_equal(got[0][2 * a, :P], got[0][2 * b, :P])         # the directions differ


def fitness_ref(rew, done, group, ret, alive):
    K, R = rew.shape
    ret, alive = ret.copy(), alive.copy()
    for r in range(R):
        for k in range(K):
            if alive[r]:
                ret[r] = ret[r] + np.float64(rew[k, r])
                if done[k, r] != 0:
                    alive[r] = 0
    fit = np.zeros(R // group, np.float64)
    for m in range(R // group):
        s = np.float64(0.0)
        for r in range(m * group, (m + 1) * group):
            s = s + ret[r]
        fit[m] = s / np.float64(group)
    return ret, alive, fit


def test_fitness_equals_the_float64_loop_bit_for_bit(sim):
    import torch
    K, R, group = 5, 64, 16
    rng = np.random.default_rng(3)
    rews = [rng.normal(1.0, 2.0, (K, R)).astype(np.float32) * np.float32(1.0 + 1e-3 * k) for k in range(2)]
    dones = [np.zeros((K, R), np.uint8), np.zeros((K, R), np.uint8)]
    dones[0][0, 0:8] = 1                                       # done at k = 0
    dones[0][3, 8:20] = 2                                      # a collision byte ends an episode too
    dones[0][4, 20:24] = 1
    dones[0][1, 3] = 1                                         # (a second done of a dead replica: ignored)
    dones[1][2, 24:40] = 1                                     # done in the second of two accumulated fragments
    dones[1][0, 0:4] = 1                                       # (dead since the first fragment)
    #                                                            replicas 40 .. 63: done never
    ret_d = torch.full((R,), 99.0, dtype=torch.float64, device="cuda:0")           # (accumulate = 0 ignores what is there)
    alive_d = torch.zeros(R, dtype=torch.uint8, device="cuda:0")
    fit_d = torch.zeros(R // group, dtype=torch.float64, device="cuda:0")
    ret, alive = np.zeros(R, np.float64), np.ones(R, np.uint8)
    for i in range(2):
        rw, dn = dev_tensor(rews[i]), dev_tensor(dones[i])
        check(sim, sim.lib.fs_es_fitness_dev(sim._h, K, R // group, group, rw.data_ptr(), dn.data_ptr(), i, ret_d.data_ptr(),
                                             alive_d.data_ptr(), fit_d.data_ptr()))
        sim.sync()
        assert sim.last_kernel == "k_es_fitness"
        ret, alive, fit = fitness_ref(rews[i], dones[i], group, ret, alive)
        np.testing.assert_array_equal(ret_d.cpu().numpy(), ret)
        np.testing.assert_array_equal(alive_d.cpu().numpy(), alive)
        np.testing.assert_array_equal(fit_d.cpu().numpy(), fit)
    assert alive[:40].sum() == 0 and alive[40:].all()


def weights_on_device(sim, mode, fit, N, E, top=0):
    import torch
    f = dev_tensor(np.asarray(fit, np.float64))
    u = torch.full((N,), 7.0, device="cuda:0")
    stats = torch.zeros(4, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    check(sim, sim.lib.fs_es_weights_dev(sim._h, mode, N, E, top, f.data_ptr(), u.data_ptr(), stats.data_ptr()))
    sim.sync()
    assert sim.last_kernel == "k_es_weights"
    return u.cpu().numpy(), stats.cpu().numpy()


def stats_ref(fit, N, E):
    s = np.float64(0.0)
    for x in fit[:2 * N]:
        s = s + x
    se = np.float64(0.0)
    for x in fit[2 * N:2 * N + E]:
        se = se + x
    return np.array([s / np.float64(2 * N), fit[:2 * N].min(), fit[:2 * N].max(), se / np.float64(E)], np.float64)


def test_direction_weights_equal_numpy_bit_for_bit(sim):
    from flow_amd import _lib as L
    from flow_amd.utils.device_es import ars_weights_ref, centered_ranks_ref
    rng = np.random.default_rng(11)
    N, E = 37, 3
    fit = rng.normal(50.0, 10.0, 2 * N + E)
    fit[5] = fit[40] = fit[41] = fit[2]                        # exact ties: broken by the index
    fit[10] = fit[11]                                          # a tie inside a pair: the smaller index ranks lower
    u, st = weights_on_device(sim, L.FS_ES_MODE_ES, fit, N, E)
    np.testing.assert_array_equal(u, centered_ranks_ref(fit[:2 * N]))
    np.testing.assert_array_equal(st, stats_ref(fit, N, E))
    assert u[5] < 0                                            # (the pair (10, 11) is tied: 10 ranks below 11)
    # ARS with top < N, with a tie of the keys at the cut (the smaller p is kept)
    fit2 = fit.copy()
    key = np.maximum(fit2[0:2 * N:2], fit2[1:2 * N:2])
    order = sorted(range(N), key=lambda p: (-key[p], p))
    top = 9
    a, b = sorted((order[top - 1], order[top]))
    fit2[2 * b], fit2[2 * b + 1] = key[a], key[a] - 1.0        # direction b now ties direction a's key
    for t in (top, N, 0, 1):
        u, st = weights_on_device(sim, L.FS_ES_MODE_ARS, fit2, N, E, top=t)
        want = ars_weights_ref(fit2[:2 * N], t)
        np.testing.assert_array_equal(u, want)
        assert (u != 0).sum() <= (N if t in (0, N) else t)
    u, _ = weights_on_device(sim, L.FS_ES_MODE_ARS, fit2, N, E, top=top)
    assert u[a] != 0.0 and u[b] == 0.0                         # the tie at the cut goes to the smaller p
    # ARS with all returns equal: s == 0, every weight is zero
    u, _ = weights_on_device(sim, L.FS_ES_MODE_ARS, np.full(2 * N + E, 3.25), N, E, top=5)
    np.testing.assert_array_equal(u, np.zeros(N, np.float32))
    # the largest shape: 2048 pairs in the one workgroup's LDS
    big = rng.normal(0.0, 1.0, 2 * 2048 + 1)
    u, st = weights_on_device(sim, L.FS_ES_MODE_ES, big, 2048, 1)
    np.testing.assert_array_equal(u, centered_ranks_ref(big[:4096]))
    np.testing.assert_array_equal(st, stats_ref(big, 2048, 1))


@pytest.mark.parametrize("N", [1, 3, 257])
@pytest.mark.parametrize("mode", ["es", "ars"])
def test_gradient_is_within_the_float32_summation_bound_and_repeats(sim, N, mode):
    import torch
    from flow_amd import _lib as L
    P, gen = 2306, 5
    rng = np.random.default_rng(N)
    u = rng.normal(0.0, 0.3, N).astype(np.float32)
    if N > 3:
        u[::5] = 0.0                                           # (directions ARS dropped: skipped, adding exactly nothing)
    theta = rng.normal(0, 0.5, P).astype(np.float32)
    coef = np.float32(0.005 if mode == "es" else 0.2)
    work = torch.zeros(int(sim.lib.fs_es_workspace(P, N)), device="cuda:0")
    assert work.numel() == ((N + 31) // 32) * P
    ud = dev_tensor(u)
    runs = []
    for _ in range(2):
        th, grad = dev_tensor(theta), torch.zeros(P, device="cuda:0")
        torch.cuda.synchronize()
        check(sim, sim.lib.fs_es_grad_dev(sim._h, L.FS_ES_MODE_ES if mode == "es" else L.FS_ES_MODE_ARS, P, N, ud.data_ptr(), SEED,
                                          gen, float(coef), th.data_ptr(), grad.data_ptr(), work.data_ptr(), work.numel()))
        sim.sync()
        assert sim.last_kernel == "k_es_grad"
        runs.append((th.cpu().numpy(), grad.cpu().numpy()))
    np.testing.assert_array_equal(runs[0][0], runs[1][0])      # bit-identical across launches
    np.testing.assert_array_equal(runs[0][1], runs[1][1])
    terms = u.astype(np.float64)[:, None] * eps_ref(N, P, gen).astype(np.float64)
    g64, bound = terms.sum(axis=0), (N + 2) * 2.0 ** -24 * np.abs(terms).sum(axis=0)
    if mode == "es":
        # grad = -g + l2 * theta: recover g through the exact float32 restatement of the two other operations
        np.testing.assert_array_equal(runs[0][0], theta)       # theta is not written
        g = gradient_ref(u, eps_ref(N, P, gen))
        np.testing.assert_array_equal(runs[0][1], -g + coef * theta)
    else:
        g = gradient_ref(u, eps_ref(N, P, gen))
        np.testing.assert_array_equal(runs[0][0], theta + coef * g)
    err = np.abs(g.astype(np.float64) - g64)
    print("N = %d: max error / bound = %.3g" % (N, float((err / np.maximum(bound, 1e-300)).max())))
    assert (err <= bound).all()


def gradient_ref(u, eps):
    """k_es_grad's order in numpy float32: chunks of 32 directions added in ascending p from +0 (a zero weight is
    skipped), then the chunks' partials in ascending order from +0."""
    N, P = eps.shape
    g = np.zeros(P, np.float32)
    for y in range((N + 31) // 32):
        acc = np.zeros(P, np.float32)
        for p in range(32 * y, min(32 * y + 32, N)):
            if u[p] != 0:
                acc = acc + u[p] * eps[p]
        g = g + acc
    return g


def es_env(R=128, horizon=20):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import flow_amd
    from flow_amd.envs import VecFlowEnv
    from flow_amd.utils.device_policy import DevicePolicy
    from train_vec import GaussianPolicy, ring_flow_params
    flow_amd.install_as_flow()
    vec = VecFlowEnv(ring_flow_params(horizon), num_replicas=R, device=0)
    torch.manual_seed(0)
    pi = GaussianPolicy(vec.obs_dim, vec.act_dim).to(vec.device)
    pol = DevicePolicy([pi.mu[0], pi.mu[2]], pi.mu[4], log_std=pi.log_std, seed=0)
    return vec, pol


@pytest.mark.parametrize("mode", ["es", "ars"])
def test_device_es_two_generations_equal_the_numpy_restatement(mode):
    import torch
    from flow_amd.utils.device_es import DeviceES, ars_weights_ref, centered_ranks_ref
    N, E, H = 3, 2, 20
    vec, pol = es_env(128, H)
    kw = dict(pairs=N, eval_members=E, noise_seed=SEED, mode=mode)
    kw.update(dict(sigma=0.02, lr=0.02, l2=0.005) if mode == "es" else dict(sigma=0.2, stepsize=0.2, top=2))
    es = DeviceES(vec, pol, **kw)
    assert (es.M, es.group, es.P) == (8, 16, pol.buf.numel())
    theta = es.theta.cpu().numpy().copy()
    m, v, state = np.zeros(es.P, np.float32), np.zeros(es.P, np.float32), np.array([0.0, 1.0, 1.0])
    mid = snap = None
    for gen in range(2):
        if gen == 1:                                           # the learner's state and the environments', in the middle
            mid, snap = es.state_dict(), vec.snapshot().state_dict()
        stats = es.generation(H, fragment=8)                   # 8 + 8 + 4 steps: three fragments, accumulated
        torch.cuda.synchronize()
        assert vec.sim.last_kernel == ("k_adam" if mode == "es" else "k_es_grad")
        w = es.weights.cpu().numpy()
        t = (np.float32(es.sigma) * eps_ref(N, es.P, gen)).astype(np.float32)
        np.testing.assert_array_equal(w[0:2 * N:2, :es.P], theta[None, :] + t)     # perturbed from the theta of this generation
        fit = es.fit.cpu().numpy()
        assert np.isfinite(fit).all() and len(set(fit[:2 * N].tolist())) > 1
        assert int(es.alive.sum()) == 0                        # every replica's episode ended at the horizon
        u = centered_ranks_ref(fit[:2 * N]) if mode == "es" else ars_weights_ref(fit[:2 * N], 2)
        np.testing.assert_array_equal(es.u.cpu().numpy(), u)
        np.testing.assert_array_equal(stats.cpu().numpy(), stats_ref(fit, N, E))
        g = gradient_ref(u, eps_ref(N, es.P, gen))
        if mode == "es":
            grad = -g + np.float32(es.l2) * theta
            np.testing.assert_array_equal(es.grad.cpu().numpy(), grad)
            theta, m, v, state = adam_ref(theta, grad, m, v, state, lr=es.lr, betas=es.betas, eps=es.eps)
            np.testing.assert_array_equal(es.m.cpu().numpy(), m)
            np.testing.assert_array_equal(es.v.cpu().numpy(), v)
            np.testing.assert_array_equal(es.state.cpu().numpy(), state)
        else:
            theta = theta + np.float32(es.stepsize) * g
        np.testing.assert_array_equal(es.theta.cpu().numpy(), theta)
        assert np.array_equal(pol.buf.cpu().numpy(), theta)    # theta IS the policy's buffer
    after = es.state_dict()
    # a state_dict round trip taken in the middle reproduces the second generation bit for bit: on another handle, with the
    # environments' snapshot next to it (their noise streams and the ring-length generator run on across the resets)
    vec2, pol2 = es_env(128, H)
    es2 = DeviceES(vec2, pol2, **kw)
    vec2.load_snapshot(snap)
    es2.load_state_dict(mid)
    assert es2.gen == 1
    es2.generation(H, fragment=8)
    torch.cuda.synchronize()
    again = es2.state_dict()
    for key in ("theta", "m", "v", "state"):
        np.testing.assert_array_equal(again[key].numpy(), after[key].numpy(), err_msg=key)
    assert again["generation"] == after["generation"] == 2
    np.testing.assert_array_equal(es2.fit.cpu().numpy(), es.fit.cpu().numpy())
    vec.close(), vec2.close()


@pytest.mark.parametrize("mode", ["es", "ars"])
def test_train_py_restores_to_the_uninterrupted_run_and_evaluate_reads_the_checkpoint(mode, tmp_path, monkeypatch, capsys):
    """`train.py singleagent_ring --rl_trainer es|ars` (horizon 20, 128 replicas: 3 pairs + 2 evaluation members): three
    generations; restored from the first generation's checkpoint, the run prints the reward part of the lines the
    uninterrupted run prints; examples/evaluate.py rolls the last checkpoint out (the fused single-policy kernel)."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train
    from evaluate import evaluate_checkpoint
    mod, _ = train.load_experiment("singleagent_ring")
    monkeypatch.setattr(mod.flow_params["env"], "horizon", 20)
    monkeypatch.setattr(mod.flow_params["env"], "warmup_steps", 5)
    capsys.readouterr()
    common = ["singleagent_ring", "--rl_trainer", mode, "--replicas", "128", "--rollout_size", "8", "--es_eval_members", "2",
              "--checkpoint_freq", "1"]
    full = train.main(common + ["--num_steps", "3", "--checkpoint_dir", str(tmp_path / "a")])
    first = capsys.readouterr().out.splitlines()
    rest = train.main(common + ["--num_steps", "2", "--checkpoint_dir", str(tmp_path / "b"),
                                "--restore", str(tmp_path / "a" / "checkpoint_0")])
    second = capsys.readouterr().out.splitlines()
    assert len(full) == 3 and rest == full[1:] and len(set(full)) == 3

    def rewards(ls):
        return [l.split("  generation ")[0] for l in ls if l.startswith("iteration")]
    assert len(rewards(first)) == 3 and rewards(second) == rewards(first)[1:]
    assert all("evaluation/episode_reward_mean" in l and "k_ring_policy<Population>" in l for l in first if l.startswith("iteration"))
    assert any(l.startswith("restore: the environments continue") for l in second)
    res = evaluate_checkpoint(str(tmp_path / "a" / "checkpoint_2"), num_rollouts=64, fragment=10, log=lambda *a: None)
    assert res["kernel"] == "k_ring_policy" and res["path"] == "fused" and res["episodes"] >= 64 and res["iteration"] == 2
    assert np.isfinite(res["episode_reward_mean"])
