"""Two policies on one RL vehicle (flow_amd/csrc/flowsim_policy.h k_policy_pair_act, k_loop_policy_pair): the reference's
adversarial_figure_eight -- 'av' and 'adversary' read the same AccelEnv observation, each draws an action, the vehicle
receives av + perturb_weight * adversary.

* the fused fragment equals K x (fs_policy_pair_act_dev, fs_step_dev(cmd), masked fs_reset_dev) bit for bit, and two
  fragments continue each other;
* with weight 0 the av's side IS the existing single-policy kernel (k_loop_policy, k_policy_act), bit for bit;
* the adversary's column: the network is torch's, the command is the one fma, the log-probability is the Gaussian's, and
  its draws are independent of the av's even under equal seeds;
* everything the pair kernels are not built for is refused by name before anything launches."""
import numpy as np
import pytest

from test_policy_gpu import eager_obs0, fig8_rl_spec, make_policy_in
from test_ringrl_gpu import make, rl_ring_spec

pytestmark = pytest.mark.gpu

D = 28                                  # AccelEnv's observation of 14 vehicles


def bufs(K, R, dev):
    import torch
    out = (torch.zeros((K + 1, R, D), device=dev), torch.zeros((2, K, R), device=dev), torch.zeros((2, K, R), device=dev),
           torch.zeros((K, R), device=dev), torch.zeros((K, R), dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()          # (the handles launch on streams of their own)
    return out


def set_log_std(pol, value):
    import torch
    with torch.no_grad():
        pol.log_std_param.fill_(value)
    pol.sync()
    return pol


def pair(config, seed=3):
    """(av, adversary): 'mixed' = av 3 hidden layers with the two-output head, adversary 1 hidden layer with a free log
    std; 'loud' = both with a free log std of +0.5 (std 1.65: the combined command leaves the action box often)."""
    if config == "mixed":
        return make_policy_in(D, 3, False, seed=seed), make_policy_in(D, 1, True, seed=seed + 1)
    return (set_log_std(make_policy_in(D, 2, True, seed=seed), 0.5),
            set_log_std(make_policy_in(D, 2, True, seed=seed + 1), 0.5))


def eager_fragment(sim, av, adv, w, K, reset_done=True):
    """K x (policy_pair_act_dev, step_dev(cmd), reset_dev(done)): obs, act [2, K, R], logp [2, K, R], rew, done, cmd [K, R]."""
    import torch
    dev, R = torch.device("cuda", 0), sim.R
    eo, _, _, er, ed = bufs(K, R, dev)
    ea, elp, cmd = torch.zeros((K, 2, R), device=dev), torch.zeros((K, 2, R), device=dev), torch.zeros((K, R), device=dev)
    eo[0].copy_(torch.as_tensor(eager_obs0(sim), device=dev))
    torch.cuda.synchronize()
    for k in range(K):
        sim.policy_pair_act_dev(av.struct, adv.struct, w, eo[k], ea[k], elp[k], cmd[k])
        assert sim.last_kernel == "k_policy_pair_act"
        sim.step_dev(eo[k + 1], er[k], ed[k], cmd[k].reshape(R, 1))
        if reset_done:
            sim.reset_dev(eo[k + 1], ed[k])
    sim.sync()
    return eo, ea.permute(1, 0, 2).contiguous(), elp.permute(1, 0, 2).contiguous(), er, ed, cmd


def assert_same(got, want, names=("obs", "act", "logp", "rew", "done")):
    for name, x, y in zip(names, got, want):
        np.testing.assert_array_equal(x.cpu().numpy(), y.cpu().numpy(), err_msg=name)


def assert_same_state(a, b):
    np.testing.assert_array_equal(a.pos, b.pos)
    np.testing.assert_array_equal(a.vel, b.vel)
    np.testing.assert_array_equal(a.time_counter, b.time_counter)


@pytest.mark.parametrize("noise", [0.2, 0.0])
@pytest.mark.parametrize("config", ["mixed", "loud"])
def test_fused_pair_fragment_equals_eager_stepping(config, noise):
    import torch
    K, R, w = 90, 7, 0.5                                        # a partial wave; N = 14: two idle lanes per row
    dev = torch.device("cuda", 0)
    spec = fig8_rl_spec(R, "accel", noise, horizon=35, seed=4)  # every replica finishes episodes inside the fragment
    av_a, adv_a = pair(config)
    av_b, adv_b = pair(config)
    fused, eager = make(spec, "f32"), make(spec, "f32")
    fused.reset(), eager.reset()
    out = bufs(K, R, dev)
    fused.policy_pair_rollout_dev(av_a.struct, adv_a.struct, w, K, *out, reset_done=True)
    fused.sync()
    assert fused.last_kernel == "k_loop_policy<Adversarial>"
    want = eager_fragment(eager, av_b, adv_b, w, K)
    assert_same(out, want[:5])
    assert_same_state(fused, eager)
    assert (out[4].cpu().numpy() != 0).sum() >= 2 * R
    if config == "loud":                                        # (a condition on the inputs: the clip of the command is exercised)
        cmd = want[5].cpu().numpy()
        assert (np.abs(cmd) > 3.0).mean() >= 0.01
    fused.close(), eager.close()


def test_pair_fragments_continue():
    """Two fragments of 45 steps are one of 90: the state, both sampling streams (45 is no multiple of 4: the Philox
    blocks restart mid-block) and the noise stream continue."""
    import torch
    R, w = 7, 0.5
    dev = torch.device("cuda", 0)
    spec = fig8_rl_spec(R, "accel", 0.2, horizon=35, seed=4)
    av, adv = pair("mixed")
    one, two = make(spec, "f32"), make(spec, "f32")
    one.reset(), two.reset()
    whole = bufs(90, R, dev)
    one.policy_pair_rollout_dev(av.struct, adv.struct, w, 90, *whole, reset_done=True)
    one.sync()
    first, second = bufs(45, R, dev), bufs(45, R, dev)
    two.policy_pair_rollout_dev(av.struct, adv.struct, w, 45, *first, reset_done=True)
    two.policy_pair_rollout_dev(av.struct, adv.struct, w, 45, *second, reset_done=True)
    two.sync()
    np.testing.assert_array_equal(first[0][45].cpu().numpy(), second[0][0].cpu().numpy())
    joined = (torch.cat([first[0], second[0][1:]]), torch.cat([first[1], second[1]], dim=1),
              torch.cat([first[2], second[2]], dim=1), torch.cat([first[3], second[3]]), torch.cat([first[4], second[4]]))
    assert_same(joined, whole)
    assert_same_state(one, two)
    one.close(), two.close()


def test_weight_zero_is_the_single_policy_kernel():
    """weight 0: cmd = fma(0, a_adv, a_av) = a_av, so the av's side must be k_loop_policy / k_policy_act bit for bit."""
    import torch
    K, R = 90, 7
    dev = torch.device("cuda", 0)
    spec = fig8_rl_spec(R, "accel", 0.2, horizon=35, seed=4)
    av, adv = pair("mixed")
    both, single = make(spec, "f32"), make(spec, "f32")
    both.reset(), single.reset()
    out = bufs(K, R, dev)
    both.policy_pair_rollout_dev(av.struct, adv.struct, 0.0, K, *out, reset_done=True)
    both.sync()
    o, a, lp, r, d = (torch.zeros((K + 1, R, D), device=dev), torch.zeros((K, R), device=dev), torch.zeros((K, R), device=dev),
                      torch.zeros((K, R), device=dev), torch.zeros((K, R), dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()
    single.policy_rollout_dev(av.struct, K, o, a, lp, r, d, reset_done=True)
    single.sync()
    assert single.last_kernel == "k_loop_policy"
    assert_same((out[0], out[1][0], out[2][0], out[3], out[4]), (o, a, lp, r, d))
    assert_same_state(both, single)
    # the eager forms, on the same observations at the same counters (K, then K + 1, on both handles)
    for k in (0, 1):
        obs = out[0][3 + k].clone()
        pa, plp, cmd = torch.zeros((2, R), device=dev), torch.zeros((2, R), device=dev), torch.zeros(R, device=dev)
        sa, slp = torch.zeros(R, device=dev), torch.zeros(R, device=dev)
        torch.cuda.synchronize()
        both.policy_pair_act_dev(av.struct, adv.struct, 0.0, obs, pa, plp, cmd)
        single.policy_act_dev(av.struct, obs, sa, slp)
        both.sync(), single.sync()
        assert_same((pa[0], plp[0], cmd), (sa, slp, sa), names=("act", "logp", "cmd"))
    both.close(), single.close()


def gaussian_logp(a, mu, ls):
    return -0.5 * ((a - mu) / np.exp(ls)) ** 2 - ls - 0.9189385332046727


def test_adversary_column_is_the_network_the_fma_and_the_gaussian():
    import torch
    K, R, w = 12, 64, 0.37
    dev = torch.device("cuda", 0)
    sim = make(fig8_rl_spec(R, "accel", 0.2, horizon=100, seed=2), "f32")
    sim.reset()
    av = make_policy_in(D, 3, False, seed=5)
    quiet = set_log_std(make_policy_in(D, 3, True, seed=6), -20.0)       # std 2e-9: the action is the mean
    out = bufs(K, R, dev)
    sim.policy_pair_rollout_dev(av.struct, quiet.struct, w, K, *out, reset_done=False)
    sim.sync()
    obs = out[0][:K]
    with torch.no_grad():
        mu, _ = quiet.reference(obs)
    np.testing.assert_allclose(out[1][1].cpu().numpy(), mu.cpu().numpy(), atol=1e-5, rtol=0)
    # the command and the log-probability, eager, with an adversary that does move (log std from its network)
    adv = make_policy_in(D, 2, False, seed=7)
    act, logp, cmd = (torch.zeros((K, 2, R), device=dev), torch.zeros((K, 2, R), device=dev), torch.zeros((K, R), device=dev))
    torch.cuda.synchronize()
    for k in range(K):
        sim.policy_pair_act_dev(av.struct, adv.struct, w, obs[k], act[k], logp[k], cmd[k])
    sim.sync()
    a_av, a_adv = act[:, 0].cpu().numpy(), act[:, 1].cpu().numpy()
    # float32(float64 expression): the product is exact in float64, so it is the fma's value rounded twice -- within 1 ulp
    want = (a_av.astype(np.float64) + np.float64(np.float32(w)) * a_adv.astype(np.float64)).astype(np.float32)
    got = cmd.cpu().numpy()
    assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64))
    with torch.no_grad():
        mu, ls = adv.reference(obs)
    ref = gaussian_logp(a_adv.astype(np.float64), mu.cpu().numpy().astype(np.float64), ls.cpu().numpy().astype(np.float64))
    print("logp[1] vs the Gaussian formula: max abs difference %.3g" % np.abs(logp[:, 1].cpu().numpy() - ref).max())
    np.testing.assert_allclose(logp[:, 1].cpu().numpy(), ref, atol=1e-5, rtol=0)
    sim.close()


def test_equal_seeds_still_draw_independently():
    """Both policies keyed by the SAME seed: the adversary's Philox column (0x40000000 + 1) keeps its draws apart from
    the av's (column 0x40000000).  Standardised draws g = (a - mu) / sd of the two agents over n = 64 x 90 samples:
    |correlation| < 5 / sqrt(n) (five standard errors for independent draws), each mean within 5 / sqrt(n) of 0."""
    import torch
    K, R, w = 90, 64, 0.03
    dev = torch.device("cuda", 0)
    sim = make(fig8_rl_spec(R, "accel", 0.2, horizon=35, seed=8), "f32")
    sim.reset()
    av, adv = set_log_std(make_policy_in(D, 2, True, seed=11), 0.0), set_log_std(make_policy_in(D, 2, True, seed=12), 0.0)
    adv.struct.seed = av.struct.seed
    out = bufs(K, R, dev)
    sim.policy_pair_rollout_dev(av.struct, adv.struct, w, K, *out, reset_done=True)
    sim.sync()
    obs = out[0][:K]
    g = []
    for j, pol in enumerate((av, adv)):
        with torch.no_grad():
            mu, ls = pol.reference(obs)
            g.append(((out[1][j] - mu) / ls.exp()).double().cpu().numpy().reshape(-1))
    n = K * R
    bound = 5.0 / np.sqrt(n)
    corr = np.corrcoef(g[0], g[1])[0, 1]
    print("n = %d  corr %.4f  means %.4f %.4f  stds %.4f %.4f  (bound %.4f)" % (n, corr, g[0].mean(), g[1].mean(), g[0].std(),
                                                                              g[1].std(), bound))
    assert abs(corr) < bound
    assert abs(g[0].mean()) < bound and abs(g[1].mean()) < bound
    sim.close()


def refused_handles():
    return [("ring", lambda: make(rl_ring_spec(R=4, N=22, seed=1), "f32"), 3),
            ("po_head", lambda: make(fig8_rl_spec(4, "po", 0.0, horizon=50, seed=1), "f32"), 3),
            ("obs_dim", lambda: make(fig8_rl_spec(4, "accel", 0.0, horizon=50, seed=1), "f32"), 3),
            ("mixed", lambda: make(fig8_rl_spec(4, "accel", 0.0, horizon=50, seed=1), "mixed"), D)]


@pytest.mark.parametrize("case", range(4), ids=[c[0] for c in refused_handles()])
def test_unsupported_handles_are_refused_by_name_before_any_launch(case):
    import torch
    name, build, in_dim = refused_handles()[case]
    dev = torch.device("cuda", 0)
    sim = build()
    R, K = sim.R, 3
    av, adv = make_policy_in(in_dim, 2, False, seed=1), make_policy_in(in_dim, 2, True, seed=2)
    before = sim.last_kernel
    o = torch.full((K + 1, R, sim.obs_dim), 7.0, device=dev)
    a, lp = torch.full((2, K, R), 7.0, device=dev), torch.full((2, K, R), 7.0, device=dev)
    r, d = torch.full((K, R), 7.0, device=dev), torch.full((K, R), 7, dtype=torch.uint8, device=dev)
    cmd = torch.full((R,), 7.0, device=dev)
    torch.cuda.synchronize()
    with pytest.raises(NotImplementedError, match="fs_policy_pair"):
        sim.policy_pair_rollout_dev(av.struct, adv.struct, 0.5, K, o, a, lp, r, d, reset_done=True)
    with pytest.raises(NotImplementedError, match="fs_policy_pair"):
        sim.policy_pair_act_dev(av.struct, adv.struct, 0.5, o[0], a[:, 0], lp[:, 0], cmd)
    sim.sync()
    assert sim.last_kernel == before
    for t in (o, a, lp, r, cmd):
        assert bool((t == 7.0).all())
    assert bool((d == 7).all())
    sim.close()


def test_a_weight_that_is_not_finite_is_invalid():
    import torch
    dev = torch.device("cuda", 0)
    sim = make(fig8_rl_spec(4, "accel", 0.0, horizon=50, seed=1), "f32")
    av, adv = pair("mixed")
    out = bufs(3, 4, dev)
    with pytest.raises(ValueError, match="fs_policy_pair"):
        sim.policy_pair_rollout_dev(av.struct, adv.struct, float("nan"), 3, *out)
    with pytest.raises(ValueError, match="fs_policy_pair"):
        sim.policy_pair_act_dev(av.struct, adv.struct, float("nan"), out[0][0], torch.zeros((2, 4), device=dev),
                                torch.zeros((2, 4), device=dev), torch.zeros(4, device=dev))
    sim.close()
