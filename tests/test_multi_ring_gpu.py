"""MultiWaveAttenuationPOEnv on MultiRingNetwork (head FS_ENV_MULTI_WAVE_ATTENUATION_PO; lord_of_the_rings.py): a replica
row is one ring with one agent, rewarded over the vehicles of its ring whose front is outside the junctions.

* the generic kernel k_steps against tests/multi_ring_ref.MultiRingOracle: float32 bit for bit (noise 0.2 through the exact
  Box-Muller sequence), float64 at 1e-9; rows are placed so that one and two fronts stand inside junctions (slot A, slot B
  of a lane, the row's last lane) and, with two vehicles, both: the reward 0 / 0 = NaN on both sides.  The oracle run
  itself must have seen n = N, N - 1, N - 2 and 0 vehicles on the edges, so a kernel that ignores the mask cannot pass;
* k_ring_pair<MultiRing> (HEAD 4): action-tape rollouts equal step-by-step generic stepping bit for bit, masked, zero-step
  and last-step-observation launches included, with and without noise, with and without the reciprocal divisions;
* k_ring_policy<MultiRing> (HEAD 4): the fused fragment equals eager fs_policy_act_dev + fs_step_dev + masked fs_reset_dev;
* snapshot / restore repeats the future; the scalar environment, VecFlowEnv's row order and train.py lord_of_the_rings."""
import math
import os
import sys
import types

import numpy as np
import pytest

from multi_ring_ref import MultiRingOracle, multi_ring_spec
from test_policy_gpu import buffers, eager_obs0, make_policy
from test_ringrl_gpu import make, rollout, tape

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JUNCTION_CENTRES = (57.55, 115.15, 172.75, 230.35)        # ring length 230, junctions of 0.1 m after every quarter


def in_junction(x, length=230.0, jl=0.1):
    q = length / 4 + jl
    return (x - np.floor(x / q) * q) >= length / 4


def place(N, slots, length=230.0, jl=0.1):
    """[N] positions, evenly spaced in (cyclic) ring order, with exactly the fronts of ``slots`` inside junctions and at
    least 0.5 m between any two vehicles: the rotation of the row is searched, the chosen slots are moved onto the nearest
    junction's centre."""
    loop = length + 4 * jl
    step = loop / N
    for c in np.arange(0.0, loop, 0.05):
        x = (c + step * np.arange(N)) % loop
        ok = True
        for s in slots:
            t = min(JUNCTION_CENTRES, key=lambda t: abs(t - x[s]))
            ok = ok and abs(t - x[s]) <= step - 5.5
            x[s] = t
        if ok and set(np.flatnonzero(in_junction(x, length, jl))) == set(slots):
            return x
    raise AssertionError("no placement of %d vehicles with fronts %r in junctions" % (N, slots))


def junction_rows(N, R):
    """{row: slots inside junctions}: one in slot A of a lane, one in slot B, one in either slot of the row's last lane, two
    (half a ring apart: both can stand on a centre) with one of them in the last lane.  Row 0 keeps its placement."""
    raw = [(2,), (5,), (N - 1,), (N - 2,), (N // 2 - 1, N - 1), (4, 4 + N // 2)]
    cases = [c for c in raw if all(0 <= s < N for s in c) and len(set(c)) == len(c)]
    if N == 2:
        cases = [(0, 1), (1,)]
    return {r + 1: c for r, c in enumerate(cases) if r + 1 < R}


def place_rows(spec, sims, oracles=()):
    """Write junction_rows' placements (speeds zero) into the handles and the oracles."""
    from flow_amd import _lib as L
    R, N = spec["num_replicas"], spec["num_vehicles"]
    X = np.array(sims[0].pos, dtype=np.float64)
    for r, slots in junction_rows(N, R).items():
        X[r] = place(N, slots)
    for sim in sims:
        sim.set_state(L.FS_FIELD_POS, X)
        sim.set_state(L.FS_FIELD_VEL, np.zeros((R, N)))
    for ora in oracles:
        ora.x[:] = X.astype(ora.dt_)
        ora.v[:] = 0
    return X


def expected_counts(N, R):
    return {N} | {N - len(s) for s in junction_rows(N, R).values()}


# ------------------------------------------------------------------------------------------- the generic kernel
@pytest.mark.parametrize("N,R", [(22, 9), (4, 5), (32, 9), (2, 5)])
def test_generic_kernel_f32_is_the_oracle_bit_for_bit(N, R):
    K = 40
    spec = multi_ring_spec(R=R, N=N, noise=0.2, seed=N, noise_math="exact")
    acts = tape(K, R, 1, seed=N + 3)
    sim, ora = make(spec, "f32", FLOWSIM_FORCE_GENERIC=1), MultiRingOracle(spec, np.float32)
    assert (sim.obs_dim, sim.act_dim) == (3, 1)
    np.testing.assert_array_equal(sim.reset(), ora.reset().astype(np.float32))
    place_rows(spec, [sim], [ora])
    nan_steps = 0
    for k in range(K):
        o_gpu, r_gpu, d_gpu = sim.step(acts[k])
        o_ref, r_ref, d_ref = ora.step(acts[k])
        np.testing.assert_array_equal(o_gpu, o_ref.astype(np.float32), err_msg="obs, step %d" % k)
        np.testing.assert_array_equal(r_gpu, r_ref.astype(np.float32), err_msg="reward, step %d" % k)
        np.testing.assert_array_equal(d_gpu, d_ref)
        np.testing.assert_array_equal(sim.pos, ora.x)
        np.testing.assert_array_equal(sim.vel, ora.v)
        nan_steps += int(np.isnan(r_ref).sum())
    assert sim.last_kernel.startswith("k_steps"), sim.last_kernel
    assert expected_counts(N, R) <= ora.seen_n, (sorted(ora.seen_n), sorted(expected_counts(N, R)))
    if N == 2:                                                     # both fronts in junctions: 0 / 0 on both sides
        assert 0 in ora.seen_n and nan_steps > 0 and np.isnan(r_ref).sum() == np.isnan(r_gpu).sum()
    else:
        assert nan_steps == 0 and np.abs(r_ref).max() > 0
    sim.close()


@pytest.mark.parametrize("N,R", [(22, 9), (2, 5)])
def test_generic_kernel_f64_holds_the_reference_arithmetic(N, R):
    """FS_F64 as tests/test_parity_gpu.py holds it on the other ring heads: 1e-9 on state, observation and reward."""
    K = 40
    spec = multi_ring_spec(R=R, N=N, noise=0.2, seed=N + 1)
    acts = tape(K, R, 1, seed=N + 5)
    sim, ora = make(spec, "f64"), MultiRingOracle(spec, np.float64)
    np.testing.assert_allclose(sim.reset(), ora.reset().astype(np.float32), rtol=0, atol=1e-9)
    place_rows(spec, [sim], [ora])
    for k in range(K):
        o_gpu, r_gpu, d_gpu = sim.step(acts[k])
        o_ref, r_ref, d_ref = ora.step(acts[k])
        np.testing.assert_allclose(sim.pos, ora.x, rtol=0, atol=1e-9)
        np.testing.assert_allclose(sim.vel, ora.v, rtol=0, atol=1e-9)
        np.testing.assert_allclose(o_gpu, o_ref.astype(np.float32), rtol=0, atol=1e-9)
        np.testing.assert_allclose(r_gpu, r_ref.astype(np.float32), rtol=0, atol=1e-9)       # (NaN equals NaN)
        np.testing.assert_array_equal(d_gpu, d_ref)
    assert sim.last_kernel.startswith("k_steps"), sim.last_kernel
    assert expected_counts(N, R) <= ora.seen_n
    sim.close()


def test_max_cost_table_through_the_reward_of_standing_vehicles():
    """Every vehicle at rest: cost = ||[target] * n|| = max_cost[n] up to the rounding of the summation order, so the
    reward is within a few ulps of 0; a table entry off by a factor would show as a reward of order one.  And the
    precondition of the bit-for-bit tests: the library's table (a running float64 sum of target^2, then sqrt) equals
    numpy's norm for the targets used, 4 and 4.3, n = 0 .. 32."""
    for target in (4.0, 4.3):
        ss, lib = 0.0, []
        for n in range(33):
            lib.append(math.sqrt(ss))
            ss += target * target
        want = [float(np.linalg.norm(np.array([target] * n, dtype=np.float64))) for n in range(33)]
        assert np.array_equal(np.float32(lib), np.float32(want)), target
    spec = multi_ring_spec(R=9, N=22, noise=0.0, seed=2, target=4.3)
    sim, ora = make(spec, "f32", FLOWSIM_FORCE_GENERIC=1), MultiRingOracle(spec, np.float32)
    sim.reset(), ora.reset()
    place_rows(spec, [sim], [ora])
    a = np.zeros((9, 1), np.float32)
    o_gpu, r_gpu, _ = sim.step(a)
    o_ref, r_ref, _ = ora.step(a)
    np.testing.assert_array_equal(r_gpu, r_ref.astype(np.float32))
    assert {22, 21, 20} <= ora.seen_n and np.all(np.abs(r_gpu) < 0.05)       # (one step from rest: speeds below 0.1 m/s)
    sim.close()


# ------------------------------------------------------------------------------------------- k_ring_pair HEAD 4
def step_rows(sim, acts):
    out = [sim.step(a) for a in acts]
    return (np.stack([o for o, _, _ in out]), np.stack([r for _, r, _ in out]), np.stack([d for _, _, d in out]))


@pytest.mark.parametrize("N,R,noise,env", [(22, 5, 0.2, {}), (22, 9, 0.0, {}), (32, 9, 0.2, {}), (4, 9, 0.2, {}),
                                           (2, 5, 0.0, {}), (22, 9, 0.2, {"FLOWSIM_NO_FASTDIV": 1})])
def test_ring_pair_rollouts_equal_generic_stepping(N, R, noise, env):
    spec = multi_ring_spec(R=R, N=N, noise=noise, warmup=3, horizon=30, seed=N + R)
    fast, slow = make(spec, "f32", **env), make(spec, "f32", FLOWSIM_NO_RING_RL=1)
    np.testing.assert_array_equal(fast.reset(), slow.reset())                      # (warm-up steps: no actions, reward 0)
    assert fast.last_kernel == "k_ring_pair<MultiRing>" and slow.last_kernel.startswith("k_steps")
    place_rows(spec, [fast, slow])
    np.testing.assert_array_equal(eager_obs0(fast), eager_obs0(slow))              # a zero-step launch
    acts = tape(1 + 16 + 37 + 5, R, 1, seed=N)
    k0 = 0
    saw_nan = False
    for K in (1, 16, 37):
        o, r, d = rollout(fast, K, acts[k0:k0 + K])
        assert fast.last_kernel == "k_ring_pair<MultiRing>"
        so, sr, sd = step_rows(slow, acts[k0:k0 + K])
        np.testing.assert_array_equal(o, so, err_msg="obs, K = %d" % K)
        np.testing.assert_array_equal(r, sr, err_msg="reward, K = %d" % K)
        np.testing.assert_array_equal(d != 0, sd)
        np.testing.assert_array_equal(fast.pos, slow.pos)
        np.testing.assert_array_equal(fast.vel, slow.vel)
        saw_nan = saw_nan or bool(np.isnan(sr).any())
        k0 += K
    assert saw_nan == (N == 2)
    assert (d != 0).any()                                                          # the horizon fell inside the rollouts
    # a masked reset (placement, three warm-up steps of the masked rows only), then the observation of the last step only
    mask = np.zeros(R, np.uint8)
    mask[[0, R - 1]] = 1
    np.testing.assert_array_equal(fast.reset(mask), slow.reset(mask))
    assert fast.last_kernel == "k_ring_pair<MultiRing>"
    np.testing.assert_array_equal(fast.pos, slow.pos)
    np.testing.assert_array_equal(fast.time_counter, slow.time_counter)
    o, r, d = rollout(fast, 5, acts[k0:k0 + 5], obs_every_step=False)
    so, sr, sd = step_rows(slow, acts[k0:k0 + 5])
    np.testing.assert_array_equal(o[0], so[-1])
    np.testing.assert_array_equal(r[0], sr[-1])
    np.testing.assert_array_equal(fast.pos, slow.pos)
    fast.close(), slow.close()


def test_mixed_handles_of_this_head_are_refused_by_name():
    with pytest.raises(NotImplementedError, match="FS_ENV_MULTI_WAVE_ATTENUATION_PO"):
        make(multi_ring_spec(R=4, N=22, noise=0.0), "mixed")


# ------------------------------------------------------------------------------------------- k_ring_policy HEAD 4
def eager_fragment(sim, pol, K):
    import torch
    dev, R = torch.device("cuda", 0), sim.R
    eo, ea, elp, er, ed = buffers(K, R, dev)
    eo[0].copy_(torch.as_tensor(eager_obs0(sim), device=dev))
    torch.cuda.synchronize()
    for k in range(K):
        sim.policy_act_dev(pol.struct, eo[k], ea[k], elp[k])
        assert sim.last_kernel == "k_policy_act"
        sim.step_dev(eo[k + 1], er[k], ed[k], ea[k].reshape(R, 1))
        sim.reset_dev(eo[k + 1], ed[k])
    sim.sync()
    return eo, ea, elp, er, ed


@pytest.mark.parametrize("R", [5, 9])
@pytest.mark.parametrize("N,noise,free,greedy", [(22, 0.2, True, False), (22, 0.2, False, False), (22, 0.0, False, True),
                                                 (32, 0.2, True, True)])
def test_fused_fragment_equals_eager_stepping(R, N, noise, free, greedy):
    import torch
    K = 20
    dev = torch.device("cuda", 0)
    spec = multi_ring_spec(R=R, N=N, noise=noise, warmup=3, horizon=7, seed=R + N)       # resets fall inside the fragment
    pol_a, pol_b = make_policy(2, free, seed=5), make_policy(2, free, seed=5)
    pol_a.greedy = pol_b.greedy = greedy
    fused, eager = make(spec, "f32"), make(spec, "f32")
    fused.reset(), eager.reset()
    place_rows(spec, [fused, eager])
    out = buffers(K, R, dev)
    fused.policy_rollout_dev(pol_a.struct, K, *out, reset_done=True)
    fused.sync()
    assert fused.last_kernel == "k_ring_policy<MultiRing>"
    want = eager_fragment(eager, pol_b, K)
    for name, x, y in zip(("obs", "act", "logp", "rew", "done"), out, want):
        np.testing.assert_array_equal(x.cpu().numpy(), y.cpu().numpy(), err_msg=name)
    np.testing.assert_array_equal(fused.pos, eager.pos)
    np.testing.assert_array_equal(fused.vel, eager.vel)
    np.testing.assert_array_equal(fused.time_counter, eager.time_counter)
    assert (out[4].cpu().numpy() != 0).sum() >= 2 * R and np.abs(out[3].cpu().numpy()).max() > 0
    # the draw counters: the next sampled action of both handles for one observation is the same draw
    pol_a.greedy = pol_b.greedy = False
    obs = out[0][K].clone()
    a1, l1, a2, l2 = (torch.zeros(R, device=dev) for _ in range(4))
    torch.cuda.synchronize()
    fused.policy_act_dev(pol_a.struct, obs, a1, l1)
    eager.policy_act_dev(pol_b.struct, obs, a2, l2)
    fused.sync(), eager.sync()
    np.testing.assert_array_equal(a1.cpu().numpy(), a2.cpu().numpy())
    fused.close(), eager.close()


def test_snapshot_and_restore_repeat_the_future():
    import torch
    R, K = 5, 10
    dev = torch.device("cuda", 0)
    spec = multi_ring_spec(R=R, N=22, noise=0.2, warmup=3, horizon=7, seed=8)
    pol = make_policy(2, False, seed=6)
    sim = make(spec, "f32")
    sim.reset()
    place_rows(spec, [sim])
    warm = buffers(3, R, dev)
    sim.policy_rollout_dev(pol.struct, 3, *warm, reset_done=True)          # (draw counters off zero, mid Philox block)
    blob = torch.zeros(int(sim.snapshot_info().bytes), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    sim.snapshot_dev(blob)
    first = buffers(K, R, dev)
    sim.policy_rollout_dev(pol.struct, K, *first, reset_done=True)
    sim.sync()
    state = (sim.pos, sim.vel, sim.time_counter)
    sim.restore_dev(blob)
    again = buffers(K, R, dev)
    sim.policy_rollout_dev(pol.struct, K, *again, reset_done=True)
    sim.sync()
    assert sim.last_kernel == "k_ring_policy<MultiRing>"
    for x, y in zip(first, again):
        np.testing.assert_array_equal(x.cpu().numpy(), y.cpu().numpy())
    for x, y in zip(state, (sim.pos, sim.vel, sim.time_counter)):
        np.testing.assert_array_equal(x, y)
    sim.close()


# ------------------------------------------------------------------------------------------- the env layer
def lord_params(num_rings, horizon=50, warmup=4):
    """flow_params of lord_of_the_rings.py with NUM_RINGS = num_rings, a short horizon and the exact noise sequence."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    __import__("train")                                        # (installs flow_amd as `flow`)
    path = os.path.join(ROOT, "examples", "exp_configs", "rl", "multiagent", "lord_of_the_rings.py")
    with open(path) as f:
        text = f.read()
    assert text.count("NUM_RINGS = 1\n") == 1
    scope = {"__name__": "lord_of_the_rings_%d" % num_rings}
    exec(compile(text.replace("NUM_RINGS = 1\n", "NUM_RINGS = %d\n" % num_rings), path, "exec"), scope)
    fp = scope["flow_params"]
    fp["env"].horizon, fp["env"].warmup_steps = horizon, warmup
    fp["sim"].noise_math, fp["sim"].seed = "exact", 31
    return fp


def test_scalar_env_with_two_rings_is_the_oracle():
    fp = lord_params(2)
    network = fp["network"](name=fp["exp_tag"], vehicles=fp["veh"], net_params=fp["net"], initial_config=fp["initial"])
    env = fp["env_name"](fp["env"], fp["sim"], network)
    ora = MultiRingOracle(env._spec, np.float32)
    assert env.k.vehicle.get_rl_ids() == ["rl_0_0", "rl_1_0"] and env.sim.R == 2
    obs, o_ref = env.reset(), ora.reset()
    assert sorted(obs) == ["rl_0_0", "rl_1_0"]
    rng = np.random.default_rng(3)
    for k in range(20):
        a = rng.uniform(-1.2, 1.2, 2)
        obs, rew, done, _ = env.step({"rl_0_0": np.array([a[0]]), "rl_1_0": np.array([a[1]])})
        o_ref, r_ref, d_ref = ora.step(a.astype(np.float32).reshape(2, 1))
        np.testing.assert_array_equal(env.sim.pos, ora.x)
        np.testing.assert_array_equal(env.sim.vel, ora.v)
        for g, rl_id in enumerate(("rl_0_0", "rl_1_0")):
            np.testing.assert_allclose(obs[rl_id], o_ref[g].astype(np.float64), rtol=0, atol=1e-12)
            assert abs(rew[rl_id] - float(r_ref[g])) <= 1e-12
        assert done["__all__"] == bool(d_ref[0])
    assert env.k.vehicle.get_leader("rl_1_0") == "human_1_0" and env.k.vehicle.get_edge("human_1_0").endswith("_1")
    assert env.step(None)[1] == {}                                   # rl_actions None: no rewards (:103-105)
    env.terminate()


def test_vec_env_rows_are_env_major():
    import torch
    from flow_amd.envs import VecFlowEnv
    vec = VecFlowEnv(lord_params(2), num_replicas=3)
    assert (vec.num_envs, vec.num_rings, vec.num_rows, vec.obs_dim, vec.act_dim) == (3, 2, 6, 3, 1)
    spec = vec.env._spec
    X = np.asarray(spec["init_pos"])
    assert X.shape == (6, 22) and np.array_equal(X[0::2], np.tile(X[0], (3, 1))) and np.array_equal(X[1::2], np.tile(X[1], (3, 1)))
    assert abs((X[1] - X[0])[0] - 1e-13) < 1e-12 and not np.array_equal(X[0], X[1])
    ora = MultiRingOracle(spec, np.float32)
    np.testing.assert_array_equal(vec.reset().cpu().numpy(), ora.reset().astype(np.float32))
    a = torch.linspace(-1, 1, 6, device=vec.device).reshape(6, 1).contiguous()
    for _ in range(5):
        o, r, d = vec.step(a)
        o_ref, r_ref, d_ref = ora.step(a.cpu().numpy())
    np.testing.assert_array_equal(o.cpu().numpy(), o_ref.astype(np.float32))
    np.testing.assert_array_equal(r.cpu().numpy(), r_ref.astype(np.float32))
    assert tuple(r.shape) == (6,) and len(set(r.cpu().numpy().tolist())) == 6          # every row its own stream
    vec.close()


@pytest.mark.parametrize("extra", [[], ["--device_adam"]])
def test_train_lord_of_the_rings_fused_equals_the_captured_graph(extra, monkeypatch, capsys):
    """`train.py lord_of_the_rings --fuse_policy [--device_adam]` with two rings: two iterations; the fused kernel's
    iterations are those of the captured graph around k_policy_act + step + reset launches (the library draws both).
    choose_rollout's probes and the graph's eager warm-up steps move the draw counters and the noise stream by different
    amounts on the two routes, so the comparison puts the handle back to its state before them (snapshot / restore) and
    resets: both routes then start from the same streams."""
    fp = lord_params(2, horizon=9, warmup=3)
    train = __import__("train")
    train_vec = __import__("train_vec")
    from flow_amd.envs import VecFlowEnv
    args = ["lord_of_the_rings", "--fuse_policy", "--num_steps", "2", "--rollout_size", "12", "--replicas", "6"] + extra
    module = types.SimpleNamespace(flow_params=fp)
    choose = train_vec.choose_rollout

    def aligned(vec, *a, **kw):
        snap = vec.snapshot()
        fused, graph, graph_policy = choose(vec, *a, **kw)
        vec.restore(snap)
        obs = vec.reset()
        if graph is not None:
            graph.begin(obs)
        return fused, graph, graph_policy
    monkeypatch.setattr(train_vec, "choose_rollout", aligned)

    def run():
        history = train.train_device(module, train.parse_args(args), multiagent=True)
        lines = capsys.readouterr().out.splitlines()
        return ([ln for ln in lines if ln.startswith("rollout:")][0], [ln for ln in lines if ln.startswith("iteration")],
                history)

    how, fused, h_fused = run()
    assert "fused policy + step kernel (k_ring_policy<MultiRing>)" in how, how

    def refuse(self, *a, **kw):
        raise NotImplementedError("the fused form is switched off for this comparison")
    monkeypatch.setattr(VecFlowEnv, "policy_rollout", refuse)
    how, graph, h_graph = run()
    assert "around the policy kernel (k_policy_act)" in how, how
    assert len(fused) == 2 and len(graph) == 2 and len(h_fused) == 2

    def numbers(ln):                                            # the iteration line without its timings
        return ln.split("  rollout ")[0], ln.split("episodes ended ")[1]
    for a, b in zip(fused, graph):
        assert numbers(a) == numbers(b), (a, b)
    assert h_fused == h_graph and all(math.isfinite(h) for h in h_fused), (h_fused, h_graph)


def test_evaluate_replays_a_lord_of_the_rings_checkpoint(tmp_path, capsys):
    """A checkpoint of `train.py lord_of_the_rings --checkpoint_dir D --checkpoint_env_state --evaluation_interval 1` is
    replayed by examples/evaluate.py on the fused kernel: one episode per ROW (RLlib's per-policy statistics)."""
    fp = lord_params(2, horizon=9, warmup=3)
    train = __import__("train")
    evaluate = __import__("evaluate")
    args = ["lord_of_the_rings", "--fuse_policy", "--device_adam", "--num_steps", "1", "--rollout_size", "9", "--replicas", "4",
            "--checkpoint_dir", str(tmp_path), "--checkpoint_env_state", "--evaluation_interval", "1", "--episode_stats"]
    history = train.train_device(types.SimpleNamespace(flow_params=fp), train.parse_args(args), multiagent=True)
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("iteration")][0]
    assert len(history) == 1 and math.isfinite(history[0]) and "evaluation/episode_reward_mean" in line, line
    res = evaluate.evaluate_checkpoint(os.path.join(str(tmp_path), "checkpoint_0"), num_rollouts=4, fragment=100,
                                       log=lambda *a: None)
    assert (res["path"], res["kernel"], res["steps"]) == ("fused", "k_ring_policy<MultiRing>", 9), res
    assert res["episodes"] == 8 and math.isfinite(res["episode_reward_mean"]) and res["episode_len_mean"] == 9
