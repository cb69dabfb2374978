"""The figure-eight step at its edges: `k_rollout_loop` (flow_amd/csrc/flowsim_fig8.h) and its restatement
`loop_policy_body` (flowsim_policy.h: k_loop_policy, k_greedy_loop_policy, k_loop_policy_pair) against the float32 oracle
(oracle/refsim.py RingOracle) bit for bit, and the FS_MIXED instantiation against the float64 oracle.

Organic runs of helpers.figure_eight_spec never pass three segment starts in a step, never wrap and advance in one, never
stand on a boundary of a `>= / <` pair and never reach the time limit off a block of four steps.  The layouts here are
constructed (tests/helpers.py; tests/test_loop_edges_cpu.py proves on the oracle alone that they reach their events) from
vehicles that move EXACTLY in float32 and float64 (RL vehicles without clamps, parked and waiting IDM vehicles), so a
vehicle is ON a boundary, or one ulp off it, at a chosen step.  Every test repeats the oracle-side assertion that the
event it is named for happened: those are conditions on the inputs, not tolerances.

What is compared with what:
  * single steps with the oracle after every step (obs, reward, done, pos, vel; time at the end): the FULL form;
  * the run as ONE launch and cut into odd fragments with the oracle's rows, on all four forms of the step --
    k_rollout_loop<FULL>, the run-time-flag form, the form without the exponent-4 shortcut, the generic k_steps;
  * fused policy fragments with in-place resets: their own actions replayed through the oracle with masked resets;
  * FS_MIXED: positions, speeds and done flags EQUAL the float64 oracle's where every vehicle moves exactly (derived, not
    measured: every operation is exact in both types); the bounds of
    test_figure_eight_mixed_holds_1e_4_against_the_float64_reference_where_float32_does_not elsewhere."""
import os

import numpy as np
import pytest

from helpers import (CURSOR_N, LOOP_FORMS, ODD_CYCLE, POLICY_HORIZON, SHORT_CYCLE, TAIL_FIRST_CRASH, TAIL_K, TIES, LoopLog,
                     assert_cursor_events, assert_policy_cursor_events, assert_tie, cursor_spec, degenerate_spec,
                     degenerate_winners, fragments_of, gap_tie_spec, oracle_rows, policy_cursor_spec, shape_spec,
                     start_phases, tail_spec, tie_inside, tie_spec, with_form, zero_actions)
from oracle import refsim as S

pytestmark = pytest.mark.gpu

GUARD = 64          # elements of untouched memory kept on either side of every output


def make(spec, precision="f32", env=None):
    from flow_amd.sim import FlowSim
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        return FlowSim(spec, precision)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def guarded(shape, fill, dtype):
    """A tensor of `shape` inside a larger allocation filled with `fill` (NaN / 7, as the rollouts of
    tests/test_parity_gpu.py prefill theirs) -> (whole allocation, the view handed to the kernel)."""
    import torch
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=torch.device("cuda", 0))
    return whole, whole[GUARD:GUARD + n].view(*shape)


def launch(sim, K, acts):
    """One launch of K steps into guarded, prefilled outputs -> obs [K, R, D], rew [K, R], done [K, R] (uint8)."""
    import torch
    R = sim.R
    bufs = [guarded((K, R, sim.obs_dim), float("nan"), torch.float32), guarded((K, R), float("nan"), torch.float32),
            guarded((K, R), 7, torch.uint8)]
    a = None if acts is None else torch.as_tensor(np.ascontiguousarray(acts), device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    sim.rollout_dev(K, bufs[0][1], bufs[1][1], bufs[2][1], actions=a)
    sim.sync()
    out = []
    for (whole, view), fill in zip(bufs, (None, None, 7)):
        w = whole.cpu().numpy()
        for g in (w[:GUARD], w[-GUARD:]):
            assert np.isnan(g).all() if fill is None else (g == fill).all(), "a store outside [K, R]"
        out.append(view.cpu().numpy())
    assert not np.isnan(out[0]).any() and not np.isnan(out[1]).any() and (out[2] < 4).all(), "an element of [K, R] not stored"
    return out


def assert_rows(got, want, k0, crash, what):
    """Rows k0 .. of a launch against the oracle's (obs, rew, done, limit) and the collision bit against `crash`."""
    obs, rew, done = got
    O, Rw, D, lim = want
    for j in range(len(obs)):
        msg = "%s, step %d" % (what, k0 + j)
        np.testing.assert_array_equal(obs[j], O[k0 + j].astype(np.float32), err_msg="obs: " + msg)
        np.testing.assert_array_equal(rew[j], Rw[k0 + j].astype(np.float32), err_msg="reward: " + msg)
        np.testing.assert_array_equal(done[j] != 0, D[k0 + j], err_msg="done: " + msg)
        np.testing.assert_array_equal((done[j] & 1) != 0, lim[k0 + j], err_msg="time limit: " + msg)
        if crash is not None:
            np.testing.assert_array_equal((done[j] & 2) != 0, crash[k0 + j], err_msg="collision: " + msg)


def assert_state(sim, ora, log, what):
    np.testing.assert_array_equal(sim.pos, log.x1[-1], err_msg="pos: " + what)
    np.testing.assert_array_equal(sim.vel, log.v1[-1], err_msg="vel: " + what)
    np.testing.assert_array_equal(sim.time_counter, ora.time_counter, err_msg="time: " + what)


def stepped(spec, acts, K, ora, log, want, env, kernel, precision="f32"):
    """Single steps: everything compared with the oracle after every step."""
    sim = make(spec, precision, env)
    sim.reset()
    O, Rw, D, lim = want
    for k in range(K):
        o, r, d = sim.step(acts[k])
        assert sim.last_kernel.startswith(kernel), (k, sim.last_kernel)
        msg = "stepped, step %d" % k
        np.testing.assert_array_equal(o, O[k].astype(np.float32), err_msg="obs: " + msg)
        np.testing.assert_array_equal(r, Rw[k].astype(np.float32), err_msg="reward: " + msg)
        np.testing.assert_array_equal(d, D[k], err_msg="done: " + msg)
        np.testing.assert_array_equal(sim.pos, log.x1[k], err_msg="pos: " + msg)
        np.testing.assert_array_equal(sim.vel, log.v1[k], err_msg="vel: " + msg)
    if K == len(O):
        np.testing.assert_array_equal(sim.time_counter, ora.time_counter)
    sim.close()


def launched(spec, acts, fragments, ora, log, want, env, kernel, crash=True):
    sim = make(spec, "f32", env)
    sim.reset()
    k0 = 0
    for n in fragments:
        got = launch(sim, n, acts[k0:k0 + n])
        assert sim.last_kernel == kernel or (kernel == "k_steps" and sim.last_kernel.startswith(kernel)), sim.last_kernel
        assert_rows(got, want, k0, np.array(log.crash) if crash else None, "%s, launches %r" % (kernel, fragments[:6]))
        k0 += n
    assert k0 == len(want[0])
    assert_state(sim, ora, log, "%s, launches %r" % (kernel, fragments[:6]))
    sim.close()


def all_forms(spec, K, check, cuts=(), forms=LOOP_FORMS):
    """The run on every form of the step: `check(spec, ora, log, done)` asserts the oracle's side; the FULL form steps and
    launches (whole, and each of `cuts`), the others launch whole and in odd fragments."""
    for form in forms:
        s, env, kernel = with_form(spec, form)
        acts = zero_actions(s, K)
        ora, log, O, Rw, D, lim = oracle_rows(s, acts, K)
        check(s, ora, log, D)
        want = (O, Rw, D, lim)
        if form == "full":
            stepped(s, acts, K, ora, log, want, env, kernel)
        for cut in [[K]] + ([fragments_of(K, c) for c in cuts] if form == "full" else [fragments_of(K, ODD_CYCLE)]):
            launched(s, acts, cut, ora, log, want, env, kernel)


# ------------------------------------------------------------------ 1: the segment cursor
@pytest.mark.parametrize("full16", [True, False])
def test_segment_cursor_passes_three_and_four_starts_wraps_and_lands_on_starts(full16):
    """`k = x < c_st ? 0 : k + (x >= c_next) + (x >= c_next2)` and the `while (adv_m)` behind it: steps that pass 3 and 4
    starts, wrap and pass 1 and 2 past 0, pass the last start and wrap, land on a start (x == start is the new segment), in
    tables of 16 rows (tab_start[k + 2] at k = 15 is the second sentinel) and of 10.  Oracle side: helpers.CURSOR_REPLICAS."""
    def check(s, ora, log, done):
        assert_cursor_events(log)
        rl = [i for i in range(CURSOR_N) if i != CURSOR_N - 2]
        assert (ora.v[:, rl] == np.asarray(s["init_vel"])[:, rl]).all()
    all_forms(cursor_spec(full16), 200, check, cuts=(ODD_CYCLE, SHORT_CYCLE))


# ------------------------------------------------------------------ 2: ties at the crossing
@pytest.mark.parametrize("name", sorted(TIES) + ["gap"])
def test_crossing_ties_on_the_boundary_and_one_ulp_either_side(name):
    """sm_in(x, lo, hi) is lo <= x < hi and sm_lt(h, crash_gap) is h < crash_gap, at the first snapshot of a launch (the
    launch start computes jf) and inside one (jf rides in bits 4 and 5 of the collision butterfly): helpers.TIES."""
    K = 8

    def check(s, ora, log, done):
        assert_tie(name, log, done, K)
    all_forms(gap_tie_spec() if name == "gap" else tie_spec(name), K, check, cuts=(SHORT_CYCLE,))


# ------------------------------------------------------------------ 3: both lines within one look-ahead
@pytest.mark.parametrize("a_first", [True, False])
def test_degenerate_table_takes_the_smaller_of_the_two_stop_speeds(a_first):
    """cap2_m != 0: a vehicle on both approaches with both boxes blocked.  The stop speed grows with the gap, so the nearer
    line binds: stream a's in one table, stream b's in the other (the farther line cannot win with one vehicle's
    parameters; asserted as `== 0`)."""
    def check(s, ora, log, done):
        a_wins, b_wins, replicas = degenerate_winners(log)
        assert replicas >= 2 and (a_wins if a_first else b_wins) >= 3 and (b_wins if a_first else a_wins) == 0
    all_forms(degenerate_spec(a_first), 60, check, cuts=(ODD_CYCLE,))


# ------------------------------------------------------------------ 4: the tail of a launch, the time limit
def test_collisions_in_every_slot_of_a_block_and_of_the_tail():
    """Lane j of a block finishes step j one block late: a collision first seen in step 4, 5, 6, 7 (a full block) and 8, 9,
    10 (a tail of three) of an 11-step launch, and in launches of 1, 2 and 3 steps."""
    def check(s, ora, log, done):
        first = tuple(int(np.argmax(done[:, r])) if done[:, r].any() else None for r in range(done.shape[1]))
        assert first == TAIL_FIRST_CRASH
    all_forms(tail_spec(), TAIL_K, check, cuts=(SHORT_CYCLE, (3, 2, 1)))


@pytest.mark.parametrize("form", LOOP_FORMS)
def test_time_limit_in_every_slot_and_in_the_tail(form):
    """done = t_j >= step_limit with t_j = tcount - (nsteps - 1 - j): horizons 1, 2, 3, 5, 6, 7 in a launch of 11 steps,
    and K - 1 for K = 9, 10, 11 (K % 4 = 1, 2, 3) -- the first done step in every slot of a full block and of the tail."""
    for H, K in [(1, 11), (2, 11), (3, 11), (5, 11), (6, 11), (7, 11), (8, 9), (9, 10), (10, 11)]:
        s, env, kernel = with_form(tail_spec(horizon=H), form)
        acts = zero_actions(s, K)
        ora, log, O, Rw, D, lim = oracle_rows(s, acts, K)
        assert int(np.argmax(lim[:, 7])) == H - 1 and lim[H - 1:].all() and not lim[:H - 1].any()
        launched(s, acts, [K], ora, log, (O, Rw, D, lim), env, kernel)
        if form == "full" and K == 11:
            launched(s, acts, fragments_of(K, (3, 2, 1)), ora, log, (O, Rw, D, lim), env, kernel)


def test_odd_fragments_with_noise_equal_one_launch_and_the_oracle():
    """The run cut as 1, 7, 3, 16, 5, ... and as 2, 3, 1, 4, 6, ...: the Philox block of four draws is entered at every
    phase, the noise (exact math) is the oracle's bit for bit."""
    K = 61
    s, env, kernel = with_form(tail_spec(), "full")
    rng = np.random.default_rng(4)
    acts = (rng.integers(-8, 9, (K, s["num_replicas"], 1)) / 8.0).astype(np.float32)        # dyadic, inside [-1, 1]
    ora, log, O, Rw, D, lim = oracle_rows(s, acts, K)
    assert np.abs(np.diff(np.array(log.v1)[:, :, -1], axis=0)).min() > 0          # the noisy follower's speed never rests
    cuts = [fragments_of(K, ODD_CYCLE), fragments_of(K, SHORT_CYCLE)]
    assert start_phases(cuts[0]) | start_phases(cuts[1]) == {0, 1, 2, 3}
    for cut in [[K]] + cuts:
        launched(s, acts, cut, ora, log, (O, Rw, D, lim), env, kernel)
    launched(s, acts, cuts[0], ora, log, (O, Rw, D, lim), {"FLOWSIM_NO_LOOP_KERNEL": "1"}, "k_steps")


# ------------------------------------------------------------------ 5: shapes
@pytest.mark.parametrize("N,R", [(2, 1), (2, 5), (9, 5), (16, 1), (16, 5)])
def test_rows_of_two_nine_and_sixteen_vehicles_one_and_five_replicas(N, R):
    """N = 16: a full row, slot 15's leader comes from row_newbcast; N = 9: the smallest row the host gives k_rollout_loop
    (up to 8 vehicles it lays a replica out in 8 lanes: those handles step on k_steps -- asserted, and held to the same
    oracle); R = 1 and 5: three rows of the last wave are clamped duplicates that store nothing (every output sits between
    guards that must stay as prefilled)."""
    K = 40
    spec = shape_spec(N, R)
    acts = zero_actions(spec, K)
    ora, log, O, Rw, D, lim = oracle_rows(spec, acts, K)
    ev = log.cursor_events()
    assert ev["pass3"].sum() + ev["pass4"].sum() >= 1 and ev["changed"].sum() >= 4 * R and not D.any()
    kernel = "k_rollout_loop<FULL>" if N >= 9 else "k_steps"
    stepped(spec, acts, 12, ora, log, (O, Rw, D, lim), {}, kernel)
    for cut in ([K], fragments_of(K, ODD_CYCLE)):
        launched(spec, acts, cut, ora, log, (O, Rw, D, lim), {}, kernel)


def test_the_policy_kernels_refuse_a_row_of_eight_lanes_by_name():
    """Up to 8 vehicles a replica is laid out in 8 lanes: k_loop_policy (rows of 16) is not built for such a handle."""
    import torch
    dev = torch.device("cuda", 0)
    spec = shape_spec(2, 5, rl_slots=(1,))
    sim = make(spec)
    sim.reset()
    pol = policy_net(4)
    out = (torch.zeros((4, 5, 4), device=dev), torch.zeros((3, 5), device=dev), torch.zeros((3, 5), device=dev),
           torch.zeros((3, 5), device=dev), torch.zeros((3, 5), dtype=torch.uint8, device=dev))
    with pytest.raises(NotImplementedError, match="num_vehicles"):
        sim.policy_rollout_dev(pol.struct, 3, *out, reset_done=True)
    sim.close()


def test_multi_agent_head_with_rl_vehicles_in_the_first_and_last_slot_and_side_by_side():
    """MultiAgentAccelPOEnv (HEAD 2): the follower's lane writes two values of its leader's block -- the wrap lane for the
    RL vehicle in slot 0, an RL lane for the one in slot 6 (slots 5 and 6 are both RL, and so are 11 and 0)."""
    K = 40
    spec = shape_spec(12, 5, env=S.ENV_ACCEL_PO_MA, rl_slots=(0, 5, 6, 11))
    acts = zero_actions(spec, K)
    ora, log, O, Rw, D, lim = oracle_rows(spec, acts, K)
    ev = log.cursor_events()
    assert O.shape[2] == 24 and ev["changed"].sum() >= 6 and ev["last_wrap"].sum() >= 1
    for env, kernel in (({}, "k_rollout_loop<FULL,AccelMA>"), ({"FLOWSIM_NO_LOOP_FULL": "1"}, "k_rollout_loop<AccelMA>"),
                        ({"FLOWSIM_NO_LOOP_KERNEL": "1"}, "k_steps")):
        for cut in ([K], fragments_of(K, ODD_CYCLE)):
            launched(spec, acts, cut, ora, log, (O, Rw, D, lim), env, kernel, crash=False)      # (this head sees no collision)


# ------------------------------------------------------------------ the fused policy kernels
def policy_net(in_dim, seed=3, bias=None):
    """A sampling policy (random weights), or with `bias` the zero-weight net whose mean action is exactly `bias`."""
    import torch
    from test_policy_gpu import make_policy_in
    pol = make_policy_in(in_dim, 2, True, seed=seed)
    if bias is not None:
        with torch.no_grad():
            for l in pol.hidden + [pol.head]:
                l.weight.zero_()
                l.bias.zero_()
            pol.head.bias.fill_(bias)
        pol.sync()
        pol.greedy = True
    return pol


def fragment(spec, pol, K, pair=None, reset_done=True):
    import torch
    dev = torch.device("cuda", 0)
    R, D = spec["num_replicas"], 2 * spec["num_vehicles"]
    sim = make(spec)
    sim.reset()
    shape = (2, K, R) if pair else (K, R)
    out = (torch.zeros((K + 1, R, D), device=dev), torch.zeros(shape, device=dev), torch.zeros(shape, device=dev),
           torch.zeros((K, R), device=dev), torch.zeros((K, R), dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()
    if pair:
        sim.policy_pair_rollout_dev(pol.struct, pair[0].struct, pair[1], K, *out, reset_done=reset_done)
    else:
        sim.policy_rollout_dev(pol.struct, K, *out, reset_done=reset_done)
    sim.sync()
    assert sim.last_kernel == ("k_loop_policy<Adversarial>" if pair else "k_loop_policy"), sim.last_kernel
    res = [t.cpu().numpy() for t in out] + [sim.pos.copy(), sim.vel.copy(), sim.time_counter.copy()]
    sim.close()
    return res


def replayed(spec, res, K, reset_done=True):
    """The fragment's own actions through the float32 oracle with masked resets: obs, reward, done, the final state.
    -> (LoopLog, done [K, R] bool)."""
    on, an, _, rn, dn, pos, vel, time = res
    R = spec["num_replicas"]
    ora = S.RingOracle(spec, np.float32)
    log = LoopLog(ora)
    np.testing.assert_array_equal(on[0], ora.reset().astype(np.float32))
    dones = []
    for k in range(K):
        o, r, d = ora.step(an[k].reshape(R, 1))
        lim = ora.time_counter >= spec["horizon"]
        if reset_done and d.any():
            o = ora.reset(d)
        np.testing.assert_array_equal(on[k + 1], o.astype(np.float32), err_msg="obs, step %d" % k)
        np.testing.assert_array_equal(rn[k], r.astype(np.float32), err_msg="reward, step %d" % k)
        np.testing.assert_array_equal(dn[k] != 0, d, err_msg="done, step %d" % k)
        np.testing.assert_array_equal((dn[k] & 1) != 0, lim, err_msg="time limit, step %d" % k)
        np.testing.assert_array_equal((dn[k] & 2) != 0, log.crash[-1], err_msg="collision, step %d" % k)
        dones.append(d)
    np.testing.assert_array_equal(pos, ora.x)
    np.testing.assert_array_equal(vel, ora.v)
    np.testing.assert_array_equal(time, ora.time_counter)
    return log, np.array(dones)


def test_policy_fragment_on_the_cursor_table_resets_on_cursor_events():
    """k_loop_policy rescans the table when a vehicle leaves its segment and after a reset: episodes of 3 steps that end
    on the step that passes the mid-loop cluster and wraps, and episodes that carry the advanced cursor on."""
    K = 31
    spec = policy_cursor_spec()
    res = fragment(spec, policy_net(2 * spec["num_vehicles"]), K)
    log, dones = replayed(spec, res, K)
    assert_policy_cursor_events(log, dones)
    assert np.abs(res[1]).max() > 0 and dones.sum() == (K // POLICY_HORIZON) * spec["num_replicas"]


@pytest.mark.parametrize("name", [n for n in sorted(TIES) if TIES[n][0] == "approach"])
def test_policy_fragment_with_a_vehicle_on_an_approach_boundary(name):
    """The approach ties under a SAMPLING policy (the RL vehicle is the one at rest inside the box: it creeps, and stays
    inside), episodes of 4 steps: the waiting vehicle is back on its boundary after every reset."""
    K = 10
    spec = tie_spec(name, horizon=4)
    res = fragment(spec, policy_net(2 * spec["num_vehicles"]), K)
    log, dones = replayed(spec, res, K)
    x0, x1, _, held = log.arrays()
    inside = tie_inside(name)
    for k in (0, 4, 8):                                      # the first step of every episode
        np.testing.assert_array_equal(held[k, :, 1], inside)
        assert (x1[k, ~inside, 1] > x0[k, ~inside, 1]).all() and (x1[k, inside, 1] == x0[k, inside, 1]).all()
    assert held[:, inside, 1].all() and np.abs(res[1]).max() > 0 and dones[3].all() and dones[7].all()


def test_policy_fragment_on_the_degenerate_table_and_into_a_collision():
    K = 40
    for a_first in (True, False):
        spec = degenerate_spec(a_first, horizon=25)
        X = np.array(spec["init_pos"])
        X[:, 0] = 46.0                                       # (the creeping RL vehicle stays inside both boxes for 25 steps)
        spec["init_pos"] = X
        log, dones = replayed(spec, fragment(spec, policy_net(2 * spec["num_vehicles"]), K), K)
        a_wins, b_wins, replicas = degenerate_winners(log)
        assert replicas >= 2 and (a_wins if a_first else b_wins) >= 3 and (b_wins if a_first else a_wins) == 0
    spec = tail_spec(horizon=9)                              # the RL vehicle rams the parked one, or the time runs out
    log, dones = replayed(spec, fragment(spec, policy_net(2 * spec["num_vehicles"]), K), K)
    crash = np.array(log.crash)
    assert crash.any(axis=0).sum() >= 2 and (dones & ~crash).any()


GREEDY_TIES = [n for n in sorted(TIES) if TIES[n][0] != "approach"] + ["gap"]


@pytest.mark.parametrize("name", GREEDY_TIES)
def test_greedy_policy_keeps_the_rl_vehicle_exact_on_the_tie_layouts(name):
    """k_greedy_loop_policy with a zero-weight net: the mean action is its output bias, 0 -- the tie layouts unchanged."""
    K = 8
    spec = gap_tie_spec() if name == "gap" else tie_spec(name)
    res = fragment(spec, policy_net(2 * spec["num_vehicles"], bias=0.0), K, reset_done=False)
    assert (res[1] == 0).all()
    log, dones = replayed(spec, res, K, reset_done=False)
    assert_tie(name, log, dones, K)


def test_greedy_policy_with_a_dyadic_bias_on_the_cursor_table():
    """Mean action 1/2: the RL vehicle gains 1/16 m/s per step, exactly; the cursor events of the policy layout."""
    K = 31
    spec = policy_cursor_spec()
    res = fragment(spec, policy_net(2 * spec["num_vehicles"], bias=0.5), K)
    assert (res[1] == 0.5).all()
    log, dones = replayed(spec, res, K)
    assert_policy_cursor_events(log, dones)
    assert (np.array(log.v1)[:3, :, -1] == 8.0 + 0.0625 * np.arange(1, 4)[:, None]).all()


def test_pair_fragment_on_the_cursor_table_equals_the_pair_act_and_eager_steps():
    """k_loop_policy_pair against k_policy_pair_act + single steps (k_rollout_loop) + masked resets, and against the
    oracle's replay of the combined command."""
    import torch
    from test_policy_gpu import eager_obs0
    dev = torch.device("cuda", 0)
    K, w = 31, 0.5
    spec = policy_cursor_spec()
    R, D = spec["num_replicas"], 2 * spec["num_vehicles"]
    res = fragment(spec, policy_net(D, seed=3), K, pair=(policy_net(D, seed=4), w))
    sim = make(spec)
    sim.reset()
    av, adv = policy_net(D, seed=3), policy_net(D, seed=4)
    eo, er, ed = torch.zeros((K + 1, R, D), device=dev), torch.zeros((K, R), device=dev), torch.zeros((K, R), dtype=torch.uint8, device=dev)
    ea, elp, cmd = torch.zeros((K, 2, R), device=dev), torch.zeros((K, 2, R), device=dev), torch.zeros((K, R), device=dev)
    eo[0].copy_(torch.as_tensor(eager_obs0(sim), device=dev))
    torch.cuda.synchronize()
    for k in range(K):
        sim.policy_pair_act_dev(av.struct, adv.struct, w, eo[k], ea[k], elp[k], cmd[k])
        assert sim.last_kernel == "k_policy_pair_act"
        sim.step_dev(eo[k + 1], er[k], ed[k], cmd[k].reshape(R, 1))
        assert sim.last_kernel.startswith("k_rollout_loop")
        sim.reset_dev(eo[k + 1], ed[k])
    sim.sync()
    want = (eo, ea.permute(1, 0, 2).contiguous(), elp.permute(1, 0, 2).contiguous(), er, ed)
    for name, x, y in zip(("obs", "act", "logp", "rew", "done"), res, want):
        np.testing.assert_array_equal(x, y.cpu().numpy(), err_msg=name)
    np.testing.assert_array_equal(res[5], sim.pos)
    np.testing.assert_array_equal(res[6], sim.vel)
    cmd = cmd.cpu().numpy()
    sim.close()
    log, dones = replayed(spec, [res[0], cmd] + res[2:], K)
    assert_policy_cursor_events(log, dones)


# ------------------------------------------------------------------ FS_MIXED
def mixed_run(spec, K, exact):
    """Single steps and one launch on k_rollout_loop's float64-state instantiation against the float64 oracle."""
    acts = zero_actions(spec, K)
    ora, log, O, Rw, D, lim = oracle_rows(spec, acts, K, np.float64)
    crash = np.array(log.crash)
    sim = make(spec, "mixed")
    sim.reset()
    for k in range(K):
        o, r, d = sim.step(acts[k])
        assert sim.last_kernel.startswith("k_rollout_loop"), sim.last_kernel
        msg = "mixed, step %d" % k
        if exact:
            np.testing.assert_array_equal(sim.pos, log.x1[k], err_msg="pos: " + msg)
            np.testing.assert_array_equal(sim.vel, log.v1[k], err_msg="vel: " + msg)
        else:
            assert np.abs(sim.pos - log.x1[k]).max() < 1e-4 and np.abs(sim.vel - log.v1[k]).max() < 1e-4, msg
        np.testing.assert_array_equal(d, D[k], err_msg="done: " + msg)
        np.testing.assert_array_equal((sim.last_done_flags & 2) != 0, crash[k], err_msg="collision: " + msg)
        assert np.abs(o - O[k]).max() < 1e-6 and np.abs(r - Rw[k]).max() < 1e-5, msg
    sim.close()
    sim = make(spec, "mixed")
    sim.reset()
    obs, rew, done = launch(sim, K, acts)
    assert sim.last_kernel.startswith("k_rollout_loop")
    np.testing.assert_array_equal(done != 0, D)
    np.testing.assert_array_equal((done & 2) != 0, crash)
    assert np.abs(obs - O).max() < 1e-6 and np.abs(rew - Rw).max() < 1e-5
    if exact:
        np.testing.assert_array_equal(sim.pos, ora.x)
        np.testing.assert_array_equal(sim.vel, ora.v)
    else:
        assert np.abs(sim.pos - ora.x).max() < 1e-4 and np.abs(sim.vel - ora.v).max() < 1e-4
    sim.close()
    return log, D


@pytest.mark.parametrize("name", sorted(TIES))
def test_mixed_decides_crossing_ties_in_float64(name):
    """FS_MIXED takes the decisions of the crossing on float64 positions: the layouts one FLOAT64 ulp off their boundaries.
    Where all vehicles move exactly (the conflict zones) pos, vel and done equal the float64 oracle's; where a waiting IDM
    vehicle drives (its model runs in float32) the values keep 1e-4 -- a decision taken the other way moves the held
    vehicle by 0.1 m/s and more in one step."""
    K = 8
    log, done = mixed_run(tie_spec(name, np.float64), K, TIES[name][0] == "zone")
    assert_tie(name, log, done, K)


def test_mixed_collision_gap_one_float32_ulp_either_side():
    """h == crash_gap with the vehicle a FLOAT32 ulp (3.8e-6 m) off: the float32 gap the kernel tests holds the offset."""
    K = 8
    log, done = mixed_run(gap_tie_spec(np.float32), K, True)
    assert_tie("gap", log, done, K, np.float32)


@pytest.mark.parametrize("form", ["full", "delta2"])
def test_mixed_collision_gap_one_float64_ulp_either_side(form):
    """The vehicle one FLOAT64 ulp past the position where h == crash_gap: the float64 oracle has h = 0.5 - 1.4e-14 < 0.5,
    a collision in that step; the float32 gap the car-following models read is 0.5f.  k_rollout_loop<MX> decides on the
    float64 gap (it tested the float32 one, and reported the collision a step late): directly where every IDM exponent
    is 4, through the `h == crash_gap` branch in the instantiations with pow() ('delta2')."""
    K = 8
    log, done = mixed_run(with_form(gap_tie_spec(np.float64), form)[0], K, True)
    assert_tie("gap", log, done, K)


def test_mixed_tail_and_time_limit():
    spec = tail_spec(follower=False)
    log, done = mixed_run(spec, TAIL_K, True)
    first = tuple(int(np.argmax(done[:, r])) if done[:, r].any() else None for r in range(done.shape[1]))
    assert first == TAIL_FIRST_CRASH
    for H, K in [(2, 11), (5, 11), (7, 11), (8, 9), (9, 10), (10, 11)]:
        mixed_run(tail_spec(follower=False, horizon=H), K, True)
