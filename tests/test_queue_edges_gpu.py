"""`k_merge_queue` (flow_amd/csrc/flowsim_queue.h) at the edges of its event handler, against the float32 oracle
(oracle/opennet.py; QueueMergeOracle is that oracle with the queue formulation asserted on top) bit for bit through the C
ABI, noise off: a wave with all 64 lanes alive, two joins / arrivals / insertions in ONE sub-step, equal positions at the
join, at the tail an insertion is checked against and in the re-sort, a ramp vehicle that joins and arrives at once, a
list of 32 places, inflow schedules at begin 0 / a period of one sub-step / float64 equality / number / end, the
hand-over to and from the slot-order kernel, the fused policy with in-place resets of a full wave.

The layouts are constructed (tests/helpers.py holds them; tests/test_queue_model.py proves the queue formulation on them
on the CPU):
organic runs of helpers.merge_spec never fill the wave and never see two events of a kind in a sub-step.  Every test
asserts, on the ORACLE's side, that the event it is named for happened: a layout that stops reaching its edge fails
instead of passing.  Those are conditions on the inputs, not tolerances.  Every case runs by stepping (state compared
after every step) and again as ONE launch of the same length (a launch start rebuilds the queues, the pending inflows,
the next due index and the follower snapshot from the slot arrays); the two are equal in every emitted row and field."""
import numpy as np
import pytest

from helpers import (FULL_WAVE_PO, ReferenceLists, SubSteps, action_tape, assert_full_wave, assert_schedule,
                     assert_two_of_each, full_wave_spec, join_tie_spec, places32_spec, resort_tie_spec, schedule_spec,
                     tail_tie_spec, through_spec, two_spec)
from oracle import opennet as O
from oracle.queuenet import QueueMergeOracle
from test_open_gpu import compare_state, make
from test_queue_gpu import nan_actions

pytestmark = pytest.mark.gpu


def fields():
    from flow_amd import _lib as L
    return (L.FS_FIELD_POS, L.FS_FIELD_VEL, L.FS_FIELD_PREV_VEL, L.FS_FIELD_ACCEL, L.FS_FIELD_ROUTE, L.FS_FIELD_SEQ,
            L.FS_FIELD_ORIGIN, L.FS_FIELD_FOLLOWER, L.FS_FIELD_LEADER, L.FS_FIELD_HEADWAY, L.FS_FIELD_ARRIVED_RL,
            L.FS_FIELD_COUNTERS, L.FS_FIELD_MAX_SPEED, L.FS_FIELD_CTL_SEQ)


def reset_pair(sim, ora, mask=None):
    np.testing.assert_array_equal(sim.reset(mask), ora.reset(mask).astype(np.float32))
    compare_state(sim, ora)


def step_pair(sim, ora, a, k):
    o_ref, r_ref, d_ref = ora.step(a)
    o_gpu, r_gpu, d_gpu = sim.step(a)
    assert sim.last_kernel == "k_merge_queue", "step %d ran on %s" % (k, sim.last_kernel)
    np.testing.assert_array_equal(o_gpu, o_ref.astype(np.float32), err_msg="obs, step %d" % k)
    np.testing.assert_array_equal(r_gpu, r_ref.astype(np.float32), err_msg="reward, step %d" % k)
    np.testing.assert_array_equal(d_gpu, d_ref, err_msg="done, step %d" % k)
    compare_state(sim, ora)                              # (every step: the state right after the event)
    return o_gpu.copy(), r_gpu.copy(), d_gpu.copy()


def stepped(spec, acts, K, oracle=QueueMergeOracle, resets=None, hooks=(), each=None):
    """K steps on the kernel and on the oracle, everything compared after every step; `resets` = {step: mask} resets the
    masked replicas before that step.  -> (oracle, SubSteps, the rows of every step, every state field at the end)."""
    ora = oracle(spec, np.float32)
    sub = SubSteps(ora)
    extra = [h(ora) for h in hooks]
    sim = make(spec, "f32")
    reset_pair(sim, ora)
    rows = []
    for k in range(K):
        if resets and k in resets:
            reset_pair(sim, ora, resets[k])
        rows.append(step_pair(sim, ora, None if acts is None else acts[k], k))
        if each is not None:
            each(k, ora, rows[-1])
    np.testing.assert_array_equal(sim.time_counter, ora.time_counter)
    state = [sim.get_state(f) for f in fields()]
    sim.close()
    return (ora, sub, rows, state) + tuple(extra)


def launched(spec, acts, fragments, rows, state, resets=None):
    """The same run as launches of `fragments` steps each on a fresh handle: every row and, at the end, every field of
    every slot equals the stepped run's."""
    import torch
    dev = torch.device("cuda:0")
    R = spec["num_replicas"]
    sim = make(spec, "f32")
    sim.reset()
    acts_dev = None if acts is None else torch.from_numpy(np.ascontiguousarray(acts)).to(dev)
    k0 = 0
    for K in fragments:
        if resets and k0 in resets:
            sim.reset(resets[k0])
        out = (torch.empty((K, R, sim.obs_dim), dtype=torch.float32, device=dev),
               torch.empty((K, R), dtype=torch.float32, device=dev), torch.empty((K, R), dtype=torch.uint8, device=dev))
        sim.rollout_dev(K, *out, actions=None if acts is None else acts_dev[k0:k0 + K])
        sim.sync()
        assert sim.last_kernel == "k_merge_queue"
        obs, rew, done = [t.cpu().numpy() for t in out]
        for j in range(K):
            np.testing.assert_array_equal(obs[j], rows[k0 + j][0], err_msg="obs, step %d of launches %r" % (k0 + j, fragments))
            np.testing.assert_array_equal(rew[j], rows[k0 + j][1], err_msg="reward, step %d" % (k0 + j))
            np.testing.assert_array_equal(done[j].astype(bool), rows[k0 + j][2], err_msg="done, step %d" % (k0 + j))
        k0 += K
    assert k0 == len(rows)
    for f, want in zip(fields(), state):
        np.testing.assert_array_equal(sim.get_state(f), want, err_msg="field %d after launches %r" % (f, fragments))
    sim.close()


def odd_fragments(K):
    """K cut into launches of 1, 7, 3, 16, 5, 1, 7, ... steps."""
    out, cycle = [], (1, 7, 3, 16, 5)
    while sum(out) < K:
        out.append(min(cycle[len(out) % len(cycle)], K - sum(out)))
    return out


# ------------------------------------------------------------------ a: the full wave
@pytest.mark.parametrize("apply", [False, True])
def test_full_wave_multi_agent_head(apply):
    """64 of 64 lanes alive.  Oracle side, 400 steps, least of the two replicas (asserted at about half): 232 (actions
    applied: 263) sub-steps that start with 64 vehicles, 3 joins and 20 arrivals in such sub-steps, 19 insertions -- every
    one of them after an inflow waited for a slot -- 35 arrivals, no re-sort; observation, reward and counters compared in
    >= 100 steps that END with 64 vehicles (the reward's `n_alive < 64 ? mc_lane : o.max_cost_full`).  Actions with NaNs."""
    spec = full_wave_spec(ma_apply_actions=apply)
    acts = action_tape(nan_actions(2, 6, 13), 400)
    ends_full = []
    ora, sub, rows, state = stepped(spec, acts, 400, each=lambda k, o, row: ends_full.append((o.alive.sum(axis=1) == 64).all()))
    assert_full_wave(ora, sub)
    assert ora.resorts == 0 and sum(ends_full) >= 100
    launched(spec, acts, [400], rows, state)


def test_full_wave_single_agent_head():
    """MergePOEnv, num_rl = 6.  The layout as given has vehicles of both routes inside the junction at reset: the oracle
    reports a collision in step 0 (tests/test_queue_model.py asserts it), so the layout is spaced out by 40 m of free
    highway before the merge point.  Oracle side then: no collision in 400 steps, 176 sub-steps that start with 64 vehicles,
    4 joins and 11 arrivals from there, 16 insertions, 6 list entries made."""
    spec = full_wave_spec(env=O.ENV_MERGE_PO, **FULL_WAVE_PO)
    acts = action_tape(nan_actions(2, 6, 7, p_nan=0.0), 400)
    crashes = []
    ora, sub, rows, state = stepped(spec, acts, 400, each=lambda k, o, row: crashes.append(row[2].any()))
    assert not any(crashes) and sub.full_wave_figures(64)[0] >= 50
    assert_full_wave(ora, sub)
    launched(spec, acts, [400], rows, state)


def test_full_wave_five_sub_steps_per_step():
    """sims_per_step = 5 with the actions applied, 80 steps: an action (NaNs included) holds for five sub-steps.  Oracle
    side: 262 of the 400 sub-steps start with 64 vehicles, 3 joins and 20 arrivals from there, 19 insertions."""
    spec = full_wave_spec(sims_per_step=5, ma_apply_actions=True)
    acts = action_tape(nan_actions(2, 6, 13), 80)
    ora, sub, rows, state = stepped(spec, acts, 80)
    assert_full_wave(ora, sub)
    launched(spec, acts, [80], rows, state)


# ------------------------------------------------------------------ b: several events in one sub-step
@pytest.mark.parametrize("variant", ["one_sub_step", "two_sub_steps", "listed_rl_vehicle_arrives"])
def test_two_joins_two_arrivals_two_insertions_in_one_sub_step(variant):
    """sim_step 2 s.  Oracle side: sub-step 0 starts with 4 vehicles and has 2 joins, 2 arrivals, 2 insertions (asserted
    exactly); over the 20 steps 8 joins, 8 arrivals, 24 insertions and 6 re-sorts for the two replicas.  'two_sub_steps':
    sims_per_step 2.  'listed_rl_vehicle_arrives': MergePOEnv, the first vehicle is an RL vehicle that additional_command
    lists in sub-step 0, which then arrives -- arrival, ghost row and insertion in one sub-step."""
    po = variant == "listed_rl_vehicle_arrives"
    spec = two_spec(env=O.ENV_MERGE_PO if po else O.ENV_MERGE_MA, sims_per_step=2 if variant == "two_sub_steps" else 1,
                    rl_arrives=po)
    acts = np.full((20, 2, 2), 0.5, dtype=np.float32) if po else None
    ghosts = []
    ora, sub, rows, state = stepped(spec, acts, 20, each=lambda k, o, row: ghosts.append((row[0][:, 0::5] < -30).any()))
    assert_two_of_each(sub)
    assert ora.joins >= 4 and ora.resorts >= 1 and ora.total_arrived.min() >= 3
    if po:
        assert ghosts[0] and (ora.ctl_ctr >= 1).all()
    launched(spec, acts, [20], rows, state)


# ------------------------------------------------------------------ c: ties
@pytest.mark.parametrize("ramp_slot,highway_slot", [(2, 5), (5, 2)])
def test_join_at_bit_equal_positions_orders_by_slot(ramp_slot, highway_slot):
    """The join's `x == xe && lab < le`: highway and ramp vehicle pass the merge point at bit-equal x (329.42993) in step 2
    (asserted on the oracle: the join is in step 2, the positions are equal then, no re-sort helped)."""
    spec = join_tie_spec(ramp_slot, highway_slot, env=O.ENV_MERGE_MA)
    seen = []

    def each(k, o, row):
        seen.append((o.joins, bool((o.x[:, ramp_slot] == o.x[:, highway_slot]).all()), o.resorts))
    ora, sub, rows, state = stepped(spec, None, 8, each=each)
    assert [s[0] for s in seen[:3]] == [0, 0, 2] and seen[2][1] and seen[2][2] == 0
    launched(spec, None, [8], rows, state)


@pytest.mark.parametrize("moving_slot,resting_slot,speeds,enters", [(6, 7, (4.0, 0.0), 1), (7, 6, (4.0, 0.0), 0),
                                                                   (6, 7, (0.0, 0.0), 0)])
def test_insertion_against_a_tail_of_two_vehicles_at_one_position(moving_slot, resting_slot, speeds, enters):
    """The insertion's "vehicles AT the tail's position" loop.  Two RL vehicles (action 0, no speed-mode clamp: they keep
    their speed exactly) are at one position after sub-step 0, one at rest, one at 4 m/s; the inflow (begin 0) finds 24 m:
    enough behind the moving vehicle (21.3 m), not behind the one at rest (27.1 m).  The oracle's lowest-slot rule decides
    -- the vehicle enters in sub-step 0 iff the moving vehicle has the lower slot (asserted).  Third case: both at rest at
    equal init_pos for the whole run, nothing enters."""
    spec = tail_tie_spec(moving_slot, resting_slot, speeds=speeds)
    acts = np.zeros((6, 2, 4), dtype=np.float32)
    ora, sub, rows, state = stepped(spec, acts, 6)
    assert (sub.table()[2][0] == enters).all() and ora.resorts > 0
    if speeds == (0.0, 0.0):
        assert (ora.x[:, 6] == ora.x[:, 7]).all() and ora.total_departed.max() == 0
    launched(spec, acts, [6], rows, state)


def test_re_sort_with_three_vehicles_at_one_position():
    """Slots 8, 6, 7 (at rest, 4 m/s, 8 m/s; 0, 2, 4 m behind X) are all at X after sub-step 0: the re-sort ranks three
    equal positions by slot (oracle: queue order 6, 7, 8 asserted, 4 re-sorts in 6 steps)."""
    spec = resort_tie_spec()
    acts = np.zeros((6, 2, 4), dtype=np.float32)
    first = []
    ora, sub, rows, state = stepped(spec, acts, 6, each=lambda k, o, row: first.append(([a[:3] for a in o.A], o.x[:, 6:9].copy())))
    assert all(a == [6, 7, 8] for a in first[0][0]) and (first[0][1] == first[0][1][:, :1]).all() and ora.resorts >= 2
    launched(spec, acts, [6], rows, state)


# ------------------------------------------------------------------ d: the through-running ramp vehicle
@pytest.mark.parametrize("oracle", [O.MergeOracle, QueueMergeOracle])
@pytest.mark.parametrize("env", [O.ENV_MERGE_MA, O.ENV_MERGE_PO])
def test_ramp_vehicle_joins_and_arrives_in_one_sub_step(env, oracle):
    """sim_step 2 s, 50 m from the merge point to the end: slot 0 (ramp, 28 m/s, 4 m before the merge point) is past the
    END of the network after sub-step 0.  The kernel joins it into A and retires it as A's head in the same event.
    Oracle side: sub-step 0 has 1 arrival (slot 0) and, in the queue formulation, 1 join; 3 arrivals in 10 steps."""
    spec = through_spec(env=env)
    acts = None if env == O.ENV_MERGE_MA else np.zeros((10, 2, 4), dtype=np.float32)
    ora, sub, rows, state = stepped(spec, acts, 10, oracle=oracle)
    alive0, arrived, departed, joins = sub.table()
    assert (arrived[0] == 1).all() and ora.total_arrived.min() >= 2
    if oracle is QueueMergeOracle:
        assert (joins[0] == 1).all()
    launched(spec, acts, [10], rows, state)


# ------------------------------------------------------------------ e: a list of 32 places
def places32_actions(K, R):
    return np.random.default_rng(3).uniform(-0.5, 1.5, (K, R, 32)).astype(np.float32)


def test_list_of_32_places():
    """MergePOEnv, num_rl = 32, N = 64, three replicas, 300 steps: po_command's `1u << (place & 31)`, `below` and the
    __clz run length at places up to 31.  Replica 0: the list is in driving order (entries leave at place 0); replica 1:
    the RL slots reversed (they leave at place 31, 30, ...); replica 2 starts with 24 RL vehicles in the high slots, the RL
    inflow fills places 24 .. 31 from slots 32 .. 39, and its reset before step 40 leaves those eight as a run of departed
    entries that the removal loop takes in four passes.  Oracle side (MergePOEnv's own list statements run alongside and
    must give the oracle's list at every sub-step): 32 listed; skipped entries at places 20 22 24 26, 20 22, 20; ghost
    rows in 65 / 61 / 55 steps; ctl_ctr 89 / 90 / 86; no collision."""
    spec = places32_spec(R=3)
    acts = places32_actions(300, 3)
    resets = {40: np.array([0, 0, 1], dtype=bool)}
    ghost, crashed = np.zeros(3, dtype=int), []

    def each(k, o, row):
        ghost[:] += (row[0][:, 0::5] < -30).any(axis=1)
        crashed.append(row[2].any())
    ora, sub, rows, state, ref = stepped(spec, acts, 300, oracle=O.MergeOracle, resets=resets, hooks=(ReferenceLists,), each=each)
    assert ref.most_listed == 32 and (ghost >= 30).all() and (ora.ctl_ctr >= 60).all() and not any(crashed)
    assert len(ref.skipped_at) >= 4 and min(ref.skipped_at) > 16
    launched(spec, acts, [40, 260], rows, state, resets=resets)


def test_list_of_32_places_on_both_kernels_with_noise(monkeypatch):
    """The same spec with the acceleration noise on: one 150-step launch on k_merge_queue and, under FLOWSIM_NO_QUEUE=1, on
    k_steps_open -- every row, every field (the list and the counters in every slot)."""
    import torch
    from flow_amd import _lib as L
    spec = places32_spec(R=3)
    spec["vehicles"] = [dict(v, noise=0.2) if v["rl_index"] < 0 else v for v in spec["vehicles"]]
    K, R = 150, 3
    dev = torch.device("cuda:0")
    acts = torch.from_numpy(places32_actions(K, R)).to(dev)
    res = []
    for no_queue in ("0", "1"):
        monkeypatch.setenv("FLOWSIM_NO_QUEUE", no_queue)
        sim = make(spec, "f32")
        out = (torch.empty((K, R, sim.obs_dim), dtype=torch.float32, device=dev),
               torch.empty((K, R), dtype=torch.float32, device=dev), torch.empty((K, R), dtype=torch.uint8, device=dev))
        sim.reset()
        sim.rollout_dev(K, *out, actions=acts)
        sim.sync()
        res.append(([t.cpu().numpy() for t in out], [sim.get_state(f) for f in fields()], sim.last_kernel))
        sim.close()
    assert res[0][2] == "k_merge_queue" and res[1][2] == "k_steps_open"
    for x, y in zip(res[0][0], res[1][0]):
        np.testing.assert_array_equal(x, y)
    alive = res[0][1][fields().index(L.FS_FIELD_ROUTE)] >= 0
    for f, x, y in zip(fields(), res[0][1], res[1][1]):
        if f in (L.FS_FIELD_COUNTERS, L.FS_FIELD_ROUTE, L.FS_FIELD_ARRIVED_RL, L.FS_FIELD_CTL_SEQ):
            np.testing.assert_array_equal(x, y, err_msg="field %d" % f)
        else:
            np.testing.assert_array_equal(x[alive], y[alive], err_msg="field %d" % f)
    cnt = res[0][1][fields().index(L.FS_FIELD_COUNTERS)]
    assert (cnt[:, 2] >= 40).all() and (cnt[:, 5] >= 20).all()          # list entries made, arrivals


# ------------------------------------------------------------------ f: the inflow schedule
@pytest.mark.parametrize("which", ["always_due", "window"])
def test_inflow_schedules_at_their_edges(which):
    """due_index / my_due_of: begin = 0 (due_index's `!(t > 0)`), a period of one sub-step (a vehicle always waiting:
    pend_m never empties), period 3 * 0.2 against n * 0.2 in float64, number = 3, end = 20 s passed with ~90 due vehicles
    still outside.  Oracle side (tests/helpers.assert_schedule): 'always_due' -- both begin-0 inflows emit in
    sub-step 0, the numbered one stops at 3 (in steps 0, 6, 13), the others reach 16 and 6, the pool of 13 is full in 41
    steps; 'window' -- the vehicle due at 3 * (3 * 0.2) = 1.8000000000000003 s enters in step 9, not 8; the inflow that ends
    at 20 s has emitted 5 by then and 18 after 300 steps; the RL inflow with end = 11 s emits the vehicles due at 2, 6, 10 s
    (steps 49, 57, 65) and closes: the one of 14 s never comes.  Stepping, one launch, and launches of 1, 7, 3, 16, 5, ... steps."""
    spec = schedule_spec(which)
    emitted = []
    ora, sub, rows, state = stepped(spec, None, 300, each=lambda k, o, row: emitted.append(o.emitted[:, :4].copy()))
    assert_schedule(which, np.array(emitted))
    launched(spec, None, [300], rows, state)
    launched(spec, None, odd_fragments(300), rows, state)


# ------------------------------------------------------------------ g: hand-over on one handle
def test_full_wave_hand_over_between_the_queue_and_the_slot_order_kernel():
    """The full wave on ONE handle: 30 steps (k_merge_queue), a masked reset of replicas 0 and 2 (its zero-step launch
    runs on k_steps_open; they are back at 64 vehicles while 1 and 3 go on), 30 steps, a zero-step launch (a masked reset
    of nobody: the observation of the current state), 30 steps -- bit for bit against the oracle throughout.  Oracle side:
    every replica is at 64 vehicles at the hand-overs or within a step of them (>= 50 sub-steps start full in all)."""
    spec = full_wave_spec(R=4, ma_apply_actions=True)
    acts = action_tape(nan_actions(4, 6, 21), 90)
    ora = QueueMergeOracle(spec, np.float32)
    sub = SubSteps(ora)
    sim = make(spec, "f32")
    reset_pair(sim, ora)
    for k in range(30):
        step_pair(sim, ora, acts[k], k)
    before = ora.total_arrived.copy()
    assert before.min() >= 2
    mask = np.array([1, 0, 1, 0], dtype=bool)
    reset_pair(sim, ora, mask)
    assert sim.last_kernel == "k_steps_open"
    assert (ora.total_arrived[mask] == 0).all() and (ora.total_arrived[~mask] == before[~mask]).all()
    assert (ora.alive.sum(axis=1)[mask] == 64).all()
    for k in range(30, 60):
        step_pair(sim, ora, acts[k], k)
    nobody = np.zeros(4, dtype=bool)
    reset_pair(sim, ora, nobody)
    assert sim.last_kernel == "k_steps_open"
    for k in range(60, 90):
        step_pair(sim, ora, acts[k], k)
    assert sub.full_wave_figures(64)[0] >= 50 and ora.total_departed.min() >= 3
    sim.close()


# ------------------------------------------------------------------ h: the fused policy on the full wave
def test_fused_policy_resets_a_full_wave_in_place():
    """k_merge_queue<POLICY> ("k_merge_policy") on the multi-agent handle of case a, horizon 6 (the first vehicle needs 7
    steps to the end of the network: every episode ends with 64 vehicles in the wave), K = 20 after a stagger of 3 steps:
    replicas 0 and 2 are reset in place after steps 5, 11, 17 of the fragment, 1 and 3 after steps 2, 8, 14.  Equal to
    eager policy_act_dev + step_dev + reset_dev(done) bit for bit; the fragment's own actions replayed through the oracle
    give its observations and rewards, and the oracle says that every reset found 64 vehicles (asserted)."""
    import torch
    from test_policy_gpu import eager_obs0, make_policy_in
    from test_policy_merge_gpu import buffers, stagger
    dev = torch.device("cuda", 0)
    K, R, A, STAGGER = 20, 4, 6, 3
    spec = full_wave_spec(R=R, ma_apply_actions=True, horizon=6)
    pol_a, pol_b = make_policy_in(5, 2, False, seed=5), make_policy_in(5, 2, False, seed=5)
    fused, eager = make(spec, "f32"), make(spec, "f32")
    for sim in (fused, eager):
        stagger(sim, 5, steps=STAGGER)
    D = fused.obs_dim
    f = buffers(K, R, D, A)
    fused.policy_rollout_dev(pol_a.struct, K, *f, reset_done=True)
    fused.sync()
    assert fused.last_kernel == "k_merge_policy"
    e = buffers(K, R, D, A)
    eo, ea, elp, er, ed = e
    eo[0].copy_(torch.as_tensor(eager_obs0(eager), device=dev))
    torch.cuda.synchronize()
    for s in range(K):
        eager.policy_act_dev(pol_b.struct, eo[s], ea[s], elp[s])
        eager.step_dev(eo[s + 1], er[s], ed[s], ea[s])
        eager.reset_dev(eo[s + 1], ed[s])
    eager.sync()
    for name, x, y in zip(("obs", "act", "logp", "rew", "done"), f, e):
        np.testing.assert_array_equal(x.cpu().numpy(), y.cpu().numpy(), err_msg=name)
    for fld in fields():
        np.testing.assert_array_equal(fused.get_state(fld), eager.get_state(fld), err_msg="field %d" % fld)
    np.testing.assert_array_equal(fused.time_counter, eager.time_counter)
    # the oracle on the fragment's action tape
    on, an, rn, dn = f[0].cpu().numpy(), f[1].cpu().numpy(), f[3].cpu().numpy(), f[4].cpu().numpy()
    ora = QueueMergeOracle(spec, np.float32)
    ora.reset()
    pre = np.random.default_rng(5).uniform(-1.0, 1.0, (STAGGER, R, A)).astype(np.float32)       # (stagger's actions)
    for k in range(STAGGER):
        ora.step(pre[k])
    ora.reset(np.arange(R) % 2 == 0)
    np.testing.assert_array_equal(on[0], ora.get_state().astype(np.float32))
    resets, found = np.zeros(R, dtype=int), []
    for k in range(K):
        o_ref, r_ref, d_ref = ora.step(an[k])
        np.testing.assert_array_equal(rn[k], r_ref.astype(np.float32), err_msg="reward, step %d" % k)
        np.testing.assert_array_equal(dn[k] != 0, d_ref, err_msg="done, step %d" % k)
        if d_ref.any():
            found += list(ora.alive.sum(axis=1)[d_ref])
            resets += d_ref
            o_ref = ora.reset(d_ref)
        np.testing.assert_array_equal(on[k + 1], o_ref.astype(np.float32), err_msg="obs, step %d" % k)
    compare_state(fused, ora)
    assert (resets == 3).all() and found == [64] * 12
    assert (~np.isnan(an)).all()                        # all six agents present throughout: six network passes per step
    fused.close(), eager.close()
