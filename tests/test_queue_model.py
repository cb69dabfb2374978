"""The queue formulation of the open-network neighbour rules (oracle/queuenet.py: what the HIP kernel k_merge_queue keeps
instead of comparing pairs) equals the all-pairs statement of oracle/opennet.py -- leader, headway, sticky follower --
at every sub-step, through insertions, arrivals, merges and collisions (re-sorts).  CPU only."""
import numpy as np
import pytest

from helpers import (FULL_WAVE_PO, ReferenceLists, SubSteps, action_tape, assert_full_wave, assert_schedule,
                     assert_two_of_each, full_wave_spec, join_tie_spec, merge_spec, nan_actions, places32_spec,
                     resort_tie_spec, schedule_spec, tail_tie_spec, through_spec, tie_at_the_join, two_spec)
from oracle import opennet as O
from oracle.queuenet import QueueMergeOracle


def quiet(spec):
    spec = dict(spec)
    spec["vehicles"] = [dict(v, noise=0.0) for v in spec["vehicles"]]
    return spec


@pytest.mark.parametrize("seed", [1, 2, 7, 8, 11])
@pytest.mark.parametrize("env", [O.ENV_MERGE_MA, O.ENV_MERGE_PO])
def test_queue_structure_gives_the_all_pairs_neighbours(seed, env):
    kw = dict(R=3, cap_human=20 + seed % 5, cap_rl=4, num_rl=2, horizon=200, seed=seed, env=env,
              q_highway=1500 + 100 * seed, q_merge=200 + 80 * seed, sims_per_step=1 + seed % 3)
    if seed % 4 == 3:
        kw["sim_step"] = 0.5
    spec = quiet(merge_spec(**kw))
    if seed % 3 == 2:                                   # "aggressive": nobody obeys SUMO's safe speed -> collisions
        spec["vehicles"] = [dict(v, speed_mode=0) for v in spec["vehicles"]]
    q = QueueMergeOracle(spec, np.float32)
    q.reset()
    rng = np.random.default_rng(seed)
    for _ in range(200):
        q.step(rng.uniform(-1.0, 1.5, (3, spec["num_rl"])).astype(np.float32))      # (every sub-step asserts)
    assert q.checks >= 3 * 200 and q.joins > 0 and q.total_arrived.sum() > 0
    if seed in (8, 11) and env == O.ENV_MERGE_MA:
        assert q.resorts > 0                            # the collision runs went through the re-sort


def run_model(spec, acts, K):
    """K steps of the queue formulation (every sub-step asserts it against the all-pairs rule) -> (oracle, SubSteps)."""
    q = QueueMergeOracle(spec, np.float32)
    sub = SubSteps(q)
    q.reset()
    for k in range(K):
        q.step(None if acts is None else acts[k])
    assert q.checks >= q.R * K
    return q, sub


@pytest.mark.parametrize("apply", [False, True])
def test_queue_structure_on_a_full_wave(apply):
    """a. 64 of 64 slots alive: the join with nA + n1 = 64 (lane nA is U1's tail, not a dead lane), arrivals with no dead
    lane behind A, insertions refused for lack of a slot.  No re-sort (asserted: the structure is held by the events alone)."""
    spec = full_wave_spec(ma_apply_actions=apply)
    q, sub = run_model(spec, action_tape(nan_actions(2, 6, 13), 400), 400)
    assert_full_wave(q, sub)
    assert q.resorts == 0


def test_queue_structure_on_a_full_wave_of_the_single_agent_head():
    """a, MergePOEnv.  The layout as given puts vehicles of both routes into the junction at reset: a collision in step 0
    (measured: done in step 0, every step after it too).  Spaced out by 40 m of free highway before the merge point, the
    head of the ramp goes first and the run shows 176 sub-steps that start with 64 vehicles before any collision (none in
    400 steps)."""
    dense = O.MergeOracle(full_wave_spec(env=O.ENV_MERGE_PO), np.float32)
    dense.reset()
    assert dense.step(np.zeros((2, 6), dtype=np.float32))[2].all()
    spec = full_wave_spec(env=O.ENV_MERGE_PO, **FULL_WAVE_PO)
    acts = action_tape(nan_actions(2, 6, 7, p_nan=0.0), 400)
    q = QueueMergeOracle(spec, np.float32)
    sub = SubSteps(q)
    q.reset()
    first_crash = None
    for k in range(400):
        if q.step(acts[k])[2].any() and first_crash is None:
            first_crash = k
    assert first_crash is None
    assert_full_wave(q, sub)
    assert (q.ctl_ctr >= 6).all()


@pytest.mark.parametrize("variant", ["one_sub_step", "two_sub_steps", "listed_rl_vehicle_arrives"])
def test_queue_structure_with_two_of_every_event_in_one_sub_step(variant):
    """b. sim_step 2 s: sub-step 0 has 2 joins, 2 arrivals and 2 insertions (the second iteration of each of the
    kernel's event loops); measured over 20 steps: 8 joins, 8 arrivals, 24 insertions, 6 re-sorts per replica pair."""
    spec = two_spec(env=O.ENV_MERGE_PO if variant == "listed_rl_vehicle_arrives" else O.ENV_MERGE_MA,
                    sims_per_step=2 if variant == "two_sub_steps" else 1, rl_arrives=variant == "listed_rl_vehicle_arrives")
    acts = None if spec["env"] == O.ENV_MERGE_MA else np.full((20, 2, 2), 0.5, dtype=np.float32)
    q, sub = run_model(spec, acts, 20)
    assert_two_of_each(sub)


@pytest.mark.parametrize("ramp_slot,highway_slot", [(2, 5), (5, 2)])
def test_queue_structure_orders_a_tie_at_the_join_by_slot(ramp_slot, highway_slot):
    """c. `x == xe && lab < le`: the two pass the merge point at bit-equal x (329.42993) in step 2."""
    spec = join_tie_spec(ramp_slot, highway_slot, env=O.ENV_MERGE_MA)
    q = QueueMergeOracle(spec, np.float32)
    q.reset()
    for k in range(3):
        q.step(None)
        assert (q.joins > 0) == (k == 2)
    assert tie_at_the_join(q, ramp_slot, highway_slot) and q.resorts == 0
    assert all(a[:2] == sorted([ramp_slot, highway_slot]) for a in q.A)
    for k in range(5):
        q.step(None)


@pytest.mark.parametrize("moving_slot,resting_slot,enters", [(6, 7, True), (7, 6, False)])
def test_queue_structure_checks_an_insertion_against_the_lowest_slot_of_a_tied_tail(moving_slot, resting_slot, enters):
    """c. Two vehicles at one position are the tail of the highway's queue, one at rest, one at 4 m/s: the gap of 24 m is
    enough behind the moving one only.  The oracle's rule (the lowest slot) decides: the vehicle enters in sub-step 0 iff
    the moving vehicle has the lower slot."""
    spec = tail_tie_spec(moving_slot, resting_slot)
    q, sub = run_model(spec, np.zeros((6, 2, 4), dtype=np.float32), 6)
    assert (sub.table()[2][0] == int(enters)).all() and q.resorts > 0


def test_queue_structure_checks_an_insertion_against_two_vehicles_at_rest_at_one_position():
    """c. Equal init_pos, init_vel = 0, both held at rest (RL vehicles with action 0: no command moves them): the tail of
    two every sub-step; the gap of 24 m is too small behind a vehicle at rest, nothing enters."""
    spec = tail_tie_spec(6, 7, speeds=(0.0, 0.0))
    q, sub = run_model(spec, np.zeros((6, 2, 4), dtype=np.float32), 6)
    assert (q.x[:, 6] == q.x[:, 7]).all() and (q.v[:, [6, 7]] == 0).all() and q.total_departed.max() == 0


def test_queue_structure_re_sorts_three_vehicles_at_one_position():
    spec = resort_tie_spec()
    q = QueueMergeOracle(spec, np.float32)
    q.reset()
    q.step(np.zeros((2, 4), dtype=np.float32))
    assert (q.x[:, 6] == q.x[:, 8]).all() and (q.x[:, 7] == q.x[:, 8]).all() and q.resorts > 0
    assert all(a[:3] == [6, 7, 8] for a in q.A)
    for _ in range(5):
        q.step(np.zeros((2, 4), dtype=np.float32))


@pytest.mark.parametrize("env", [O.ENV_MERGE_MA, O.ENV_MERGE_PO])
def test_queue_structure_lets_a_ramp_vehicle_join_and_arrive_in_one_sub_step(env):
    """d. The order of the events is the kernel's: re-sort, join, arrivals, insertions.  (With the arrivals taken from
    the head of A before the join, this layout raised AssertionError (0, [], {0}).)"""
    spec = through_spec(env=env)
    q, sub = run_model(spec, None if env == O.ENV_MERGE_MA else np.zeros((10, 2, 4), dtype=np.float32), 10)
    alive0, arrived, departed, joins = sub.table()
    assert (joins[0] == 1).all() and (arrived[0] == 1).all() and (q.route[:, 0] != 1).all()


@pytest.mark.parametrize("which", ["always_due", "window"])
def test_queue_structure_under_inflow_schedules_at_their_edges(which):
    spec = schedule_spec(which)
    q = QueueMergeOracle(spec, np.float32)
    q.reset()
    emitted = []
    for _ in range(300):
        q.step(None)
        emitted.append(q.emitted[:, :4].copy())
    assert_schedule(which, np.array(emitted))


def test_merge_po_list_of_32_places_follows_the_reference_list_operations():
    """e on the CPU: 32 places, the list held to MergePOEnv's own list statements at every sub-step of three replicas --
    driving order, reversed, and one whose reset leaves a run of eight departed entries at places 20 .. 27 (the removal
    loop skips every second one: measured skipped places 20 22 24 26, 20 22, 20)."""
    spec = places32_spec(R=3)
    ora = O.MergeOracle(spec, np.float32)
    ref = ReferenceLists(ora)
    ora.reset()
    rng = np.random.default_rng(3)
    for k in range(80):
        if k == 40:
            ora.reset(np.array([0, 0, 1], dtype=bool))
        ora.step(rng.uniform(-0.5, 1.5, (3, 32)).astype(np.float32))
    assert ref.most_listed == 32 and len(ref.skipped_at) >= 4 and min(ref.skipped_at) > 16
