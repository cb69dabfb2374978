"""The constructed layouts of tests/test_loop_edges_gpu.py reach the events they are named for -- proven on the oracle
alone (oracle/refsim.py RingOracle), in float32 (the kernels' twin) and in float64 (FS_MIXED's reference).  The GPU tests
repeat these assertions on the oracle's side of every comparison: a layout that stops reaching its edge fails there too.
These are conditions on inputs, not tolerances."""
import numpy as np
import pytest

from helpers import (CURSOR_N, LOOP_FORMS, ODD_CYCLE, SHORT_CYCLE, TAIL_FIRST_CRASH, TAIL_K, TIES, TIE_J, TIE_L, TIE_SEGS, LoopLog,
                     assert_cursor_events, assert_policy_cursor_events, assert_tie, cursor_spec, degenerate_spec,
                     degenerate_winners, fragments_of, gap_tie_spec, loop_edge_spec, oracle_rows, policy_cursor_spec,
                     rl_mover, shape_spec, start_for, start_phases, tail_spec, tie_spec, ulps, with_form, zero_actions)
from oracle import refsim as S

DTYPES = [np.float32, np.float64]


@pytest.mark.parametrize("dtype", DTYPES)
def test_an_rl_vehicle_without_clamps_moves_exactly(dtype):
    """x0 = 1, v = 4, dt = 1/8: x == a_in = 32 after 62 steps, in both types; a dyadic action keeps the speed dyadic."""
    spec = loop_edge_spec(TIE_L, TIE_SEGS, TIE_J, [rl_mover(0), rl_mover(1)], [[1.0, 129.0]], [[4.0, 4.0]])
    ora = S.RingOracle(spec, dtype)
    ora.reset()
    for k in range(62):
        ora.step(np.zeros((1, 2), np.float32))
    assert ora.x[0, 0] == 32.0 and ora.v[0, 0] == 4.0
    ora.step(np.array([[0.5, -0.25]], np.float32))
    assert ora.v[0, 0] == 4.0625 and ora.v[0, 1] == 3.96875 and ora.x[0, 0] == 32.0 + 4.0625 / 8


@pytest.mark.parametrize("dtype", DTYPES)
def test_start_for_lands_on_the_ulp(dtype):
    for target in (32.0, 160.0, 24.0, 94.5):
        for off in (-1, 0, 1):
            for steps in (0, 1, 5):
                t = ulps(target, off, dtype)
                x = start_for(t, 4.0, steps, dtype)
                for _ in range(steps):
                    x = dtype(x + dtype(0.5))
                assert x == t and (off == 0 or t != dtype(target))


@pytest.mark.parametrize("form", LOOP_FORMS)
@pytest.mark.parametrize("full16", [True, False])
def test_cursor_layout_reaches_every_event(full16, form):
    spec = with_form(cursor_spec(full16), form)[0]
    K = 200
    ora, log, obs, rew, done, _ = oracle_rows(spec, zero_actions(spec, K), K)
    ev = assert_cursor_events(log)
    assert len(spec["segments"]) == (16 if full16 else 10)
    # the RL vehicles kept their speeds: the events above are the constructed ones
    rl = [i for i in range(CURSOR_N) if i != CURSOR_N - 2]
    assert (ora.v[:, rl] == np.asarray(spec["init_vel"])[:, rl]).all()
    # the cursor is visible: the IDM vehicle is on internal rows (uncommanded) and on edges, positions come from every row
    x0 = log.arrays()[0][:, :, CURSOR_N - 2]
    inside = ora.in_junction(x0)
    assert inside.any(axis=0).sum() >= (4 if full16 else 2) and (~inside).any(axis=0).all()      # (the 10-row table's internal rows are 1/8 m long)
    rows = np.unique(np.floor((obs[:, :, CURSOR_N:] * 192.0 - 1000.0) / 64.0 + 1e-3))
    assert len(rows) == len(spec["segments"]), rows
    print({k: v.tolist() for k, v in ev.items()})


def test_cursor_layout_with_one_rl_vehicle_under_random_actions():
    """The policy kernels' population (ONE RL vehicle): whatever a policy commands inside [-1, 1], 60 steps contain steps
    that pass three starts, wrap and advance, and episodes of 3 steps that end on a step that changes the segment."""
    spec = policy_cursor_spec()
    rng = np.random.default_rng(3)
    for trial in range(3):
        acts = rng.uniform(-1, 1, (60, 8, 1)).astype(np.float32)
        ora = S.RingOracle(spec, np.float32)
        log = LoopLog(ora)
        ora.reset()
        dones = []
        for k in range(60):
            dones.append(ora.step(acts[k])[2])
            if dones[-1].any():
                ora.reset(dones[-1])
        assert_policy_cursor_events(log, np.array(dones))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(TIES) + ["gap"])
def test_tie_layouts_sit_on_the_boundary_and_decide_as_stated(name, dtype):
    K = 8
    for form in LOOP_FORMS:
        spec = gap_tie_spec(dtype) if name == "gap" else tie_spec(name, dtype)
        spec = with_form(spec, form)[0]
        ora, log, _, _, done, _ = oracle_rows(spec, zero_actions(spec, K), K, dtype)
        assert_tie(name, log, done, K)
        assert (ora.v[:, 2:] == 0).all() and (ora.x[:, 2:] == np.asarray(spec["init_pos"])[:, 2:]).all()    # parked, noise and all


@pytest.mark.parametrize("a_first", [True, False])
def test_degenerate_table_blocks_both_lines_and_each_stream_binds_once(a_first):
    spec = degenerate_spec(a_first)
    ora, log, _, _, done, _ = oracle_rows(spec, zero_actions(spec, 60), 60)
    a_wins, b_wins, replicas = degenerate_winners(log)
    print(a_wins, b_wins, replicas)
    assert replicas >= 2 and (a_wins if a_first else b_wins) >= 3 and (b_wins if a_first else a_wins) == 0
    line = min(spec["junction"]["a_in"], spec["junction"]["b_in"])
    assert (ora.x[:, 1] < line).all() and (ora.x[:, 1] > line - 4.0).all() and not done.any()    # it stopped at the nearer line


def test_tail_layout_crashes_in_every_slot_and_the_fragments_start_in_every_phase():
    spec = tail_spec()
    _, _, _, _, done, _ = oracle_rows(spec, zero_actions(spec, TAIL_K), TAIL_K)
    first = [int(np.argmax(done[:, r])) if done[:, r].any() else None for r in range(done.shape[1])]
    assert tuple(first) == TAIL_FIRST_CRASH
    assert {c % 4 for c in first if c is not None and c < 8} == {0, 1, 2, 3} and {8, 9, 10} <= set(first)
    for H in (1, 2, 3, 5, 6, 7, 10):
        _, _, _, _, done, lim = oracle_rows(tail_spec(horizon=H), zero_actions(spec, TAIL_K), TAIL_K)
        assert int(np.argmax(lim[:, 7])) == H - 1 and (done[:, 7] == lim[:, 7]).all()
    assert start_phases(fragments_of(61, ODD_CYCLE)) | start_phases(fragments_of(61, SHORT_CYCLE)) == {0, 1, 2, 3}
    assert {1, 2, 3} <= set(fragments_of(61, SHORT_CYCLE))


@pytest.mark.parametrize("N,R", [(2, 1), (2, 5), (9, 5), (16, 1), (16, 5)])
def test_shape_layouts_keep_moving_through_the_clusters(N, R):
    spec = shape_spec(N, R)
    K = 40
    ora, log, _, _, done, _ = oracle_rows(spec, zero_actions(spec, K), K)
    ev = log.cursor_events()
    assert ev["pass3"].sum() + ev["pass4"].sum() >= 1 and ev["changed"].sum() >= 4 * R and not done.any(), ev
    if N == 16:
        assert ev["last_wrap"].sum() >= 1        # somebody passed L


def test_multi_agent_shape_layout():
    spec = shape_spec(12, 5, env=S.ENV_ACCEL_PO_MA, rl_slots=(0, 5, 6, 11))
    ora, log, obs, _, done, _ = oracle_rows(spec, zero_actions(spec, 40), 40)
    ev = log.cursor_events()
    assert obs.shape[2] == 24 and ev["changed"].sum() >= 6 and ev["last_wrap"].sum() >= 1 and not done.any()
