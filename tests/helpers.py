"""Shared spec builders for the oracle and the parity tests (plain dicts; the same
dict feeds oracle.refsim.RingOracle and flow_amd.sim.FlowSim)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import network as Net   # noqa: E402
from oracle import refsim as S      # noqa: E402
from oracle.opennet import ENV_MERGE_MA   # noqa: E402

IDM_DEFAULT = [30, 1, 1, 1.5, 4, 2, 0, 0]       # car_following_models.py:437-447


def idm_vehicle(**kw):
    d = dict(controller=S.CTRL_IDM, p=IDM_DEFAULT, fail_safe=S.FAILSAFE_NONE, noise=0.0, delay=0.0,
             max_accel=2.6, max_decel=4.5, length=5.0, speed_mode=0, sumo_tau=1.0, sumo_min_gap=2.5,
             sumo_max_speed=30.0, rl_index=-1, initial_speed=0.0)
    d.update(kw)
    return d


def ring_spec(R=1, N=22, length=230.0, bunching=20.0, junction_length=0.0, horizon=1500, **kw):
    net = Net.ring_network(length, junction_length=junction_length)
    pos, _ = net.gen_even_start_pos(N, bunching=bunching)
    x0 = np.array([net.get_x(e, p) for e, p in pos])
    spec = dict(num_replicas=R, num_vehicles=N, num_rl=0, sim_step=0.1, junction_length=junction_length,
                ring_length=np.full(R, length), max_speed=30.0, env=S.ENV_ACCEL, target_velocity=10.0,
                action_low=-3.0, action_high=3.0, horizon=horizon, warmup_steps=0, sims_per_step=1,
                vehicles=[idm_vehicle() for _ in range(N)], init_pos=np.tile(x0, (R, 1)))
    spec.update(kw)
    return spec




def multilane_spec(R=4, N=21, lanes=3, length=230.0, horizon=100, n_rl=0, seed=0, junction_length=0.1, **kw):
    """RingNetwork with ``lanes`` lanes: vehicles placed side by side as gen_even_start_pos does
    (network/base.py:372-378), optionally with ``n_rl`` RL vehicles in the last slots."""
    net = Net.ring_network(length, lanes=lanes, junction_length=junction_length)
    pos, start_lanes = net.gen_even_start_pos(N)
    x0 = np.array([net.get_x(e, p) for e, p in pos])
    rng = np.random.default_rng(seed)
    X = np.tile(x0, (R, 1)) + np.abs(rng.normal(0, 0.2, (R, N)))
    veh = [idm_vehicle() for _ in range(N)]
    for k in range(n_rl):
        veh[N - n_rl + k] = idm_vehicle(controller=S.CTRL_RL, rl_index=k)
    spec = dict(num_replicas=R, num_vehicles=N, num_rl=n_rl, sim_step=0.1, junction_length=junction_length,
                ring_length=np.full(R, length), max_speed=30.0, env=S.ENV_LANE_CHANGE_ACCEL, target_velocity=10.0,
                action_low=-3.0, action_high=3.0, horizon=horizon, warmup_steps=0, sims_per_step=1,
                vehicles=veh, init_pos=X, num_lanes=lanes, init_lane=np.tile(np.array(start_lanes, dtype=np.int32), (R, 1)),
                lane_change_duration=5, lane_change_mode=512, last_lc_quirk=True)
    spec.update(kw)
    return spec


def figure_eight_tables(radius=30.0, lanes=1, junction_length=0.1, center_length=9.4, half_width=0.9,
                        veh_len=5.0, time_gap=3.0):
    """Physical segment table + crossing model of a one-lane figure eight, written out literally here so
    the tests do not depend on the product's network class: (phys_start, internal, flow_start, flow_slope)
    in route order bottom -> top -> upper_ring -> right -> left -> lower_ring (networks/figure_eight.py:189-206),
    flow_* from Flow's edge-start tables (figure_eight.py:225-263; internal edges without a table entry fall
    back to a constant, network/traci.py:280-287)."""
    net = Net.figure_eight_network(radius, lanes, center_length=center_length, junction_length=junction_length)
    tab = net.total_edgestarts_dict
    e = radius * np.pi / 2.0
    order = [("bottom", radius, False, tab["bottom"], 1.0),
             (":center_1", center_length, True, tab[":center_1"], 1.0),
             ("top", radius, False, tab["top"], 1.0),
             (":top_0", junction_length, True, tab[":top"], 0.0),
             ("upper_ring", 3 * e, False, tab["upper_ring"], 1.0),
             (":right_0", junction_length, True, tab[":right"], 0.0),
             ("right", radius, False, tab["right"], 1.0),
             (":center_0", center_length, True, tab[":center_0"], 1.0),
             ("left", radius, False, tab["left"], 1.0),
             (":left_0", junction_length, True, tab[":left"], 0.0),
             ("lower_ring", 3 * e, False, tab["lower_ring"], 1.0),
             (":bottom_0", junction_length, True, tab[":bottom"], 0.0)]
    segs, starts, s0 = [], {}, 0.0
    for name, length, internal, fs, slope in order:
        segs.append((s0, internal, fs, slope))
        starts[name] = s0
        s0 += length
    a_in, b_in = starts[":center_1"], starts[":center_0"]
    junction = dict(a_in=a_in, a_out=a_in + center_length, b_in=b_in, b_out=b_in + center_length,
                    lookahead=radius, time_gap=time_gap,
                    za_lo=a_in + center_length / 2 - half_width, za_hi=a_in + center_length / 2 + veh_len + half_width,
                    zb_lo=b_in + center_length / 2 - half_width, zb_hi=b_in + center_length / 2 + veh_len + half_width)
    return segs, junction, s0, starts, net


def figure_eight_spec(R=4, N=14, radius=30.0, horizon=200, seed=0, junction_length=0.1, center_length=9.4, **kw):
    """FigureEightNetwork, N vehicles placed by gen_even_start_pos (table coordinates -> loop coordinates)."""
    segs, junction, total, starts, net = figure_eight_tables(radius, 1, junction_length, center_length)
    pos, _ = net.gen_even_start_pos(N)
    x0 = np.array([starts[e] + p for e, p in pos])
    order = np.argsort(x0)
    assert (order == np.arange(N)).all()
    rng = np.random.default_rng(seed)
    X = np.tile(x0, (R, 1)) + np.abs(rng.normal(0, 0.2, (R, N)))
    veh = [idm_vehicle(speed_mode=1, max_decel=1.5) for _ in range(N)]
    spec = dict(num_replicas=R, num_vehicles=N, num_rl=0, sim_step=0.1, junction_length=junction_length,
                ring_length=np.full(R, total - 4 * junction_length), max_speed=30.0, env=S.ENV_ACCEL,
                target_velocity=20.0, action_low=-3.0, action_high=3.0, horizon=horizon, warmup_steps=0,
                sims_per_step=1, vehicles=veh, init_pos=X, junction_mode=1, segments=segs, junction=junction)
    spec.update(kw)
    return spec


def merge_tables(pre=200.0, merge=100.0, post=100.0, junction_length=0.1, center_length=22.5, inflow_len=100.0):
    """Route tables of MergeNetwork written out literally (independent of flow_amd.networks.merge so the
    host mirror can be checked against it).  Both routes share one coordinate with the merge point (start
    of edge 'center') at merge_x; Flow's edge-start table is flow/networks/merge.py:198-216; internal edges
    resolve to their table entry without the position (network/traci.py:280-287, slope 0)."""
    j, J = junction_length, center_length
    up0 = inflow_len + j + pre + J                  # length of the highway route upstream of the merge point
    up1 = inflow_len + j + merge + J
    merge_x = max(up0, up1)
    s0, s1 = merge_x - up0, merge_x - up1
    c_start = inflow_len + pre + 22.6               # ("center", INFLOW_EDGE_LEN + premerge + 22.6)
    r0 = [(s0, 0, 0.0, 1.0), (s0 + inflow_len, 1, inflow_len, 0.0), (s0 + inflow_len + j, 0, inflow_len + 0.1, 1.0),
          (s0 + inflow_len + j + pre, 1, inflow_len + pre + 0.1, 0.0), (merge_x, 0, c_start, 1.0)]
    im = inflow_len + pre + post + 22.6             # ("inflow_merge", ...)
    r1 = [(s1, 0, im, 1.0), (s1 + inflow_len, 1, 2 * inflow_len + pre + post + 22.6, 0.0),
          (s1 + inflow_len + j, 0, 2 * inflow_len + pre + post + 22.7, 1.0),
          (s1 + inflow_len + j + merge, 1, inflow_len + pre + 0.1, 0.0), (merge_x, 0, c_start, 1.0)]
    net_length = 2 * inflow_len + pre + merge + post + 2 * j + 2 * J
    return dict(routes=[dict(start=s0, segments=r0), dict(start=s1, segments=r1)], merge_x=merge_x,
                box_in=merge_x - J, end_x=merge_x + post, net_length=net_length)


def merge_spec(R=4, cap_human=12, cap_rl=4, num_rl=2, pre=200.0, merge=100.0, post=100.0, horizon=200, seed=0,
               q_highway=1800.0, q_rl=200.0, q_merge=300.0, n_init=3, env=None, time_gap=1.0, **kw):
    """MergeNetwork + MergePOEnv-like spec: IDM humans (noise 0.2, obey_safe_speed) and RL vehicles entering
    through three inflows as in examples/exp_configs/rl/multiagent/multiagent_merge.py:46-83."""
    from oracle import opennet as O
    tb = merge_tables(pre, merge, post)
    N = cap_human + cap_rl
    veh = [idm_vehicle(noise=0.2, speed_mode=1, type=0) for _ in range(cap_human)] + \
          [idm_vehicle(controller=S.CTRL_RL, rl_index=k, speed_mode=1, type=1) for k in range(cap_rl)]
    rng = np.random.default_rng(seed)
    alive = np.zeros((R, N), dtype=bool)
    alive[:, :n_init] = True
    s0 = tb["routes"][0]["start"]
    # initial humans spread over the highway edges, slot 0 furthest downstream (placement is host work)
    base = s0 + 100.1 + pre - 30.0 - 40.0 * np.arange(n_init)
    X = np.zeros((R, N))
    X[:, :n_init] = base[None, :] + rng.uniform(0, 5.0, (R, n_init))
    spec = dict(num_replicas=R, num_vehicles=N, num_rl=num_rl, sim_step=0.2, max_speed=30.0,
                env=O.ENV_MERGE_PO if env is None else env, target_velocity=20.0, action_low=-1.5, action_high=1.5,
                horizon=horizon, warmup_steps=0, sims_per_step=1, vehicles=veh, seed=seed,
                junction=dict(enabled=1, lookahead=merge, time_gap=time_gap), junction_mode=1,
                inflows=[dict(type=0, route=0, period=3600.0 / q_highway, begin=1.0, end=86400.0, number=-1,
                              depart_speed=10.0, depart_pos=5.0),
                         dict(type=1, route=0, period=3600.0 / q_rl, begin=1.0, end=86400.0, number=-1,
                              depart_speed=10.0, depart_pos=5.0),
                         dict(type=0, route=1, period=3600.0 / q_merge, begin=1.0, end=86400.0, number=-1,
                              depart_speed=7.5, depart_pos=5.0)],
                init_alive=alive, init_pos=X, init_vel=np.zeros((R, N)), init_route=np.zeros((R, N), dtype=np.int32),
                network="merge", **tb)
    spec.update(kw)
    return spec


def merge_layout(spec, layout):
    """A constructed initial state of the merge network: ``layout`` = {slot: (x, speed, route)} on the routes' common
    coordinate (spec['merge_x'], spec['end_x']), the same in every replica.  Returns the init_alive / init_pos /
    init_vel / init_route entries of a spec (merge_spec takes them through **kw; dict.update on a built spec too)."""
    R, N = int(spec["num_replicas"]), int(spec["num_vehicles"])
    alive = np.zeros((R, N), dtype=bool)
    X, V = np.zeros((R, N)), np.zeros((R, N))
    route = np.zeros((R, N), dtype=np.int32)
    for slot, (x, speed, rt) in layout.items():
        assert 0 <= slot < N and not alive[0, slot]
        alive[:, slot], X[:, slot], V[:, slot], route[:, slot] = True, x, speed, rt
    return dict(init_alive=alive, init_pos=X, init_vel=V, init_route=route)


def quiet_spec(spec):
    """The same spec with the acceleration noise switched off (bit-exact comparisons)."""
    spec = dict(spec)
    spec["vehicles"] = [dict(v, noise=0.0) for v in spec["vehicles"]]
    return spec


def nan_actions(R, A, seed, p_nan=0.2):
    """k -> [R, A] actions (call in step order), NaN with probability p_nan: "the vehicle just entered", no action."""
    rng = np.random.default_rng(seed)

    def acts(k):
        a = rng.uniform(-1.0, 1.5, (R, A)).astype(np.float32)
        a[rng.random((R, A)) < p_nan] = np.nan
        return a
    return acts


def action_tape(action_fn, K):
    """[K, R, A]: the actions of steps 0 .. K - 1."""
    return np.stack([action_fn(k) for k in range(K)])


# ------------------------------------------------------------------ constructed edge states of the merge network
# (tests/test_queue_model.py proves the queue formulation on them on the CPU, tests/test_queue_edges_gpu.py runs them on
# k_merge_queue), the event counters of an oracle run and the floors the tests assert on them
class SubSteps:
    """Per sub-step event counts of an oracle run, [sub-step, R]: vehicles alive when the sub-step starts, arrivals,
    insertions and (QueueMergeOracle) joins and re-sorts.  SubSteps(ora) hooks the oracle's _substep."""

    def __init__(self, ora):
        self.ora, self.alive0, self.arrived, self.departed, self.joins, self.resorts = ora, [], [], [], [], []
        inner = ora._substep

        def substep(actions, active):
            n0, rs0 = ora.alive.sum(axis=1), getattr(ora, "resorts", 0)
            crash = inner(actions, active)
            self.alive0.append(np.where(active, n0, 0))
            self.arrived.append(np.where(active, ora.num_arrived, 0))
            self.departed.append(np.where(active, ora.num_departed, 0))
            self.joins.append(np.where(active, getattr(ora, "joins_now", np.zeros(ora.R, dtype=np.int64)), 0))
            self.resorts.append(getattr(ora, "resorts", 0) - rs0)
            return crash
        ora._substep = substep

    def table(self):
        """[sub-step, R] arrays: (alive at the start, arrivals, insertions, joins)."""
        return tuple(np.array(a).reshape(-1, self.ora.R) for a in (self.alive0, self.arrived, self.departed, self.joins))

    def full_wave_figures(self, full):
        """(sub-steps that start with `full` vehicles, joins from there, arrivals from there) -- the least of any replica."""
        alive0, arrived, _, joins = self.table()
        at = alive0 == full
        return int(at.sum(axis=0).min()), int((joins * at).sum(axis=0).min()), int((arrived * at).sum(axis=0).min())


def full_wave_spec(R=2, env=ENV_MERGE_MA, spacing=7.0, ramp_head=8.0, hole=0.0, **kw):
    """All 64 slots of a 64-lane wave alive from the start: 40 vehicles on the highway, the first 8 m before the end of
    the network, and 24 on the ramp, the first `ramp_head` m before the merge point, `spacing` m apart at 5 m/s, slots shuffled
    (36 humans + 4 RL vehicles on the highway, 22 + 2 on the ramp); busy inflows keep the pool full."""
    kw.setdefault("horizon", 1000)
    spec = quiet_spec(merge_spec(R=R, cap_human=58, cap_rl=6, num_rl=6, q_highway=2400.0, q_merge=900.0, sim_step=0.2, env=env, **kw))
    rng = np.random.default_rng(64)
    humans, rls = rng.permutation(58), 58 + rng.permutation(6)
    on0 = rng.permutation(np.concatenate([humans[:36], rls[:4]]))
    on1 = rng.permutation(np.concatenate([humans[36:], rls[4:]]))
    at0 = spec["end_x"] - 8.0 - spacing * np.arange(40)
    at0 = np.where(at0 < spec["merge_x"], at0 - hole, at0)     # `hole` m of free highway before the merge point
    lay = {int(s): (float(at0[i]), 5.0, 0) for i, s in enumerate(on0)}
    lay.update({int(s): (spec["merge_x"] - ramp_head - spacing * i, 5.0, 1) for i, s in enumerate(on1)})
    assert len(lay) == 64
    spec.update(merge_layout(spec, lay))
    return spec


def two_spec(R=2, rl_arrives=False, **kw):
    """sim_step 2 s: the two highway vehicles pass the end of the network and the two ramp vehicles the merge point in
    the FIRST sub-step, and (begin = 1 s <= now = 2 s) the inflows insert.  rl_arrives: the first vehicle is an RL one."""
    kw.setdefault("horizon", 1000)
    spec = quiet_spec(merge_spec(R=R, cap_human=20, cap_rl=2, sim_step=2.0, **kw))
    e, m = spec["end_x"], spec["merge_x"]
    spec.update(merge_layout(spec, {(20 if rl_arrives else 0): (e - 5.0, 20.0, 0), 1: (e - 32.0, 20.0, 0),
                                    2: (m - 3.0, 15.0, 1), 3: (m - 28.0, 15.0, 1)}))
    return spec


def join_tie_spec(ramp_slot, highway_slot, R=2, **kw):
    """A highway and a ramp vehicle 12 m before the merge point at 10 m/s, no right of way: they pass it side by side, at
    bit-equal x, and the join orders them by slot."""
    kw.setdefault("horizon", 1000)
    spec = quiet_spec(merge_spec(R=R, cap_human=10, cap_rl=2, sim_step=0.5, **kw))
    spec["junction"] = dict(spec["junction"], enabled=0)
    m = spec["merge_x"]
    spec.update(merge_layout(spec, {highway_slot: (m - 12.0, 10.0, 0), ramp_slot: (m - 12.0, 10.0, 1)}))
    return spec


def through_spec(R=2, **kw):
    """sim_step 2 s, 50 m from the merge point to the end: the ramp vehicle (slot 0, 28 m/s, 4 m before the merge point)
    passes the merge point AND the end of the network in the first sub-step -- it joins and arrives at once."""
    kw.setdefault("horizon", 1000)
    spec = quiet_spec(merge_spec(R=R, cap_rl=4, num_rl=4, sim_step=2.0, post=50.0, **kw))
    spec["junction"] = dict(spec["junction"], enabled=0)
    m = spec["merge_x"]
    spec.update(merge_layout(spec, {0: (m - 4.0, 28.0, 1), 1: (m - 40.0, 20.0, 0)}))
    return spec


def tail_tie_spec(moving_slot, resting_slot, R=2, route=0, speeds=(4.0, 0.0), **kw):
    """An insertion checked against a tail of TWO vehicles at one position (M3; oracle/opennet.py takes the lowest slot):
    RL vehicles with action 0 and no speed-mode clamp keep their speed exactly, so the one at rest at X and the one 2 m
    behind it at 4 m/s (sim_step 0.5) are both at X after the first sub-step.  The inflow on that route (begin 0: due in
    that sub-step) finds a gap of 24 m: the SUMO-IDM desired gap is 27.1 m behind the vehicle at rest and 21.3 m behind
    the moving one, so WHICH of the two is the tail decides whether the vehicle enters.  speeds = (0, 0): the plain case of two vehicles
    at rest at equal init_pos (nothing enters)."""
    kw.setdefault("horizon", 1000)
    spec = quiet_spec(merge_spec(R=R, cap_human=6, cap_rl=4, num_rl=4, sim_step=0.5, env=ENV_MERGE_MA, ma_apply_actions=True, **kw))
    spec["vehicles"] = [dict(v, speed_mode=0) if v["rl_index"] >= 0 else v for v in spec["vehicles"]]
    x_dep = spec["routes"][route]["start"] + 5.0
    X = x_dep + 5.0 + 24.0
    spec.update(merge_layout(spec, {moving_slot: (X - speeds[0] * 0.5, speeds[0], route), resting_slot: (X, speeds[1], route)}))
    spec["inflows"] = [dict(spec["inflows"][0], route=route, begin=0.0, period=50.0)]
    return spec


def resort_tie_spec(R=2, **kw):
    """Three vehicles at ONE position after the first sub-step, reached from behind: RL vehicles with action 0 and no
    speed-mode clamp (they keep their speed exactly) 0, 2 and 4 m behind X at 0, 4 and 8 m/s, in a slot order that is
    not the queue order -- the re-sort ranks three equal positions by slot."""
    kw.setdefault("horizon", 1000)
    spec = quiet_spec(merge_spec(R=R, cap_human=6, cap_rl=4, num_rl=4, sim_step=0.5, env=ENV_MERGE_MA, ma_apply_actions=True, **kw))
    spec["vehicles"] = [dict(v, speed_mode=0) if v["rl_index"] >= 0 else v for v in spec["vehicles"]]
    X = spec["routes"][0]["start"] + 150.0
    spec.update(merge_layout(spec, {8: (X, 0.0, 0), 6: (X - 2.0, 4.0, 0), 7: (X - 4.0, 8.0, 0), 0: (X - 40.0, 0.0, 0)}))
    return spec


def schedule_spec(which, R=2, **kw):
    """Inflow schedules at their edges (M2), sim_step 0.2 s, a pool of 10 + 3 slots that runs full, empty at reset.
    'always_due': RL vehicles on the highway, begin 0, period 3 sim_step, number = 3 (first in InFlows order: they take the
    first three gaps); humans on the highway, begin 0, period = sim_step (a vehicle is due every sub-step: one always
    waits); humans on the ramp, begin 0, period = 3 sim_step.
    'window': humans on the ramp, begin 1, period 0.2, end = 20 s (~95 vehicles are due by then and wait for a gap or a slot
    long after); two humans on the highway from begin = 3 * (3 * 0.2) = 1.8000000000000003 > 9 * 0.2 in float64: the first
    is due at sub-step index 10, not 9, and the entrance is free then; the default highway inflow from 4 s; RL vehicles on
    the highway due at 2, 6 and 10 s, end = 11 s: the fourth (14 s) is beyond the end -- the inflow closes after three."""
    kw.setdefault("horizon", 1000)
    spec = quiet_spec(merge_spec(R=R, cap_human=10, cap_rl=3, num_rl=3, sim_step=0.2, env=ENV_MERGE_MA, n_init=0, **kw))
    hw, rl, ramp = spec["inflows"]
    if which == "always_due":
        spec["inflows"] = [dict(rl, begin=0.0, period=3 * 0.2, number=3), dict(hw, begin=0.0, period=0.2),
                           dict(ramp, begin=0.0, period=3 * 0.2)]
    else:
        spec["inflows"] = [dict(ramp, begin=1.0, period=0.2, end=20.0), dict(hw, begin=3 * (3 * 0.2), period=3 * 0.2, number=2),
                           dict(hw, begin=4.0), dict(rl, begin=2.0, period=4.0, end=11.0)]
    return spec


def places32_spec(R=2, **kw):
    """MergePOEnv with a list of 32 places on 64 slots: 26 RL vehicles on the highway, the first 6 m before the end of
    the network, 6 on the ramp, 15 m apart, one human behind the highway's.  The list's order is the slots' order at
    reset: in replica 0 that is the driving order (the vehicle that leaves is at place 0), replica 1 holds the same
    vehicles in the RL slots REVERSED (it leaves from place 31, 30, ...), replica 2: see below."""
    kw.setdefault("horizon", 10 ** 6)
    spec = quiet_spec(merge_spec(R=R, cap_human=32, cap_rl=32, num_rl=32, pre=500.0, q_rl=1800.0, q_highway=600.0, sim_step=0.5,
                                 **kw))
    e, m = spec["end_x"], spec["merge_x"]
    lay = {32 + i: (e - 6.0 - 15.0 * i, 8.0, 0) for i in range(26)}
    lay.update({58 + i: (m - 40.0 - 15.0 * i, 5.0, 1) for i in range(6)})
    lay[0] = (e - 6.0 - 15.0 * 26, 8.0, 0)
    spec.update(merge_layout(spec, lay))
    if R > 1:
        perm = np.arange(64)
        perm[32:] = perm[32:][::-1]
        for key in ("init_alive", "init_pos", "init_vel", "init_route"):
            spec[key][1, perm] = spec[key][1].copy()
    if R > 2:
        # replica 2: 18 + 6 RL vehicles in the HIGH RL slots 40 .. 63, 100 m further back (nobody leaves for 30 s): the RL
        # inflow fills slots 32 .. 39 and places 24 .. 31.  reset() keeps rl_veh (merge.py:223-231): a reset then leaves
        # those eight as a run of departed entries at places 24 .. 31, which the removal loop takes in four passes
        for key in ("init_alive", "init_pos", "init_vel", "init_route"):
            spec[key][2] = 0
        late = {40 + i: (e - 106.0 - 15.0 * i, 8.0, 0) for i in range(18)}
        late.update({58 + i: (m - 40.0 - 15.0 * i, 5.0, 1) for i in range(6)})
        for slot, (x, v, rt) in late.items():
            for key, val in (("init_alive", True), ("init_pos", x), ("init_vel", v), ("init_route", rt)):
                spec[key][2, slot] = val
    return spec


class ReferenceLists:
    """MergePOEnv.additional_command (merge.py:189-221) with its own Python list operations, driven by the vehicles the
    oracle has in the network at every call (tests/test_open_cpu.py holds the oracle to them at four places): the oracle's
    rl_veh must be that list at every sub-step.  Counts what the run reached: `most_listed`, and `skipped_at` = the
    places of the entries the removal loop skipped (it removes from the list it iterates)."""

    def __init__(self, ora):
        import collections
        self.ora, self.most_listed, self.skipped_at = ora, 0, []
        self.queues = [collections.deque() for _ in range(ora.R)]
        self.lists = [[] for _ in range(ora.R)]
        inner = ora._additional_command

        def hooked(active):
            for r in range(ora.R):
                if active[r]:
                    self.reference(r)
            inner(active)
            for r in range(ora.R):
                if active[r]:
                    ids = self.vehicle_ids(r)
                    got = [self.name(r, i) if ora.alive[r, i] and ora.is_rl[i] else None
                           for i in sorted(np.flatnonzero(ora.ctl_seq[r] >= 0), key=lambda i: ora.ctl_seq[r, i])]
                    assert got == [v if v in ids else None for v in self.lists[r]], (r, got, self.lists[r])
                    self.most_listed = max(self.most_listed, sum(1 for v in self.lists[r] if v in ids))
        ora._additional_command = hooked

    def name(self, r, i):
        return (int(self.ora.episode[r]) if self.ora.origin[r, i] >= 0 else -1, int(self.ora.origin[r, i]))

    def vehicle_ids(self, r):
        ora = self.ora
        slots = sorted(np.flatnonzero(ora.alive[r] & ora.is_rl), key=lambda i: ora.seq[r, i])
        return [self.name(r, i) for i in slots]

    def reference(self, r):
        rl_ids, rl_queue, rl_veh = self.vehicle_ids(r), self.queues[r], self.lists[r]
        for veh_id in rl_ids:                                         # merge.py:201-203
            if veh_id not in list(rl_queue) + rl_veh:
                rl_queue.append(veh_id)
        for veh_id in list(rl_queue):                                 # :205-207
            if veh_id not in rl_ids:
                rl_queue.remove(veh_id)
        gone = [(p, v) for p, v in enumerate(rl_veh) if v not in rl_ids]
        for veh_id in rl_veh:                                         # :208-210 (iterates the list it shrinks)
            if veh_id not in rl_ids:
                rl_veh.remove(veh_id)
        self.skipped_at += [p for p, v in gone if v in rl_veh]
        while len(rl_queue) > 0 and len(rl_veh) < self.ora.num_rl:    # :213-215
            rl_veh.append(rl_queue.popleft())


# the floors of the full wave (measured on this layout, 400 steps, R = 2, the least of the replicas: MultiAgentMergePOEnv
# as shipped 232 sub-steps that start with 64 vehicles, 3 joins and 20 arrivals from there, 19 insertions; actions applied
# 263 / 3 / 20 / 19; MergePOEnv on the spaced layout 176 / 4 / 11 / 16, no collision; actions: nan_actions seeds 13 and 7)
FULL_WAVE_FLOORS = dict(full=100, joins=1, arrivals=10, departed=8)
FULL_WAVE_PO = dict(hole=40.0)          # MergePOEnv: 40 m of free highway before the merge point


def assert_full_wave(q, sub, floors=FULL_WAVE_FLOORS):
    full, joins, arrivals = sub.full_wave_figures(64)
    assert full >= floors["full"] and arrivals >= floors["arrivals"], (full, joins, arrivals)
    if hasattr(q, "joins"):
        assert joins >= floors["joins"], (full, joins, arrivals)
    assert q.total_departed.min() >= floors["departed"]
    return full, joins, arrivals


def assert_two_of_each(sub):
    alive0, arrived, departed, joins = sub.table()
    assert (alive0[0] == 4).all() and (arrived[0] == 2).all() and (departed[0] == 2).all()
    if hasattr(sub.ora, "joins"):
        assert (joins[0] == 2).all()


def tie_at_the_join(q, ramp_slot, highway_slot):
    """the sub-step of the (first) join: both vehicles are past the merge point at bit-equal x"""
    x = q.x[:, [ramp_slot, highway_slot]]
    return (x[:, 0] == x[:, 1]).all() and (x[:, 0] >= q.merge_x).all()


def assert_schedule(which, emitted):
    """emitted [step, R, flow] of 300 steps of schedule_spec(which), by the oracle."""
    if which == "always_due":
        assert (emitted[0, :, 0] == 1).all() and (emitted[0, :, 2] == 1).all()        # begin = 0: in at sub-step 0
        assert (emitted[-1, :, 0] == 3).all()                                          # emitted == number (at step 13)
        assert (emitted[-1, :, 1] >= 8).all() and (emitted[-1, :, 2] >= 3).all()        # (measured 16, 6)
    else:
        # the highway vehicle due at 1.8000000000000003 s enters at n = 10 (step 9), not at n = 9: 9 * 0.2 = 1.8 < due
        assert (emitted[8, :, 1] == 0).all() and (emitted[9, :, 1] == 1).all() and (emitted[-1, :, 1] == 2).all()
        # now = (k + 1) * 0.2 > end = 20 s from step 100 on: the vehicles that were due by then still enter
        assert (emitted[-1, :, 0] - emitted[100, :, 0] >= 5).all()                      # (measured 13: 5 by 20 s, 18 by 60 s)
        assert (emitted[-1, :, 0] < 96).all()
        # the inflow with end = 11 s closed itself: due at 2, 6, 10 s, the vehicle of 14 s never comes
        assert (emitted[-1, :, 3] == 3).all() and (emitted[150, :, 3] == 3).all()


def bottleneck_tables(junction_length=0.1, zipper_length=20.0, scaling=1):
    """BottleneckNetwork (flow/networks/bottleneck.py:111-165, scaling 1) on one coordinate: edges 1-5 of
    100 / 310 / 140 / 280 / 155 m with 4 / 4 / 4 / 2 / 1 lanes, short internal edges at nodes 2 and 3, zipper
    junctions of ``zipper_length`` at nodes 4 and 5.  Flow's edge-start table is ("1",0),("2",100),("3",405),
    ("4",425),("5",580) (:232-234); internal edges have no table entry (slope 0, value -1001 does not matter: the
    bottleneck envs only use edge-relative positions)."""
    j, z = junction_length, zipper_length
    e = [100.0, 310.0, 140.0, 280.0, 155.0]
    s1 = 0.0
    s2 = s1 + e[0] + j
    s3 = s2 + e[1] + j
    s4 = s3 + e[2] + z
    s5 = s4 + e[3] + z
    end = s5 + e[4]
    segs = [(s1, 0, 0.0, 1.0), (s1 + e[0], 1, -1001.0, 0.0), (s2, 0, 100.0, 1.0), (s2 + e[1], 1, -1001.0, 0.0),
            (s3, 0, 405.0, 1.0), (s3 + e[2], 1, -1001.0, 0.0), (s4, 0, 425.0, 1.0), (s4 + e[3], 1, -1001.0, 0.0),
            (s5, 0, 580.0, 1.0)]
    starts = dict(zip("12345", [s1, s2, s3, s4, s5]))
    lanes = dict(zip("12345", [4 * scaling, 4 * scaling, 4 * scaling, 2 * scaling, scaling]))
    lengths = dict(zip("12345", e))
    return dict(routes=[dict(start=0.0, segments=segs)], num_paths=4 * scaling, merge1_x=s4, merge2_x=s5, merge_x=s5,
                box_in=s5 - z, end_x=end, net_length=sum(e) + 2 * j + 2 * z + 1.0,   # + the 1 m rendering-only fake_edge
                edge_start=starts, edge_lanes=lanes, edge_length=lengths)


def segment_cells(tb, segments):
    """[(edge_start_x, lo, hi, lane, is_last_segment)] in the order the bottleneck envs walk them: edge, segment,
    lane (np.linspace(0, edge_length, n + 1) boundaries, bottleneck.py:796-812)."""
    cells = []
    for edge, n in segments:
        bounds = np.linspace(0, tb["edge_length"][edge], n + 1)
        for k in range(n):
            for lane in range(tb["edge_lanes"][edge]):
                cells.append((tb["edge_start"][edge], float(bounds[k]), float(bounds[k + 1]), lane, k == n - 1))
    return cells


def bottleneck_spec(R=4, cap_human=40, cap_rl=8, horizon=300, seed=0, q=2300.0, av_frac=0.1, env=None,
                    zipper_distance=50.0, warmup_steps=0, scaling=1, **kw):
    """singleagent_bottleneck.py: humans and RL vehicles all driven by the SUMO car-following model, inflow on
    edge 1 with departLane='random', BottleneckDesiredVelocityEnv head (141 observations, 20 actions)."""
    from oracle import opennet as O
    tb = bottleneck_tables(scaling=scaling)
    N = cap_human + cap_rl
    veh = [idm_vehicle(controller=S.CTRL_SIM, speed_mode=31, type=0) for _ in range(cap_human)] + \
          [idm_vehicle(controller=S.CTRL_RL, rl_index=k, speed_mode=9, type=1) for k in range(cap_rl)]
    rng = np.random.default_rng(seed)
    alive = np.zeros((R, N), dtype=bool)
    X = np.zeros((R, N))
    route = np.zeros((R, N), dtype=np.int32)
    # one human and one RL vehicle to start with, on edges 2.. (InitialConfig edges_distribution)
    alive[:, 0], X[:, 0], route[:, 0] = True, 300.0 + rng.uniform(0, 10, R), 1
    alive[:, cap_human], X[:, cap_human], route[:, cap_human] = True, 600.0 + rng.uniform(0, 10, R), 2
    obs_cells = segment_cells(tb, [("1", 1), ("2", 3), ("3", 3), ("4", 3), ("5", 1)])
    act_cells = segment_cells(tb, [("2", 2), ("3", 2), ("4", 2)])
    spec = dict(network="bottleneck", num_replicas=R, num_vehicles=N, num_rl=len(act_cells), sim_step=0.5, max_speed=23.0,
                env=O.ENV_BOTTLENECK_DV if env is None else env, target_velocity=40.0, action_low=-1.5, action_high=1.5,
                horizon=horizon, warmup_steps=warmup_steps, sims_per_step=1, vehicles=veh, seed=seed,
                junction=dict(enabled=0, lookahead=0.0, time_gap=1.0), junction_mode=1, speed_limit=23.0,
                zipper_distance=zipper_distance, scaling=scaling, obs_cells=obs_cells, action_cells=act_cells,
                obs_outflow_window=20, reward_outflow_window=10, track_followers=False,
                inflows=[dict(type=0, route=-1, period=3600.0 / (q * (1 - av_frac)), begin=1.0, end=86400.0, number=-1,
                              depart_speed=10.0, depart_pos=5.0),
                         dict(type=1, route=-1, period=3600.0 / (q * av_frac), begin=1.0, end=86400.0, number=-1,
                              depart_speed=10.0, depart_pos=5.0)],
                init_alive=alive, init_pos=X, init_vel=np.zeros((R, N)), init_route=route,
                **{k: v for k, v in tb.items() if k not in ("edge_start", "edge_lanes", "edge_length")})
    spec.update(kw)
    return spec


def bottleneck_layout(R, N, layout, end_x=None):
    """A constructed initial state of the lane-drop network: ``layout`` = {slot: (metres before end_x, speed, path)},
    the same in every replica.  Returns the init_alive / init_pos / init_vel / init_route entries of a spec
    (bottleneck_spec takes them through **kw)."""
    end_x = bottleneck_tables()["end_x"] if end_x is None else end_x
    alive = np.zeros((R, N), dtype=bool)
    X, V = np.zeros((R, N)), np.zeros((R, N))
    route = np.zeros((R, N), dtype=np.int32)
    for slot, (before_end, speed, path) in layout.items():
        alive[:, slot], X[:, slot], V[:, slot], route[:, slot] = True, end_x - before_end, speed, path
    return dict(init_alive=alive, init_pos=X, init_vel=V, init_route=route)


GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fig8_fixture_case():
    """tests/golden/fig8_emission.csv (the reference's tests/fast_tests/test_files/fig8_emission.csv, a SUMO
    emission file its visualizer tests read): 14 IDM vehicles on the one-lane figure eight, sim_step 1 s, four
    timestamps.  Returns (spec starting from the fixture's first timestamp, {time: {slot: (loop x, speed)}}, ids in
    slot order).  The experiment of that file is examples/exp_configs/non_rl/figure_eight.py:15-27 (IDMController
    defaults, speed_mode obey_safe_speed, decel 1.5) of a Flow version that still commanded vehicles on
    junction-internal edges (junction_mode 0: idm_8 gains 0.99 m/s inside ':center_0' at t = 4, Flow's IDM, not SUMO's
    2.6 m/s^2)."""
    import csv
    segs, junction, total, starts, _ = figure_eight_tables(30.0, 1, 0.1, 9.4)
    data = {}
    with open(os.path.join(GOLDEN_DIR, "fig8_emission.csv")) as f:
        for r in csv.DictReader(f):
            data.setdefault(int(r["id"].split("_")[1]), {})[float(r["time"])] = (
                starts[r["edge_id"]] + float(r["relative_position"]), float(r["speed"]))
    N = 14
    x0 = np.array([data[i][1.0][0] for i in range(N)])
    assert (np.diff(x0) > 0).all()                       # ids are in driving order already
    veh = [idm_vehicle(speed_mode=1, max_decel=1.5) for _ in range(N)]
    spec = dict(num_replicas=1, num_vehicles=N, num_rl=0, sim_step=1.0, junction_length=0.1,
                ring_length=np.full(1, total - 0.4), max_speed=30.0, env=S.ENV_ACCEL, target_velocity=20.0,
                action_low=-3.0, action_high=3.0, horizon=100, warmup_steps=0, sims_per_step=1, vehicles=veh,
                init_pos=x0[None, :], junction_mode=0, segments=segs, junction=junction)
    expected = {t: {i: data[i][t] for i in range(N)} for t in (2.0, 3.0, 4.0)}
    return spec, expected


# what the crossing model S-J (docs/HISTORY.md section 2) does NOT reproduce of that file: idm_8 starts 0.56 m before the
# crossing on the minor stream while idm_1's tail still covers the crossing point; SUMO lets it creep in behind the
# leaving vehicle (0.84 / 1.76 / 2.75 m/s), S-J holds it until the tail has left the box; idm_7 behind it feels that
# from the third step on
FIG8_FIXTURE_DEVIATIONS = {(8, 2.0), (8, 3.0), (8, 4.0), (7, 4.0)}


# ------------------------------------------------------------------ constructed edge layouts of the figure-eight step
# (k_rollout_loop, flowsim_fig8.h, and loop_policy_body, flowsim_policy.h; tests/test_loop_edges_cpu.py proves on the oracle
# that every layout reaches the event it is named for, tests/test_loop_edges_gpu.py runs them on the kernels).  Everything
# is dyadic: sim_step 1/8, slowdown_ramp 1, loop lengths and table entries on multiples of 1/8.  Three kinds of vehicle
# move EXACTLY, in float32 and float64 alike:
#   * an RL vehicle with speed_mode 0 and a dyadic action keeps a dyadic speed (action 0: x advances by v / 8 per step);
#   * a `parked` IDM vehicle (s0 = minGap = 512 m > every headway of these loops) has a negative acceleration whatever its
#     leader does and stays at v = 0, noise 0.2 included (a - 3 + 0.2 g < 0 for |g| < 15);
#   * a `waiting` IDM vehicle (default parameters, v = 0, obey_safe_speed) stays where it is while the crossing holds it --
#     the stop speed towards a line less than 2 m ahead is 0 -- and accelerates as soon as it is released.
LOOP_DT = 0.125
LOOP_CRASH_GAP = 0.5


def rl_mover(rl_index=0, speed_mode=0):
    return idm_vehicle(controller=S.CTRL_RL, rl_index=rl_index, speed_mode=speed_mode)


def parked(noise=0.0, delta=4):
    return idm_vehicle(p=[30, 1, 1, 1.5, delta, 512, 0, 0], sumo_min_gap=512.0, noise=noise, speed_mode=1)


def waiting(noise=0.0, delta=4):
    return idm_vehicle(p=[30, 1, 1, 1.5, delta, 2, 0, 0], noise=noise, speed_mode=1)


def ulps(x, n, dtype=np.float32):
    """x as `dtype`, moved n representable numbers up (n < 0: down)."""
    T = np.dtype(dtype).type
    x = T(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, T(np.inf) if n > 0 else T(-np.inf))
    return x


def start_for(target, v, steps, dtype=np.float32):
    """init_pos from which `steps` steps of x <- x + v / 8 (rounded to `dtype` each time, as the step does) end EXACTLY on
    `target` (itself a `dtype` number, possibly one ulp off a table entry)."""
    T = np.dtype(dtype).type
    target, inc = T(target), T(v) * T(LOOP_DT)
    x0 = T(np.float64(target) - steps * np.float64(inc))
    for _ in range(16):
        x = x0
        for _ in range(steps):
            x = T(x + inc)
        if x == target:
            return x0
        x0 = np.nextafter(x0, T(np.inf) if x < target else T(-np.inf))
    raise AssertionError("no %s start reaches %r in %d steps" % (np.dtype(dtype).name, target, steps))


def loop_edge_spec(L, segs, junction, vehicles, X, V, **kw):
    """The spec of a constructed loop: X, V [R, N] initial positions and speeds."""
    X, V = np.asarray(X, dtype=np.float64), np.asarray(V, dtype=np.float64)
    R, N = X.shape
    assert V.shape == X.shape and len(vehicles) == N and (X >= 0).all() and (X < L).all()
    spec = dict(num_replicas=R, num_vehicles=N, num_rl=sum(v["controller"] == S.CTRL_RL for v in vehicles),
                sim_step=LOOP_DT, slowdown_ramp=1.0, junction_length=0.0, ring_length=np.full(R, float(L)), max_speed=32.0,
                env=S.ENV_ACCEL, target_velocity=8.0, action_low=-1.0, action_high=1.0, horizon=10 ** 6, warmup_steps=0,
                sims_per_step=1, vehicles=vehicles, init_pos=X, init_vel=V, junction_mode=1, segments=segs,
                junction=junction, crash_gap=LOOP_CRASH_GAP, seed=12345, noise_math="exact", track_aux=False)
    spec.update(kw)
    return spec


def with_form(spec, form):
    """-> (spec, environment, last_kernel) of one of the four forms the figure-eight rollout step exists in.  'full' wants a
    noisy IDM slot in the spec; 'delta2' gives the first IDM slot the exponent 2 (pow_delta's x * x: still exact)."""
    if form == "full":
        return spec, {}, "k_rollout_loop<FULL>"
    if form == "flags":
        return spec, {"FLOWSIM_NO_LOOP_FULL": "1"}, "k_rollout_loop"
    if form == "k_steps":
        return spec, {"FLOWSIM_NO_LOOP_KERNEL": "1"}, "k_steps"
    assert form == "delta2"
    veh, first = [], True
    for v in spec["vehicles"]:
        if v["controller"] == S.CTRL_IDM and first:
            v, first = dict(v, p=list(v["p"][:4]) + [2] + list(v["p"][5:])), False
        veh.append(v)
    assert not first
    return dict(spec, vehicles=veh), {}, "k_rollout_loop"


LOOP_FORMS = ("full", "flags", "delta2", "k_steps")


# ---- case 1: the segment cursor
def cursor_table(L=64.0, full16=True):
    """Starts in clusters 1/8 m apart: three right after 0, four mid-loop, three right before L and (full16: 16 rows =
    FS_MAX_SEGMENTS) three at L / 4 and 3 L / 4.  Every row has its own flow_start; odd rows are internal (slope 0)."""
    starts = [0.0, 0.125, 0.25]
    if full16:
        starts += [L / 4, L / 4 + 0.125, L / 4 + 0.25]
    starts += [L / 2, L / 2 + 0.125, L / 2 + 0.25, L / 2 + 0.375]
    if full16:
        starts += [3 * L / 4, 3 * L / 4 + 0.125, 3 * L / 4 + 0.25]
    starts += [L - 0.375, L - 0.25, L - 0.125]
    assert len(starts) == (16 if full16 else 10)
    return [(st, k % 2, 1000.0 + 64.0 * k, 0.0 if k % 2 else 1.0) for k, st in enumerate(starts)]


def cursor_junction(L=64.0):
    """A small crossing off the clusters (the FULL form needs one): lines at 5 L / 16 and 7 L / 8 - 3 (no multiple of the
    16 m, or the 32 m, between the vehicles of these layouts apart: no two of them in the two conflict zones at once)."""
    a, b = 5 * L / 16, 7 * L / 8 - 3
    return dict(a_in=a, a_out=a + 1, b_in=b, b_out=b + 1, lookahead=0.0, time_gap=0.125,      # (nobody is ever held)
                za_lo=a + 0.25, za_hi=a + 0.5, zb_lo=b + 0.25, zb_hi=b + 0.5)


# (speed, fraction of a metre) of a replica's vehicles, which start an integer number of metres before the clusters; at
# v = 8 a step is 1 m, at v = 4 half a metre.  With C a cluster's first start (the mid-loop one has four starts):
#   .25 @ 8: C - .75 -> C + .25 passes 3 starts and lands on the third; L - .75 -> .25 passes the last three, wraps, passes 2
#   .375 @ 8: -> C + .375 passes 4 mid-loop and lands on the fourth      .5 @ 8: -> C + .5 passes 4
#   .125 @ 8 and @ 4: -> .125 wraps and passes 1                          0 @ 4: L - .5 -> 0.0 lands on L = 0
#   .25 @ 4: C - .25 -> C + .25 passes 3; L - .25 -> .25 passes the last start, wraps, passes 2
#   .375 @ 4: C - .125 -> C + .375 passes 4; L - .625 -> L - .125 passes 3 and lands on the last start
CURSOR_REPLICAS = ((8.0, 0.25), (8.0, 0.375), (8.0, 0.125), (8.0, 0.5), (4.0, 0.0), (4.0, 0.25), (4.0, 0.375), (4.0, 0.125))
CURSOR_N = 12


def cursor_spec(full16=True, replicas=CURSOR_REPLICAS, one_rl=False, lead=8.0, **kw):
    """12 vehicles 16 m apart all round a loop of 192 m (the rollout kernels take rows of 9 to 16), all at the replica's
    speed, vehicle 0 `lead` m (one value, or one per replica) minus the replica's fraction before the mid-loop cluster --
    and so vehicles 3, 6 and 9 before the clusters at 3 L / 4, L and L / 4.  RL vehicles (they keep their speed exactly)
    but for slot 10, a noisy IDM vehicle: the one whose commands the internal rows switch off.  one_rl (the policy
    kernels take ONE RL vehicle): slot 11 is the RL vehicle, the others are IDM vehicles."""
    N, L = CURSOR_N, 16.0 * CURSOR_N
    veh, n_rl = [], 0
    for i in range(N):
        if i == N - 2 or (one_rl and i != N - 1):
            veh.append(waiting(noise=0.2 if i == N - 2 else 0.0))
        else:
            veh.append(rl_mover(n_rl))
            n_rl += 1
    lead = np.broadcast_to(np.asarray(lead, dtype=np.float64), (len(replicas),))
    X = np.array([[(L / 2 - d + f + 16.0 * i) % L for i in range(N)] for d, (_, f) in zip(lead, replicas)])
    V = np.array([[v] * N for v, _ in replicas])
    return loop_edge_spec(L, cursor_table(L, full16), cursor_junction(L), veh, X, V, **kw)


class LoopLog:
    """What an oracle run reached, per sub-step (hooks RingOracle._substep and _yield_speed_cap): positions before and
    after, the vehicles the crossing held (a finite yield speed), the collisions."""

    def __init__(self, ora):
        self.ora, self.x0, self.x1, self.v0, self.v1, self.held, self.crash = ora, [], [], [], [], [], []
        step, cap = ora._substep, ora._yield_speed_cap

        def capped(v):
            c = cap(v)
            self.held.append(c < ora.dt_.type(1.0e38))
            return c

        def substep(actions, active):
            self.x0.append(ora.x.copy())
            self.v0.append(ora.v.copy())
            crash = step(actions, active)
            self.x1.append(ora.x.copy())
            self.v1.append(ora.v.copy())
            self.crash.append(crash.copy())
            return crash
        ora._substep, ora._yield_speed_cap = substep, capped

    def arrays(self):
        return tuple(np.array(a) for a in (self.x0, self.x1, self.v0, self.held))     # each [K, R, N]

    def cursor_events(self):
        """{event: count [R]} over the run."""
        x0, x1, _, _ = self.arrays()
        starts = np.array([s[0] for s in self.ora.segments], dtype=self.ora.dt_)
        k0 = (x0[..., None] >= starts).sum(axis=-1) - 1
        k1 = (x1[..., None] >= starts).sum(axis=-1) - 1
        wrapped = x1 < x0
        last = len(starts) - 1
        ev = dict(pass3=~wrapped & (k1 - k0 == 3), pass4=~wrapped & (k1 - k0 == 4), wrap1=wrapped & (k1 == 1),
                  wrap2=wrapped & (k1 == 2), last_wrap=wrapped & (k0 < last),
                  exact=(x1 != x0) & (x1[..., None] == starts).any(axis=-1), changed=(k1 != k0))
        return {name: m.sum(axis=(0, 2)) for name, m in ev.items()}


    def changed_rows(self):
        """[K, R]: some vehicle of the replica is on another segment after the step."""
        x0, x1, _, _ = self.arrays()
        starts = np.array([s[0] for s in self.ora.segments], dtype=self.ora.dt_)
        return ((x0[..., None] >= starts).sum(axis=-1) != (x1[..., None] >= starts).sum(axis=-1)).any(axis=2)


CURSOR_EVENTS = ("pass3", "pass4", "wrap1", "wrap2", "last_wrap", "exact")
POLICY_HORIZON = 3


def policy_cursor_spec(**kw):
    """The cursor layout for the fused policy kernels: ONE RL vehicle, episodes of 3 steps, everybody at 8 m/s.  Vehicles
    0, 3, 6 and 9 start 3, 2 or 1 m (the replica number modulo 3) before a cluster: replicas 0, 3 and 6 pass the clusters
    and wrap in the LAST step of every episode, so the reset that follows finds the cursor advanced; the others carry it
    on for a step or two."""
    reps = tuple((8.0, f) for _, f in CURSOR_REPLICAS)
    return cursor_spec(one_rl=True, replicas=reps, lead=[3.0 - r % 3 for r in range(len(reps))], horizon=POLICY_HORIZON, **kw)


def assert_policy_cursor_events(log, dones):
    """dones [K, R] of the replayed fragment: episodes end on steps that change the segment, steps pass three starts and
    more, wrap and advance -- also in steps that do not end an episode."""
    ev, changed = log.cursor_events(), log.changed_rows()
    ends = int((dones & changed).sum())
    inside = int((~dones & changed).sum())
    assert ends >= 3 and inside >= 3 and ev["pass3"].sum() + ev["pass4"].sum() >= 3 and \
        ev["wrap1"].sum() + ev["wrap2"].sum() >= 3, (ends, inside, ev)


def assert_cursor_events(log, names=CURSOR_EVENTS, total=3, replicas=2):
    ev = log.cursor_events()
    for name in names:
        assert ev[name].sum() >= total and (ev[name] > 0).sum() >= replicas, (name, ev[name])
    return ev


# ---- case 2: ties at the crossing
TIE_L = 256.0
TIE_SEGS = [(0.0, 0, 0.0, 1.0), (128.0, 0, 128.0, 1.0)]
TIE_J = dict(a_in=32.0, a_out=40.0, b_in=160.0, b_out=168.0, lookahead=2.0, time_gap=2.0,
             za_lo=35.0, za_hi=42.0, zb_lo=163.0, zb_hi=170.0)
# name -> (kind, the boundary, closed: does x == boundary count as inside, where the other vehicle stands)
#   'approach': a waiting IDM vehicle (slot 1) ON the boundary of an approach window, the box held busy by the RL vehicle
#               at rest in the other stream (slot 0); inside: it is held for the whole run, outside: it drives off
#   'busy':     the RL vehicle (slot 0, 4 m/s) reaches the boundary of its stream's busy window at step `at`; a waiting IDM
#               vehicle 1 m before the other stream's line is held while the window is occupied
#   'zone':     the RL vehicle reaches the boundary of its conflict zone at step `at` with a parked vehicle inside the
#               other zone: a collision inside, none outside
TIES = {
    "jb_in-look": ("approach", 158.0, True, 36.0), "jb_in": ("approach", 160.0, False, 36.0),
    "ja_in-look": ("approach", 30.0, True, 164.0), "ja_in": ("approach", 32.0, False, 164.0),
    "ja_in-tgap*v": ("busy", 24.0, True, 159.0), "ja_out+len": ("busy", 45.0, False, 159.0),
    "jb_out+len": ("busy", 173.0, False, 31.0),
    "za_lo": ("zone", 35.0, True, 165.0), "za_hi": ("zone", 42.0, False, 165.0),
    "zb_lo": ("zone", 163.0, True, 37.0), "zb_hi": ("zone", 170.0, False, 37.0),
}
TIE_OFFSETS = (-1, 0, 1, -1, 0, 1)          # replica r stands TIE_OFFSETS[r] ulps off the boundary ...
TIE_AT = {"approach": (0, 0, 0, 0, 0, 0), "busy": (0, 0, 0, 5, 5, 5), "zone": (1, 1, 1, 5, 5, 5),
          "gap": (2, 2, 2, 5, 5, 5)}        # ... at this step (0: the first snapshot of a launch)
TIE_PROP = (220.0, 220.0, 220.0, 216.5, 216.5, 216.5)     # the parked noisy vehicle (the last slot): the replicas differ in it
TIE_PARKED = (180.0, 186.0, 192.0, 198.0, 204.0, 210.0)   # parked vehicles that fill the row (the rollout kernels take 9 to 16)


def padded(veh, X, V, last=None, extra=TIE_PARKED):
    """The vehicles, positions and speeds with parked vehicles at `extra` appended and then `last` = (vehicle, x [R], v)."""
    veh = list(veh) + [parked() for _ in extra]
    X = [list(x) + list(extra) for x in X]
    V = [list(v) + [0.0] * len(extra) for v in V]
    if last is not None:
        veh.append(last[0])
        X = [x + [xl] for x, xl in zip(X, last[1])]
        V = [v + [last[2]] for v in V]
    return veh, X, V


def tie_inside(name):
    """[R] does replica r count as inside (held / busy / colliding) at its step."""
    closed = TIES[name][2]
    return np.array([(o >= 0) if closed else (o < 0) for o in TIE_OFFSETS])


def tie_spec(name, dtype=np.float32, **kw):
    """dtype: the type the ulps are counted in (float32 kernels and their oracle twin; float64 for FS_MIXED)."""
    kind, bound, _, other = TIES[name]
    X, V = [], []
    for off, at, prop in zip(TIE_OFFSETS, TIE_AT[kind], TIE_PROP):
        edge = ulps(bound, off, dtype)
        if kind == "approach":
            X.append([other, edge])
            V.append([0.0, 0.0])
        else:
            X.append([start_for(edge, 4.0, at, dtype), other])
            V.append([4.0, 0.0])
    veh, X, V = padded([rl_mover(0), parked() if kind == "zone" else waiting()], X, V, (parked(noise=0.2), TIE_PROP, 0.0))
    return loop_edge_spec(TIE_L, TIE_SEGS, TIE_J, veh, X, V, **kw)


def gap_tie_spec(dtype=np.float32, **kw):
    """h == crash_gap: the RL vehicle (4 m/s) is 5.5 m behind the front of a parked vehicle of 5 m at its step: no collision
    on the boundary or an ulp before it, one an ulp past it -- and for everyone one step later."""
    X, V = [], []
    for off, at, prop in zip(TIE_OFFSETS, TIE_AT["gap"], TIE_PROP):
        X.append([start_for(ulps(94.5, off, dtype), 4.0, at, dtype), 100.0])
        V.append([4.0, 0.0])
    veh, X, V = padded([rl_mover(0), parked()], X, V, (parked(noise=0.2), TIE_PROP, 0.0))
    return loop_edge_spec(TIE_L, TIE_SEGS, TIE_J, veh, X, V, **kw)


def assert_tie(name, log, dones, K, dtype=None):
    """The oracle's side of a tie run of K steps (dones [K, R]; the horizon is out of reach: done = collision); dtype:
    the type the layout's ulps were counted in (the oracle's own unless given)."""
    x0, x1, v0, held = log.arrays()
    dtype = log.ora.dt_ if dtype is None else dtype
    kind = TIES[name][0] if name != "gap" else "gap"
    at = np.array(TIE_AT[kind])
    rows = np.arange(len(at))
    if kind == "gap":
        assert (x1[at - 1, rows, 0] == np.array([ulps(94.5, o, dtype) for o in TIE_OFFSETS])).all()
        np.testing.assert_array_equal(dones[at - 1, rows], np.array(TIE_OFFSETS) > 0)
        assert dones[at, rows].all() and not dones[:at.min() - 1].any()
        return
    inside = tie_inside(name)
    edge = np.array([ulps(TIES[name][1], o, dtype) for o in TIE_OFFSETS])
    if kind == "approach":                                   # held for the whole run / gone with the first step
        assert (x0[0, :, 1] == edge).all()
        np.testing.assert_array_equal(held[0, :, 1], inside)
        assert held[:, inside, 1].all() and (x1[-1, inside, 1] == edge[inside]).all()
        assert (x1[0, ~inside, 1] > edge[~inside]).all()
    elif kind == "busy":                                     # the snapshot of step `at` decides step `at`
        assert (x0[at, rows, 0] == edge).all()
        np.testing.assert_array_equal(held[at, rows, 1], inside)
    else:                                                    # the state AFTER step `at - 1` is the one judged
        assert (x1[at - 1, rows, 0] == edge).all()
        np.testing.assert_array_equal(dones[at - 1, rows], inside)
    assert K > at.max()


# ---- case 3: both lines within one look-ahead
def degenerate_spec(a_first=True, **kw):
    """ja_in and jb_in 4 m apart with a look-ahead of 16 m, ONE vehicle at rest (the RL vehicle, slot 0, at 46) inside both
    boxes: an IDM vehicle (slot 1, obey_safe_speed) drives up to the lines on both approaches at once and stops at the
    nearer one -- stream a's (a_first) or stream b's.  The stop speed grows with the gap, so the nearer line is the one
    that binds; the two tables are there so that each STREAM's line is that one once."""
    near, far = (40.0, 48.0), (44.0, 52.0)
    (a_in, a_out), (b_in, b_out) = (near, far) if a_first else (far, near)
    J = dict(a_in=a_in, a_out=a_out, b_in=b_in, b_out=b_out, lookahead=16.0, time_gap=2.0,
             za_lo=a_in + 5.0, za_hi=a_in + 5.5, zb_lo=b_in + 5.0, zb_hi=b_in + 5.5)
    X = [[46.0, 20.0], [46.0, 22.5], [46.0, 18.25], [46.0, 25.0]]
    V = [[0.0, 6.0], [0.0, 4.0], [0.0, 8.0], [0.0, 5.0]]
    veh, X, V = padded([rl_mover(0), waiting()], X, V, (parked(noise=0.2), TIE_PROP[1:5], 0.0))
    return loop_edge_spec(TIE_L, TIE_SEGS, J, veh, X, V, **kw)


def degenerate_winners(log):
    """(steps in which stream a's stop speed is the smaller of the two, steps in which stream b's is, replicas with a
    vehicle on both approaches and both boxes blocked) -- restated from the oracle's snapshot with its own model function."""
    from oracle import controllers as C
    ora = log.ora
    x0, _, v0, held = log.arrays()
    T, J = ora.dt_.type, ora.junction
    x, v = x0[:, :, 1], v0[:, :, 1]
    both = held[:, :, 1] & (x >= T(J["a_in"]) - T(J["lookahead"])) & (x < T(J["a_in"])) & \
        (x >= T(J["b_in"]) - T(J["lookahead"])) & (x < T(J["b_in"]))
    vs = ora.veh[1]
    stop = [C.sumo_idm_speed(v, np.zeros_like(v), T(J[line]) - x, np.ones(v.shape, bool), ora.dt, accel=vs["max_accel"],
                             decel=vs["max_decel"], tau=vs["sumo_tau"], min_gap=vs["sumo_min_gap"],
                             max_speed=vs["sumo_max_speed"]) for line in ("a_in", "b_in")]
    return int((both & (stop[0] < stop[1])).sum()), int((both & (stop[1] < stop[0])).sum()), int(both.any(axis=0).sum())


# ---- case 4: the tail of a launch and the time limit
TAIL_K = 11
TAIL_FIRST_CRASH = (4, 5, 6, 7, 8, 9, 10, None)      # replica r: the step of its first collision (a launch of 11 steps:
                                                     # every slot of the second block of four, every slot of the tail)


def tail_spec(follower=True, horizon=10 ** 6, **kw):
    """The RL vehicle (slot 0, 4 m/s) runs into a parked one (slot 1, front at 100, 5 m long): the gap is below 0.5 m after
    step TAIL_FIRST_CRASH[r].  follower: a noisy IDM vehicle (the last slot) follows the RL vehicle -- visible noise;
    without it every vehicle moves exactly.  Parked vehicles fill the row."""
    X, V = [], []
    for r, c in enumerate(TAIL_FIRST_CRASH):
        X.append([20.0 if c is None else 94.75 - 0.5 * (c + 1), 100.0])
        V.append([4.0, 0.0])
    last = (waiting(noise=0.2), [(x[0] - 30.0 - 0.25 * r) % TIE_L for r, x in enumerate(X)], 4.0) if follower else None
    veh, X, V = padded([rl_mover(0), parked()], X, V, last, TIE_PARKED + (() if follower else (216.0,)))
    return loop_edge_spec(TIE_L, TIE_SEGS, TIE_J, veh, X, V, horizon=horizon, **kw)


def fragments_of(K, cycle):
    """K cut into launches of cycle[0], cycle[1], ... steps, cyclically."""
    out = []
    while sum(out) < K:
        out.append(min(cycle[len(out) % len(cycle)], K - sum(out)))
    return out


ODD_CYCLE = (1, 7, 3, 16, 5)           # (tests/test_queue_edges_gpu.py odd_fragments)
SHORT_CYCLE = (2, 3, 1, 4, 6)          # launches of 1, 2 and 3 steps; starts two steps into a block of four


def start_phases(fragments):
    """{launch start mod 4}: where in Philox's block of four draws the launches begin."""
    return {int(s) % 4 for s in np.cumsum([0] + list(fragments[:-1]))}


# ---- case 5: shapes
def shape_spec(N, R, env=None, rl_slots=None, **kw):
    """N vehicles 16 m apart on the cursor table of a loop of max(64, 16 N) m, 8 m/s (RL vehicles keep it exactly), the
    replicas 1/8 m apart; IDM vehicles (noisy) at slot N - 2 or wherever rl_slots leaves one."""
    L = float(max(64, 16 * N))
    rl_slots = [i for i in range(N) if i != N - 2] if rl_slots is None else list(rl_slots)
    veh = [rl_mover(rl_slots.index(i)) if i in rl_slots else waiting(noise=0.2) for i in range(N)]
    X = np.array([[(L / 2 - 8.75 + 0.125 * r + 16.0 * i) % L for i in range(N)] for r in range(R)])
    spec = loop_edge_spec(L, cursor_table(L, True), cursor_junction(L), veh, X, np.full((R, N), 8.0), **kw)
    if env is not None:
        spec["env"] = env
    return spec


def oracle_rows(spec, acts, K, dtype=np.float32, log=True):
    """K oracle steps -> (oracle, LoopLog, obs [K, R, D], rew [K, R], done [K, R] bool, limit [K, R] bool)."""
    ora = S.RingOracle(spec, dtype)
    lg = LoopLog(ora) if log else None
    ora.reset()
    o, r, d, lim = [], [], [], []
    for k in range(K):
        ok, rk, dk = ora.step(None if acts is None else acts[k])
        o.append(ok), r.append(rk), d.append(dk.copy()), lim.append(ora.time_counter >= spec["horizon"])
    return ora, lg, np.array(o), np.array(r), np.array(d), np.array(lim)


def zero_actions(spec, K):
    return np.zeros((K, spec["num_replicas"], max(spec["num_rl"], 1)), dtype=np.float32)
