"""CPU tests of the open-network row: the merge oracle (oracle/opennet.py) against hand-checkable facts,
the host mirror (MergeNetwork, InFlows, slot pools, MergePOEnv spec) and the C-ABI validation of open
configurations.  No GPU."""
import os

import numpy as np
import pytest

from helpers import idm_vehicle, merge_spec, merge_tables
from oracle import opennet as O
from oracle import refsim as S

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def quiet(spec):
    spec = dict(spec)
    spec["vehicles"] = [dict(v, noise=0.0) for v in spec["vehicles"]]
    return spec


# ------------------------------------------------------------------ oracle
def test_vehicle_count_is_conserved_and_nobody_overlaps():
    spec = quiet(merge_spec(R=4, cap_human=28, cap_rl=4, num_rl=2, horizon=600, seed=2))
    o = O.MergeOracle(spec, np.float64)
    o.reset()
    n0 = o.alive.sum(axis=1)
    rng = np.random.default_rng(0)
    for k in range(600):
        _, _, done = o.step(rng.uniform(0.3, 1.5, (4, 2)))
        assert not done.any() or k == 599                                  # no collision with right of way on
        np.testing.assert_array_equal(o.total_departed - o.total_arrived, o.alive.sum(axis=1) - n0)
        h = np.where(o.alive & (o.lead >= 0), o.h, 1.0)
        assert (h > 0).all()
        x = np.where(o.alive, o.x, o.merge_x)
        start = np.where(o.route == 1, spec["routes"][1]["start"], spec["routes"][0]["start"])
        assert (x >= start - 1e-9).all() and (x < o.end_x).all()
    assert o.total_arrived.min() > 10
    # ids: departure numbers are unique among the vehicles in the network
    for r in range(4):
        seqs = o.seq[r][o.alive[r]]
        assert len(set(seqs.tolist())) == len(seqs)


def test_inflow_schedule_on_an_empty_road():
    """M2: the k-th vehicle of a flow is due at begin + k * period; it appears after the first step whose start
    time n * dt is >= that (n counts integration steps, the reset's own step included)."""
    spec = quiet(merge_spec(R=1, cap_human=20, cap_rl=2, num_rl=1, n_init=0, q_highway=360.0, q_rl=1e-3,
                            q_merge=1e-3, horizon=1000))
    o = O.MergeOracle(spec, np.float64)
    o.reset()
    seen = []
    for n in range(1, 400):                     # env step n runs integration step n (start time n * 0.2)
        o.step(None)
        seen.append(int(o.total_departed[0]))
    period, dt = 10.0, 0.2
    for n in range(1, 400):
        due = int(np.floor((n * dt - 1.0) / period + 1e-9)) + 1 if n >= 5 else 0
        # the two 1e-3 veh/h flows emit their first vehicle at t = 1 too: the on-ramp one at once (step 5), the
        # highway one after the first human has cleared the SUMO-IDM desired gap 2.5 + 10 * 1 m (M3) -- step 13
        assert seen[n - 1] == due + (1 if n >= 5 else 0) + (1 if n >= 13 else 0), (n, seen[n - 1], due)


def test_insertion_waits_for_a_safe_gap_and_for_a_free_slot():
    spec = quiet(merge_spec(R=1, cap_human=3, cap_rl=1, num_rl=1, n_init=0, q_highway=3600.0, q_rl=1e-3,
                            q_merge=1e-3, horizon=1000))
    o = O.MergeOracle(spec, np.float64)
    o.reset()
    for _ in range(200):
        o.step(None)
        gaps = o.h[0][o.alive[0] & (o.lead[0] >= 0)]
        assert (gaps > 2.0).all()
    # 3 human slots: never more than 3 humans in the network although one is due every second
    assert o.alive[0, :3].sum() <= 3 and o.total_departed[0] < 200 * 0.2 + 2
    assert o.emitted[0, 0] == o.total_departed[0] - o.emitted[0, 1] - o.emitted[0, 2]


def test_rl_queue_is_first_in_first_out_and_the_ghost_row():
    spec = quiet(merge_spec(R=1, cap_human=10, cap_rl=4, num_rl=1, n_init=0, q_highway=600.0, q_rl=900.0,
                            q_merge=1e-3, horizon=2000, pre=60.0, post=60.0))
    o = O.MergeOracle(spec, np.float64)
    o.reset()
    controlled, ghosts = [], 0
    for k in range(900):
        obs, _, _ = o.step(np.full((1, 1), 0.8))
        ctl = np.flatnonzero(o.ctl_seq[0] >= 0)
        assert len(ctl) <= 1
        if len(ctl):
            i = int(ctl[0])
            key = int(o.origin[0, i]) if o.alive[0, i] else controlled[-1]
            if not controlled or controlled[-1] != key:
                controlled.append(key)
            if not o.alive[0, i]:                                          # arrived this step: error values
                ghosts += 1
                np.testing.assert_allclose(obs[0], [-1001 / 30, (30 + 1001) / 30, 1.0, -1001 / 30, 1.0])
        else:
            np.testing.assert_array_equal(obs[0], np.zeros(5))             # unused places stay 0
    ks = [c & 0xFFFFF for c in controlled]
    assert len(ks) >= 3 and ks == sorted(ks) and ghosts >= 2               # served in order of entering


def test_actions_reach_the_vehicle_at_its_place_in_rl_veh():
    spec = quiet(merge_spec(R=1, cap_human=6, cap_rl=4, num_rl=2, n_init=0, q_highway=1e-3, q_rl=1200.0,
                            q_merge=1e-3, horizon=500))
    o = O.MergeOracle(spec, np.float64)
    o.reset()
    for k in range(60):
        o.step(np.array([[1.0, -1.0]]))
    rank = o._ctl_rank()[0]
    first, second = int(np.flatnonzero(rank == 0)[0]), int(np.flatnonzero(rank == 1)[0])
    assert o.seq[0, first] < o.seq[0, second]
    assert o.last_accel[0, first] == 1.0 and o.last_accel[0, second] == -1.0


def test_sticky_follower_rule():
    """vehicle/traci.py:243-250: 'follower_headway' is only ever lowered; a vehicle without a leader is reset."""
    tb = merge_tables()
    veh = [idm_vehicle(type=0) for _ in range(4)]
    base = dict(num_replicas=1, num_vehicles=4, num_rl=0, sim_step=0.2, max_speed=30.0, env=O.ENV_MERGE_MA,
                vehicles=veh, inflows=[], junction=dict(enabled=0, lookahead=100.0, time_gap=1.0),
                init_alive=np.ones((1, 4), bool), init_vel=np.zeros((1, 4)), init_route=np.zeros((1, 4), int),
                init_pos=np.array([[300.0, 280.0, 200.0, 100.0]]), target_velocity=10.0, action_low=-1, action_high=1, **tb)
    o = O.MergeOracle(base, np.float64)
    o.reset()
    np.testing.assert_array_equal(o.lead[0], [-1, 0, 1, 2])
    np.testing.assert_array_equal(o.foll[0], [1, 2, 3, -1])
    assert o.foll_h[0, 1] == 280.0 - 5 - 200.0
    # vehicle 2 falls back: its headway to 1 grows, the recorded minimum stays
    o.x[0, 2] = 150.0
    o._update_neighbours(np.ones(1, bool))
    assert o.foll[0, 1] == 2 and o.foll_h[0, 1] == 75.0 and o.h[0, 2] == 125.0
    # a merge-branch vehicle becomes another follower of 1 with a larger gap than the recorded one: not registered
    o.route[0, 3], o.x[0, 3] = 1, 190.0
    o._update_neighbours(np.ones(1, bool))
    assert o.lead[0, 3] == -1                       # vehicle 1 is still upstream of the merge point: not its leader
    o.x[0, 0], o.x[0, 1] = 400.0, 330.0             # 1 moves onto the shared edge: leader of both 2 and 3
    o._update_neighbours(np.ones(1, bool))
    assert o.lead[0, 2] == 1 and o.lead[0, 3] == 1 and o.foll[0, 1] == 2 and o.foll_h[0, 1] == 75.0
    # the front vehicle has no leader: its entry restarts from 1000 each update
    assert o.foll[0, 0] == 1 and o.foll_h[0, 0] == 400.0 - 5 - 330.0


def test_minor_route_yields_and_no_box_conflict():
    spec = quiet(merge_spec(R=2, cap_human=28, cap_rl=2, num_rl=1, q_highway=1700.0, q_rl=1e-3, q_merge=600.0,
                            horizon=700, seed=3))
    o = O.MergeOracle(spec, np.float64)
    o.reset()
    waited = False
    for k in range(700):
        _, _, done = o.step(None)
        inside = o.alive & (o.x >= o.box_in) & (o.x < o.merge_x)
        assert not ((inside & (o.route == 0)).any(axis=1) & (inside & (o.route == 1)).any(axis=1)).any()
        near = o.alive & (o.route == 1) & (o.x > o.box_in - 8.0) & (o.x < o.box_in) & (o.v < 0.2)
        waited |= bool(near.any())
        assert not done.any() or k == 699
    assert waited and (o.total_arrived > 30).all()


def test_float32_twin_tracks_float64_over_a_short_horizon():
    spec = quiet(merge_spec(R=2, cap_human=12, cap_rl=2, num_rl=1, horizon=100, seed=5))
    a, b = O.MergeOracle(spec, np.float32), O.MergeOracle(spec, np.float64)
    a.reset(), b.reset()
    for k in range(60):
        act = np.full((2, 1), 0.5)
        a.step(act), b.step(act)
    np.testing.assert_array_equal(a.route, b.route)
    np.testing.assert_allclose(a.x[a.alive], b.x[b.alive], atol=5e-3)


# ------------------------------------------------------------------ host mirror
def merge_network(pre=500, n_human=5, n_rl=0, flows=True):
    from flow_amd.controllers import IDMController, RLController
    from flow_amd.core import params as P
    from flow_amd.networks.merge import ADDITIONAL_NET_PARAMS, MergeNetwork
    add = ADDITIONAL_NET_PARAMS.copy()
    add["pre_merge_length"] = pre
    v = P.VehicleParams()
    v.add("human", acceleration_controller=(IDMController, {"noise": 0.2}),
          car_following_params=P.SumoCarFollowingParams(speed_mode="obey_safe_speed"), num_vehicles=n_human)
    v.add("rl", acceleration_controller=(RLController, {}),
          car_following_params=P.SumoCarFollowingParams(speed_mode="obey_safe_speed"), num_vehicles=n_rl)
    inflow = P.InFlows()
    if flows:
        inflow.add(veh_type="human", edge="inflow_highway", vehs_per_hour=1800, departLane="free", departSpeed=10)
        inflow.add(veh_type="rl", edge="inflow_highway", vehs_per_hour=200, departLane="free", departSpeed=10)
        inflow.add(veh_type="human", edge="inflow_merge", vehs_per_hour=100, departLane="free", departSpeed=7.5)
    return MergeNetwork("merge", v, P.NetParams(inflows=inflow, additional_params=add))


def test_merge_network_tables_equal_the_literal_ones():
    from flow_amd.core.kernel.network import NetworkKernel
    from flow_amd.networks.merge import MergeNetwork
    with pytest.raises(KeyError):
        from flow_amd.core import params as P
        MergeNetwork("m", P.VehicleParams(), P.NetParams(additional_params={"merge_length": 100}))
    for pre in (200, 500):
        k = NetworkKernel(merge_network(pre), junction_length=0.1)
        t, ref = k.open_tables(), merge_tables(pre=float(pre))
        for key in ("merge_x", "box_in", "end_x", "net_length"):
            assert abs(t[key] - ref[key]) < 1e-9
        for r in range(2):
            np.testing.assert_allclose(np.array(t["routes"][r]["segments"], float),
                                       np.array(ref["routes"][r]["segments"], float), atol=1e-9)
        assert k.length() == 100 + pre + 100 + 100 + 100 + 0.2 + 45.0 and k.max_speed() == 30
        assert k.get_x(":center_0", 3.0) == 100 + pre + 0.1 == k.get_x(":center_1", 7.0)     # traci.py:283-287
        assert k.open_locate(0, t["merge_x"] + 1.0) == ("center", 1.0)
        assert k.open_coordinate("bottom", 10.0) == (1, t["routes"][1]["start"] + 100.1 + 10.0)


def test_inflows_accept_the_deprecated_spellings_and_validate():
    from flow_amd.core.params import InFlows
    f = InFlows()
    f.add(veh_type="human", edge="e", vehsPerHour=1200, departLane="free", departSpeed=10)      # params.py:1167-1178
    assert f.get()[0] == {"name": "flow_0", "vtype": "human", "edge": "e", "departLane": "free", "departSpeed": 10,
                          "begin": 1, "end": 86400, "vehsPerHour": 1200}
    f.add(veh_type="human", edge="e", period=3, number=7)
    assert f.get()[1]["name"] == "flow_1" and f.get()[1]["number"] == 7 and "end" not in f.get()[1]
    for bad in (dict(), dict(vehs_per_hour=1, period=2), dict(probability=1.5), dict(vehs_per_hour=1, begin=0)):
        with pytest.raises(ValueError):                                                             # :1188-1200
            InFlows().add(veh_type="human", edge="e", **bad)


def test_slot_capacities():
    from flow_amd.envs.spec import slot_capacities
    from flow_amd.utils.exceptions import FatalFlowError
    net = merge_network()
    flows = net.net_params.inflows.get()
    names, caps = slot_capacities(net.vehicles, flows, 64)
    assert names == ["human", "rl"] and sum(caps) == 64 and caps[1] == int(59 * 200 / 2100) and caps[0] >= 5
    assert slot_capacities(net.vehicles, flows, 64, {"human": 40, "rl": 9})[1] == [40, 9]
    assert slot_capacities(net.vehicles, [], 64)[1] == [5, 0]
    with pytest.raises(FatalFlowError):
        slot_capacities(net.vehicles, flows, 3)
    with pytest.raises(FatalFlowError):
        slot_capacities(net.vehicles, flows, 64, {"human": 2, "rl": 9})


def test_reference_merge_fixture_resolves_to_an_open_spec(monkeypatch):
    """tests/fast_tests/test_files/merge.json (committed as tests/golden/merge_flow_params.json): the stored
    flow_params of the merge_0 benchmark load into flow_amd objects and resolve to a simulator spec."""
    from test_host import build_env
    from flow_amd import _lib as L
    from flow_amd.envs import MergePOEnv
    from flow_amd.networks import MergeNetwork
    from flow_amd.utils.rllib import get_flow_params
    fp = get_flow_params(os.path.join(GOLDEN, "merge_flow_params.json"))
    assert fp["env_name"] is MergePOEnv and fp["network"] is MergeNetwork
    assert [f["vehsPerHour"] for f in fp["net"].inflows.get()] == [1800.0, 200.0, 100]
    net = fp["network"](name=fp["exp_tag"], vehicles=fp["veh"], net_params=fp["net"], initial_config=fp["initial"])
    env, spec = build_env(monkeypatch, fp["env_name"], fp["env"], fp["sim"], net)
    assert spec["network"] == "merge" and spec["env"] == L.FS_ENV_MERGE_PO and spec["num_rl"] == 5
    assert spec["num_vehicles"] == 64 and spec["sims_per_step"] == 2 and spec["sim_step"] == 0.2
    assert [f["period"] for f in spec["inflows"]] == [2.0, 18.0, 36.0]
    assert [(f["type"], f["route"], f["depart_speed"]) for f in spec["inflows"]] == [(0, 0, 10.0), (1, 0, 10.0), (0, 1, 7.5)]
    assert spec["init_alive"][0].sum() == 5 and spec["vehicles"][0]["controller"] == L.FS_CTRL_SIM
    assert spec["vehicles"][-1]["controller"] == L.FS_CTRL_RL and spec["vehicles"][0]["max_accel"] == 1.0
    tb = merge_tables(pre=500.0)
    assert abs(spec["merge_x"] - tb["merge_x"]) < 1e-9 and abs(spec["net_length"] - tb["net_length"]) < 1e-9
    assert env.observation_space.shape == (25,) and env.action_space.shape == (5,)
    # the five initial humans: spread evenly over all edges like gen_even_start_pos does (network/base.py:263-391)
    assert [env.initial_state["human_%d" % i][1] for i in range(5)] == \
        ["inflow_highway", "left", "left", "left", "center"]
    assert abs(env.initial_state["human_1"][3] - 79.9) < 1e-9 and abs(env.initial_state["human_4"][3] - 97.4) < 1e-9
    # the oracle accepts the very same dict
    o = O.MergeOracle(spec, np.float64)
    o.reset()
    for _ in range(50):
        o.step(None)
    assert o.total_departed[0] > 5


def test_merge_envs_require_their_additional_params():
    """test_environments.py:646-660, 1171-1183 (test_additional_params)."""
    from flow_amd.core.params import EnvParams, SumoParams
    from flow_amd.envs import MergePOEnv
    from flow_amd.envs.multiagent import MultiAgentMergePOEnv
    net = merge_network()
    full = {"max_accel": 1, "max_decel": 1, "target_velocity": 25, "num_rl": 5}
    for key in full:
        with pytest.raises(KeyError):
            MergePOEnv(EnvParams(additional_params={k: v for k, v in full.items() if k != key}), SumoParams(), net)
    for key in ("max_accel", "max_decel", "target_velocity"):
        with pytest.raises(KeyError):
            MultiAgentMergePOEnv(EnvParams(additional_params={k: v for k, v in full.items() if k != key}),
                                 SumoParams(), net)


def test_open_config_validation_needs_no_gpu():
    from flow_amd import build
    build.build()
    from flow_amd.sim import FlowSim

    def spec(**kw):
        s = merge_spec(R=2, cap_human=6, cap_rl=2, num_rl=1)
        s.update(kw)
        return s
    with pytest.raises(ValueError, match="vehicle type that has no slot"):
        FlowSim(spec(inflows=[dict(type=7, route=0, period=2.0, depart_speed=1.0, depart_pos=5.0)]), "f32")
    with pytest.raises(ValueError, match="inflow route"):
        FlowSim(spec(inflows=[dict(type=0, route=3, period=2.0, depart_speed=1.0, depart_pos=5.0)]), "f32")
    with pytest.raises(ValueError, match="period"):
        FlowSim(spec(inflows=[dict(type=0, route=0, period=0.0, depart_speed=1.0, depart_pos=5.0)]), "f32")
    with pytest.raises(ValueError, match="box_in < merge_x"):
        FlowSim(spec(box_in=400.0), "f32")
    with pytest.raises(ValueError, match="go together"):
        FlowSim(spec(env=S.ENV_ACCEL), "f32")
    with pytest.raises(ValueError, match="init_pos outside the route"):
        FlowSim(spec(init_pos=np.full((2, 8), 9999.0)), "f32")
    with pytest.raises(NotImplementedError, match="PISaturation"):
        s = spec()
        s["vehicles"] = [idm_vehicle(controller=S.CTRL_PISATURATION, type=0)] + s["vehicles"][1:]
        FlowSim(s, "f32")


# ------------------------------------------------------------------ lane drops (BottleneckNetwork)
def test_bottleneck_oracle_facts():
    from helpers import bottleneck_spec
    spec = bottleneck_spec(R=3, horizon=500, seed=1)
    o = O.MergeOracle(spec, np.float64)
    o.reset()
    paths = {}
    rng = np.random.default_rng(0)
    lanes_seen = set()
    for k in range(500):
        obs, rew, done = o.step(rng.uniform(-1.0, 1.0, (3, 20)))
        assert not done.any() or k == 499                      # the zipper look-ahead keeps the joins collision-free
        # nobody ever changes path (lane_change_mode = 0); a path is an entry lane 0..3
        for r in range(3):
            for i in np.flatnonzero(o.alive[r]):
                key = (r, int(o.seq[r, i]))
                assert paths.setdefault(key, int(o.route[r, i])) == int(o.route[r, i])
                lanes_seen.add(int(o.route[r, i]))
        # maxSpeed of RL vehicles stays inside the env's clip, humans keep the type value
        vm = o.vmax[:, 40:][o.alive[:, 40:]]              # 30 = the type value of a vehicle no action has reached yet
        assert (((vm <= 23.0) & (vm >= 0.01)) | (vm == 30.0)).all()
        assert (o.vmax[:, :40] == 30.0).all()
        # nobody drives faster than the edge limit allows (+ one step of acceleration tolerance)
        assert (o.v[o.alive] <= 23.0 + 1e-9).all()
        # observation: counts are multiples of 1/20, outflow consistent with the arrival history
        C = 35
        cnt = obs[:, :2 * C] * 20
        np.testing.assert_allclose(cnt, np.round(cnt), atol=1e-9)
        on_edges = np.array([(o.alive[r] & ~o._segment_lookup(o.x, o.route)[0][r]).sum() for r in range(3)])
        np.testing.assert_array_equal(np.round(cnt).sum(axis=1).astype(int), on_edges)
    assert lanes_seen == {0, 1, 2, 3} and o.total_arrived.min() > 60
    # reward = arrivals of the last 10 steps as a rate / 2000; observed outflow = last 20 steps
    last10 = np.array([o.arr_hist[r][[(o.time_counter[r] - 1 - k) % 20 for k in range(10)]].sum() for r in range(3)])
    np.testing.assert_allclose(rew, 3600 * last10 / (10 * 0.5) / 2000.0)


def test_bottleneck_cell_lookup_by_hand():
    from helpers import bottleneck_spec, bottleneck_tables
    tb = bottleneck_tables()
    spec = bottleneck_spec(R=1, horizon=10)
    o = O.MergeOracle(spec, np.float64)
    o.reset()
    o.route[:] = -1
    # edge 2 starts at 100.1 (3 observed segments of 103.33 m, 2 controlled ones of 155 m), edge 4 at 570.2 (2 lanes)
    for slot, (x, path) in enumerate([(100.1 + 10.0, 3), (100.1 + 200.0, 1), (570.2 + 279.0, 2), (100.05, 0),
                                      (100.1, 2)]):
        o.route[0, slot], o.x[0, slot] = path, x
    cells = o._cell_of(o.cells, last_of_edge=True)[0]
    names = [("1", 0)] * 0
    idx = {}
    c = 0
    for edge, n in [("1", 1), ("2", 3), ("3", 3), ("4", 3), ("5", 1)]:
        lanes = {"1": 4, "2": 4, "3": 4, "4": 2, "5": 1}[edge]
        for k in range(n):
            for lane in range(lanes):
                idx[(edge, k, lane)] = c
                c += 1
    assert cells[0] == idx[("2", 0, 3)] and cells[1] == idx[("2", 1, 1)]
    assert cells[2] == idx[("4", 2, 1)]                       # path 2 drives lane 1 after the first join
    assert cells[3] == -1                                     # on the internal edge ':2_0': not observed
    assert cells[4] == idx[("2", 2, 2)]                       # exactly at the edge start: bucket -1 = last segment
    act = o._cell_of(o.ctl_cells)[0]
    assert act[0] == 0 * 4 + 3 and act[1] == 1 * 4 + 1 and act[2] == 16 + 1 * 2 + 1 and act[3] == -1 and act[4] == -1


def test_zipper_lookahead_orders_the_joining_lanes():
    """M8: inside zipper_distance of a join a vehicle follows the nearest vehicle of either joining lane."""
    from helpers import bottleneck_spec
    spec = bottleneck_spec(R=1, horizon=10, zipper_distance=50.0)
    o = O.MergeOracle(spec, np.float64)
    o.reset()
    o.route[:] = -1
    m1 = float(o.m1)
    for slot, (x, path) in enumerate([(m1 - 20.0, 0), (m1 - 8.0, 1), (m1 - 70.0, 1), (m1 - 60.0, 2), (m1 + 30.0, 3)]):
        o.route[0, slot], o.x[0, slot] = path, x
    o._update_neighbours(np.ones(1, bool))
    assert o.lead[0, 0] == 1                    # lane 0 inside the zone: the lane-1 vehicle ahead is its leader
    assert not o.lead_same_lane[0, 0]           # ... but they are not on one physical lane yet: no collision test
    assert o.lead[0, 2] == 1 and o.lead_same_lane[0, 2]      # outside the zone: own lane only
    assert o.lead[0, 3] == 4 and o.lead[0, 1] == -1          # path 2 joins path 3's lane; path 1's lane is free ahead


def test_bottleneck_network_tables_and_spec(monkeypatch):
    from helpers import bottleneck_tables
    from test_host import build_env
    from flow_amd import _lib as L
    from flow_amd.core.kernel.network import NetworkKernel
    from flow_amd.core import params as P
    from flow_amd.envs import BottleneckDesiredVelocityEnv
    from flow_amd.networks import BottleneckNetwork
    from flow_amd.controllers import RLController, SimLaneChangeController, ContinuousRouter
    with pytest.raises(KeyError):
        BottleneckNetwork("b", P.VehicleParams(), P.NetParams(additional_params={"scaling": 1}))
    v = P.VehicleParams()
    v.add(veh_id="human", lane_change_controller=(SimLaneChangeController, {}), routing_controller=(ContinuousRouter, {}),
          car_following_params=P.SumoCarFollowingParams(speed_mode="all_checks"),
          lane_change_params=P.SumoLaneChangeParams(lane_change_mode=0), num_vehicles=1)
    v.add(veh_id="followerstopper", acceleration_controller=(RLController, {}),
          car_following_params=P.SumoCarFollowingParams(speed_mode=9),
          lane_change_params=P.SumoLaneChangeParams(lane_change_mode=0), num_vehicles=1)
    inflow = P.InFlows()
    inflow.add(veh_type="human", edge="1", vehs_per_hour=2070, departLane="random", departSpeed=10)
    inflow.add(veh_type="followerstopper", edge="1", vehs_per_hour=230, departLane="random", departSpeed=10)
    net = BottleneckNetwork("b", v, P.NetParams(inflows=inflow, additional_params={"scaling": 1, "speed_limit": 23}),
                            P.InitialConfig(spacing="uniform", min_gap=5, lanes_distribution=float("inf"),
                                            edges_distribution=["2", "3", "4", "5"]))
    k = NetworkKernel(net, junction_length=0.1)
    t, ref = k.open_tables(), bottleneck_tables()
    for key in ("merge1_x", "merge2_x", "end_x", "net_length", "num_paths", "box_in"):
        assert abs(t[key] - ref[key]) < 1e-9, key
    np.testing.assert_allclose(np.array(t["routes"][0]["segments"], float),
                               np.array(ref["routes"][0]["segments"], float), atol=1e-9)
    assert net.get_bottleneck_lanes(3) == [1, 0] and k.num_lanes("4") == 2 and k.max_speed() == 23
    add = {"target_velocity": 40, "disable_tb": True, "disable_ramp_metering": True,
           "controlled_segments": [("1", 1, False), ("2", 2, True), ("3", 2, True), ("4", 2, True), ("5", 1, False)],
           "symmetric": False, "observed_segments": [("1", 1), ("2", 3), ("3", 3), ("4", 3), ("5", 1)],
           "reset_inflow": False, "lane_change_duration": 5, "max_accel": 3, "max_decel": 3, "inflow_range": [1000, 2000]}
    env, spec = build_env(monkeypatch, BottleneckDesiredVelocityEnv,
                          P.EnvParams(warmup_steps=40, horizon=1000, additional_params=add),
                          P.SumoParams(sim_step=0.5, restart_instance=True), net)
    assert spec["network"] == "bottleneck" and spec["env"] == L.FS_ENV_BOTTLENECK_DV and spec["num_paths"] == 4
    assert spec["num_vehicles"] == 64 and spec["num_rl"] == 20 and len(spec["obs_cells"]) == 35
    assert spec["obs_outflow_window"] == 20 and spec["reward_outflow_window"] == 10 and spec["speed_limit"] == 23
    assert spec["junction"]["enabled"] == 0 and spec["zipper_distance"] == 50.0
    assert env.observation_space.shape == (141,) and env.action_space.shape == (20,)
    assert env.action_index == {"2": [0], "3": [8], "4": [16]}
    from helpers import segment_cells
    assert spec["obs_cells"] == segment_cells(ref, [("1", 1), ("2", 3), ("3", 3), ("4", 3), ("5", 1)])
    assert spec["action_cells"] == segment_cells(ref, [("2", 2), ("3", 2), ("4", 2)])
    # a lane_change_mode that lets SUMO change lanes (1621 in examples/exp_configs/non_rl/bottleneck.py) switches the
    # simplified lane-change model on for that type (M11); 0 and 512 (no autonomous changes) leave it off
    v2 = P.VehicleParams()
    v2.add(veh_id="human", lane_change_params=P.SumoLaneChangeParams(lane_change_mode=1621), num_vehicles=1)
    v2.add(veh_id="followerstopper", acceleration_controller=(RLController, {}), num_vehicles=1)
    net2 = BottleneckNetwork("b", v2, P.NetParams(inflows=inflow, additional_params={"scaling": 1, "speed_limit": 23}))
    _, spec2 = build_env(monkeypatch, BottleneckDesiredVelocityEnv, P.EnvParams(additional_params=add),
                         P.SumoParams(sim_step=0.5, lane_change_cooldown=4.0), net2)
    assert spec2["vehicles"][0]["lane_change_mode"] == 1621 and spec2["vehicles"][-1]["lane_change_mode"] == 512
    assert spec2["lane_change_cooldown_steps"] == 8 and spec2["lane_change_min_gain"] == 10.0
    with pytest.raises(NotImplementedError, match="scaling"):
        net3 = BottleneckNetwork("b", v, P.NetParams(inflows=inflow, additional_params={"scaling": 2, "speed_limit": 23}))
        build_env(monkeypatch, BottleneckDesiredVelocityEnv, P.EnvParams(additional_params=add), P.SumoParams(), net3)


def test_bottleneck_config_validation_needs_no_gpu():
    from flow_amd import build
    build.build()
    from helpers import bottleneck_spec
    from flow_amd.sim import FlowSim
    with pytest.raises(NotImplementedError, match="more than 32 vehicle slots"):
        FlowSim(bottleneck_spec(R=1, cap_human=20, cap_rl=4), "f32")
    with pytest.raises(ValueError, match="go together"):
        FlowSim(bottleneck_spec(R=1, env=O.ENV_MERGE_PO), "f32")
    with pytest.raises(ValueError, match="outflow windows"):
        FlowSim(bottleneck_spec(R=1, obs_outflow_window=30), "f32")
    with pytest.raises(ValueError, match="merge1_x <= merge2_x"):
        FlowSim(bottleneck_spec(R=1, merge1_x=900.0), "f32")
    with pytest.raises(NotImplementedError, match="256 vehicle slots"):      # k_steps_wide: at most four waves per replica
        FlowSim(bottleneck_spec(R=1, cap_human=250, cap_rl=7), "f32")
    with pytest.raises(NotImplementedError, match="FS_NET_BOTTLENECK only"):
        FlowSim(merge_spec(R=1, cap_human=60, cap_rl=6, num_rl=2), "f32")
    with pytest.raises(NotImplementedError, match="more than 64 vehicle slots"):    # scaling 2: the wide kernel only
        FlowSim(bottleneck_spec(R=1, cap_human=50, cap_rl=10, scaling=2), "f32")
    with pytest.raises(NotImplementedError, match="must be 4 or 8"):
        FlowSim(bottleneck_spec(R=1, cap_human=100, cap_rl=10, num_paths=12), "f32")


def test_scaling_two_oracle_facts():
    """BottleneckNetwork scaling 2: eight entry lanes join to four, then to two; lane = path >> joins passed."""
    from helpers import bottleneck_spec
    spec = bottleneck_spec(R=1, cap_human=120, cap_rl=20, horizon=250, seed=3, q=4000.0, scaling=2)
    assert spec["num_paths"] == 8 and len(spec["obs_cells"]) == 70 and len(spec["action_cells"]) == 40
    ora = O.MergeOracle(spec, np.float32)
    ora.reset()
    for k in range(250):
        obs, rew, done = ora.step(None)
        np.testing.assert_array_equal(ora.alive.sum(axis=1) + ora.total_arrived, 2 + ora.total_departed)
    a = ora.alive[0]
    x, p = ora.x[0][a], ora.route[0][a]
    assert set(p) == set(range(8)) and obs.shape == (1, 281)
    lane = p >> ((x >= spec["merge1_x"]).astype(int) + (x >= spec["merge2_x"]).astype(int))
    assert lane[x >= spec["merge2_x"]].max() <= 1 and lane[(x >= spec["merge1_x"]) & (x < spec["merge2_x"])].max() <= 3
    # nobody overlaps its leader on its own physical lane
    for i in np.nonzero(a)[0]:
        j = ora.lead[0][i]
        if j >= 0 and ora.lead_same_lane[0][i]:
            assert ora.x[0][j] - ora.x[0][i] - 5.0 > -1e-3


def test_wide_oracle_runs_beyond_64_slots_and_the_queue_outgrows_one_wave():
    """The oracle has no slot limit of its own: a heavy demand on 200 slots keeps more than 64 vehicles in the network
    (what the 64-slot kernel has to drop at insertion), conserves vehicles, and drops fewer than a 64-slot pool."""
    from helpers import bottleneck_spec
    spec = bottleneck_spec(R=1, cap_human=180, cap_rl=20, horizon=400, seed=2, q=3600.0)
    spec64 = bottleneck_spec(R=1, cap_human=56, cap_rl=8, horizon=400, seed=2, q=3600.0)
    ora, o64 = O.MergeOracle(spec, np.float32), O.MergeOracle(spec64, np.float32)
    ora.reset(), o64.reset()
    rng = np.random.default_rng(0)
    steps = 0
    while steps < 400 and not (ora.alive.sum() > 80):
        ora.step(rng.uniform(-1, 1, (1, spec["num_rl"])).astype(np.float32))
        o64.step(None)
        steps += 1
        np.testing.assert_array_equal(ora.alive.sum(axis=1) + ora.total_arrived, 2 + ora.total_departed)
    assert ora.alive.sum() > 80 and o64.alive.sum() <= 64
    assert (o64.total_dropped > ora.total_dropped).all()             # the 64-slot pool drops what does not fit


def test_fixed_point_and_slot_order_cell_sums_stay_within_their_derived_bounds_of_the_float64_sum():
    """The mean-speed observations of BottleneckDesiredVelocityEnv (flow/envs/bottleneck.py:900-935: the speeds of a
    lane-segment added in float64 in id order, divided by the count and by 50) as the float32 oracle states them, against
    that float64 sum of the oracle's OWN float32 speeds, with bounds derived here (u = 2^-24, the relative error of one
    float32 rounding; gamma(k) = k u / (1 - k u) bounds k roundings in a row):
      cell_sum = 'fixed' (k_drop_queue, k_steps_wide): every speed is rounded to a multiple of 2^-16 m/s, at most 2^-17 off,
        the integer sum is exact, so the sum of n speeds is at most n 2^-17 off and the mean 2^-17; three roundings follow
        (integer -> float32; / n: fl(fl(n / 20) 20) == n is checked below; / 50):
            (2^-17 (1 + gamma(3)) + gamma(3) speed_limit) / 50  =  2.35e-7 per entry;
      cell_sum = 'slot' (k_steps_open): a float32 sum of n speeds in slot order, n - 1 roundings, then / n and / 50:
            gamma(n + 1) speed_limit / 50  =  (n + 1) 2.74e-8 per entry -- 1e-6 up to 35 vehicles in a lane-segment, the
        figure of tests/test_dropq_gpu.py's comparison of the two kernels.
    The vehicle counts are equal, and the largest deviation seen is positive: the sums compared are different sums."""
    from helpers import bottleneck_spec
    spec = bottleneck_spec(R=2, cap_human=100, cap_rl=20, horizon=300, seed=6, q=3600.0)
    ora = O.MergeOracle(dict(spec, cell_sum="fixed"), np.float32)
    ora.reset()
    N, C, vlim = ora.N, len(spec["obs_cells"]), float(spec["speed_limit"])
    u = 2.0 ** -24
    gamma = lambda k: k * u / (1.0 - k * u)                          # noqa: E731
    cnts = np.arange(1, N + 1, dtype=np.float32)
    np.testing.assert_array_equal((cnts / np.float32(20)) * np.float32(20), cnts)      # un-normalising the count is exact
    bound_fixed = (2.0 ** -17 * (1.0 + gamma(3)) + gamma(3) * vlim) / 50.0
    assert 2.3e-7 < bound_fixed < 2.4e-7
    rng = np.random.default_rng(1)
    worst_fixed = worst_slot = 0.0
    most_in_a_cell = 0
    for k in range(200):
        ora.spec["cell_sum"] = "fixed"
        obs_fixed = ora.step(rng.uniform(-1.0, 1.0, (2, spec["num_rl"])).astype(np.float32))[0]
        ora.spec["cell_sum"] = "slot"
        obs_slot = ora.get_state() if k % 4 == 3 else None            # (the oracle's slot-order sum is its slow one)
        assert obs_fixed.dtype == np.float32
        assert float(ora.v[ora.alive].max()) <= vlim
        cell = ora._cell_of(ora.cells, last_of_edge=True)
        for r in range(2):
            num = np.zeros((2, C))                                     # [human | RL], float64 as in the reference
            speeds = np.zeros((2, C))
            for i in sorted(np.flatnonzero(cell[r] >= 0), key=lambda i: ora.seq[r, i]):       # id order
                speeds[int(ora.is_rl[i]), cell[r, i]] += float(ora.v[r, i])
                num[int(ora.is_rl[i]), cell[r, i]] += 1
            norm = num / 20
            unnorm = norm * 20
            mean = np.array([[speeds[t, c] / unnorm[t, c] if int(unnorm[t, c]) else 0 for c in range(C)]
                             for t in range(2)]) / 50
            want = np.concatenate([norm[0], norm[1], mean[0], mean[1]])
            n_c = np.concatenate([num[0], num[1]])
            most_in_a_cell = max(most_in_a_cell, int(n_c.max()))
            np.testing.assert_array_equal(obs_fixed[r, :2 * C], want[:2 * C].astype(np.float32))
            dev_fixed = np.abs(obs_fixed[r, 2 * C:4 * C].astype(np.float64) - want[2 * C:])
            assert (dev_fixed <= bound_fixed).all(), (k, dev_fixed.max())
            worst_fixed = max(worst_fixed, dev_fixed.max())
            if obs_slot is not None:
                assert obs_slot.dtype == np.float32
                np.testing.assert_array_equal(obs_slot[r, :2 * C], want[:2 * C].astype(np.float32))
                dev_slot = np.abs(obs_slot[r, 2 * C:4 * C].astype(np.float64) - want[2 * C:])
                assert (dev_slot <= gamma(n_c + 1) * vlim / 50.0).all(), (k, dev_slot.max())
                worst_slot = max(worst_slot, dev_slot.max())
    print("largest deviation: fixed %.3g (bound %.3g), slot %.3g; most vehicles in a lane-segment %d"
          % (worst_fixed, bound_fixed, worst_slot, most_in_a_cell))
    assert worst_fixed > 0 and worst_slot > 0
    assert most_in_a_cell >= 8 and ora.alive.sum(axis=1).min() > 40     # (sums of several speeds were compared)


def test_simplified_lane_changing_facts():
    """M11: vehicles change to an adjacent lane with a clearly larger leader gap, never inside a zipper zone or on an
    internal edge, at most one per replica and step, not again before the cool-down, never into an unsafe gap."""
    from helpers import bottleneck_spec
    spec = bottleneck_spec(R=3, horizon=400, seed=2, lane_change_cooldown_steps=10, lane_change_min_gain=10.0)
    for v in spec["vehicles"][:40]:
        v["lane_change_mode"] = 1621                     # the humans; the RL type keeps 0
    o = O.MergeOracle(spec, np.float64)
    o.reset()
    changes = np.zeros(3, dtype=int)
    for k in range(400):
        before = o.route.copy()
        seq_before = o.seq.copy()
        alive_before = o.alive.copy()
        x_before = o.x.copy()
        _, _, done = o.step(None)
        assert not done.any() or k == 399
        same = alive_before & o.alive & (seq_before == o.seq)
        moved = same & (before != o.route)
        assert (moved.sum(axis=1) <= 1).all()
        assert not moved[:, 40:].any()                    # lane_change_mode 0: the RL type never changes lane
        for r, i in zip(*np.nonzero(moved)):
            g = int(o.shift(x_before[r:r + 1, i])[0])
            assert g < 2 and int(o.shift(x_before[r:r + 1, i] + o.zip_d)[0]) == g       # not in a zipper zone
            assert abs((before[r, i] >> g) - (o.route[r, i] >> g)) == 1                  # to an adjacent lane
            assert o.last_lc[r, i] == o.time_counter[r]
            if o.lead[r, i] >= 0 and o.lead_same_lane[r, i]:
                assert o.h[r, i] > 2.0                   # it did not land on top of its new leader
        changes += moved.sum(axis=1)
    assert (changes > 50).all()
    # cool-down: no vehicle has two changes closer than 10 steps -- checked through last_lc bookkeeping above; the lanes
    # ahead of the first join are used evenly enough that nobody is starved
    assert o.total_arrived.min() > 40


def test_inflows_and_vehicle_types_match_the_reference_golden():
    """tests/golden/inflows.json: what the reference's own InFlows.add / VehicleParams.add produce (generated by
    importing flow.core.params, gen_golden.py: gen_inflows) for the calls of the merge / bottleneck experiments."""
    import json
    from flow_amd.controllers import ContinuousRouter, RLController, SimLaneChangeController
    from flow_amd.core import params as P
    gold = json.load(open(os.path.join(GOLDEN, "inflows.json")))
    inflow = P.InFlows()
    for c in gold["calls"]:
        inflow.add(**dict(c))
    assert inflow.get() == gold["flows"]
    for case in gold["errors"]:
        if case["error"] is None:
            P.InFlows().add(veh_type="human", edge="e", **case["args"])
        else:
            with pytest.raises(ValueError):
                P.InFlows().add(veh_type="human", edge="e", **case["args"])
            assert case["error"] == "ValueError"
    v = P.VehicleParams()
    v.add(veh_id="human", lane_change_controller=(SimLaneChangeController, {}), routing_controller=(ContinuousRouter, {}),
          car_following_params=P.SumoCarFollowingParams(speed_mode="all_checks"),
          lane_change_params=P.SumoLaneChangeParams(lane_change_mode=0), num_vehicles=1)
    v.add(veh_id="followerstopper", acceleration_controller=(RLController, {}),
          car_following_params=P.SumoCarFollowingParams(speed_mode=9),
          lane_change_params=P.SumoLaneChangeParams(lane_change_mode=1621), num_vehicles=1)
    for name, want in gold["vehicle_types"].items():
        tp = v.type_parameters[name]
        assert tp["acceleration_controller"][0].__name__ == want["acceleration_controller"]
        assert tp["lane_change_controller"][0].__name__ == want["lane_change_controller"]
        assert tp["car_following_params"].speed_mode == want["speed_mode"]
        assert tp["car_following_params"].controller_params == want["controller_params"]
        assert tp["lane_change_params"].lane_change_mode == want["lane_change_mode"]
        assert tp["initial_speed"] == want["initial_speed"]
    assert [(t["veh_id"], t["num_vehicles"], t["initial_speed"]) for t in v.initial] == \
        [(t["veh_id"], t["num_vehicles"], t["initial_speed"]) for t in gold["initial"]]


def test_probabilistic_inflow_statistics_of_the_oracle():
    """M2b: a flow with probability p per second generates Binomial(n_trials, p * sim_step) vehicles over n_trials
    sub-steps; deterministic for a seed, different between replicas and episodes, capped by `number`."""
    from helpers import merge_spec
    spec = merge_spec(R=64, cap_human=40, cap_rl=4, num_rl=2, horizon=400, seed=3)
    spec["vehicles"] = [dict(v, noise=0.0) for v in spec["vehicles"]]
    fl = dict(spec["inflows"][0], probability=0.5)
    fl.pop("period")
    spec["inflows"] = [fl] + [dict(f) for f in spec["inflows"][1:]]
    a, b = O.MergeOracle(spec, np.float32), O.MergeOracle(spec, np.float32)
    a.reset(), b.reset()
    for _ in range(400):
        a.step(None), b.step(None)
    np.testing.assert_array_equal(a.generated, b.generated)
    g = a.generated[:, 0].astype(np.float64)
    n_trials = 400 - 5 + 1                      # trials start at now = begin = 1.0 s = sub-step 5 (now = (n - 1) * 0.2)
    mean, std = n_trials * 0.5 * 0.2, (n_trials * 0.1 * 0.9) ** 0.5
    assert abs(g.mean() - mean) < 4 * std / 8 and 0.5 * std < g.std() < 1.6 * std, (g.mean(), g.std(), mean, std)
    assert (a.emitted[:, 0] <= a.generated[:, 0]).all()
    first = a.generated[:, 0].copy()
    a.reset()
    for _ in range(400):
        a.step(None)
    assert (a.generated[:, 0] != first).any()   # the next episode draws anew
    fl2 = dict(fl, number=7)
    c = O.MergeOracle(dict(spec, inflows=[fl2] + spec["inflows"][1:]), np.float32)
    c.reset()
    for _ in range(400):
        c.step(None)
    assert (c.generated[:, 0] == 7).all()


def test_merge_po_lists_follow_the_reference_list_operations_across_resets():
    """O2: MergePOEnv.additional_command (merge.py:189-221) restated with its own Python list operations -- including
    `for veh_id in self.rl_veh: ... self.rl_veh.remove(veh_id)` (removing from the list being iterated skips the next
    entry) and the fact that reset() (merge.py:223-231) never clears rl_veh -- and driven by the vehicles the oracle
    has in the network at every call: the oracle's rl_veh (slots ordered by ctl_seq) must be that list, step by step,
    over three episodes."""
    import collections
    from helpers import merge_spec
    spec = merge_spec(R=3, cap_human=10, cap_rl=8, num_rl=4, horizon=10 ** 6, seed=5, q_rl=1500.0, q_highway=600.0)
    spec["vehicles"] = [dict(v, noise=0.0) for v in spec["vehicles"]]
    ora = O.MergeOracle(spec, np.float32)
    R, num_rl = 3, 4
    queues = [collections.deque() for _ in range(R)]
    lists = [[] for _ in range(R)]
    skipped = [0]

    def vehicle_ids(r):
        """ids of the RL vehicles of replica r now in the network, in the order they entered"""
        alive = ora.alive[r] & ora.is_rl
        slots = sorted(np.flatnonzero(alive), key=lambda i: ora.seq[r, i])
        return [(int(ora.episode[r]) if ora.origin[r, i] >= 0 else -1, int(ora.origin[r, i])) for i in slots]

    def oracle_list(r):
        slots = sorted(np.flatnonzero(ora.ctl_seq[r] >= 0), key=lambda i: ora.ctl_seq[r, i])
        return [i for i in slots]

    original = ora._additional_command

    def hooked(active):
        for r in range(R):
            if not active[r]:
                continue
            rl_ids = vehicle_ids(r)
            rl_queue, rl_veh = queues[r], lists[r]
            for veh_id in rl_ids:                                     # merge.py:201-203
                if veh_id not in list(rl_queue) + rl_veh:
                    rl_queue.append(veh_id)
            for veh_id in list(rl_queue):                             # :205-207
                if veh_id not in rl_ids:
                    rl_queue.remove(veh_id)
            before = len(rl_veh)
            gone = sum(1 for v in rl_veh if v not in rl_ids)
            for veh_id in rl_veh:                                     # :208-210 (iterates the list it shrinks)
                if veh_id not in rl_ids:
                    rl_veh.remove(veh_id)
            skipped[0] += gone - (before - len(rl_veh))
            while len(rl_queue) > 0 and len(rl_veh) < num_rl:         # :213-215
                rl_veh.append(rl_queue.popleft())
        original(active)
        for r in range(R):
            if not active[r]:
                continue
            got = []
            for i in oracle_list(r):
                alive = ora.alive[r, i] and ora.is_rl[i]
                got.append((int(ora.episode[r]) if ora.origin[r, i] >= 0 else -1, int(ora.origin[r, i])) if alive else None)
            want = [v if v in vehicle_ids(r) else None for v in lists[r]]
            assert got == want, (r, got, want)

    ora._additional_command = hooked
    ora.reset()
    for episode in range(3):
        for _ in range(220):
            ora.step(np.zeros((R, num_rl), dtype=np.float32))
        assert all(len(v) == num_rl for v in lists)                   # the places are taken when the episode ends
        obs = ora.reset()
        # the first observation of the next episode shows the stale entries as rows of the accessors' error values
        np.testing.assert_allclose(obs[:, 0], -1001.0 / 30.0, rtol=1e-6)
    assert skipped[0] > 0                                             # the skipping did occur (after every reset)
