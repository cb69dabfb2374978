"""MultiRingNetwork / MultiWaveAttenuationPOEnv / lord_of_the_rings.py, host side (tests/test_multi_ring_gpu.py runs the
kernels): the oracle's vectorised reward against the literal per-vehicle one, the network's start positions against the
literal restatement of gen_custom_start_pos, edge starts, routes, spaces, ids, build_spec's rows, the experiment file's
parameters against the reference's (tests/golden/lord_of_the_rings_params.json), and the refusals."""
import importlib
import json
import math
import os

import numpy as np
import pytest

import multi_ring_ref as M
from flow_amd import _lib as L
from flow_amd import controllers as FC
from flow_amd.core import params as P
from flow_amd.core.kernel.network import NetworkKernel
from flow_amd.envs.multiagent import MultiWaveAttenuationPOEnv
from flow_amd.networks import MultiRingNetwork
from flow_amd.networks.multi_ring import ADDITIONAL_NET_PARAMS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def train(monkeypatch):
    monkeypatch.syspath_prepend(os.path.join(ROOT, "examples"))
    return importlib.import_module("train")               # (installs flow_amd as `flow`, as the experiment files need)


# ------------------------------------------------------------------------------------------- the reward
def reward_state(rng, R, N, fronts):
    """Rows of N speeds and positions; row r gets ``fronts[r % len(fronts)]`` fronts inside junctions."""
    x = np.sort(rng.uniform(0.0, 230.39, (R, N)), axis=1)
    v = rng.uniform(0.0, 9.0, (R, N))
    centres = np.array([57.55, 115.15, 172.75, 230.35])
    q = 57.6
    for r in range(R):
        on = (x[r] - np.floor(x[r] / q) * q) < 57.5
        x[r] = np.where(on, x[r], x[r] - 0.2)                        # nobody in a junction by chance ...
        slots = rng.permutation(N)[:fronts[r % len(fronts)]]
        x[r, slots] = rng.choice(centres, len(slots)) + rng.uniform(-0.049, 0.049, len(slots))     # ... but the chosen
    return x, v


@pytest.mark.parametrize("N", [22, 4, 2])
def test_vectorised_reward_equals_the_literal_one(N):
    rng = np.random.default_rng(N)
    R = 12
    fronts = [0, 1, 2, 0] if N > 2 else [0, 1, 2]
    x, v = reward_state(rng, R, N, fronts)
    v[3, 0] = -150.0                                                 # a speed below -100 ...
    x[3, 0] = 10.0                                                   # ... on an edge: reward 0
    spec = M.multi_ring_spec(R=R, N=N, noise=0.0, target=4.3)
    ora = M.MultiRingOracle(spec, np.float64)
    ora.x[:], ora.v[:] = x, v
    got = ora.compute_reward(np.zeros((R, 1)), np.zeros(R, bool))
    want = np.array([M.literal_reward(x[r], v[r], 230.0, 0.1, 4.3) for r in range(R)])
    assert set(fronts) <= {N - int(n) for n in ora.last_n}
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)        # (NaN equals NaN: two fronts of two in junctions)
    assert got[3] == 0.0 and (N != 2 or np.isnan(got).any()) and np.nanmax(got) > 0
    assert np.array_equal(ora.compute_reward(None, np.zeros(R, bool)), np.zeros(R))      # the warm-up steps
    assert M.literal_reward(x[0], v[0], 230.0, 0.1, 4.3, have_actions=False) == 0.0


def test_a_speed_below_minus_100_inside_a_junction_does_not_zero_the_reward():
    spec = M.multi_ring_spec(R=1, N=4, noise=0.0)
    ora = M.MultiRingOracle(spec, np.float64)
    ora.x[:] = [[10.0, 57.55, 120.0, 180.0]]
    ora.v[:] = [[3.0, -150.0, 4.0, 5.0]]
    got = ora.compute_reward(np.zeros((1, 1)), np.zeros(1, bool))
    assert got[0] == pytest.approx(M.literal_reward(ora.x[0], ora.v[0], 230.0, 0.1, 4.0), abs=1e-12) and got[0] > 0


def test_max_cost_precondition_the_running_sum_equals_numpys_norm():
    """The library builds max_cost[n] from a running float64 sum of target^2 (flowsim_sim.h); the oracle takes numpy's
    norm.  For the targets the bit-for-bit tests use, 4 and 4.3, and n = 0 .. 32 the two agree after rounding to float32
    (exactly: what the float32 bit-for-bit tests need) and in float64 to 1e-13 -- either sum of n <= 32 terms carries a
    relative error of at most n 2^-53, the root halves it: 32 x 1.1e-16 x 24.4 / 2 = 4.3e-14 -- far inside the 1e-9 at
    which the float64 tests hold the reward."""
    for target in (4.0, 4.3):
        ss, lib = 0.0, []
        for n in range(33):
            lib.append(math.sqrt(ss))
            ss += target * target
        want = M.max_cost_table(target, 32, np.float64)
        assert np.array_equal(np.float32(lib), M.max_cost_table(target, 32, np.float32)), target
        assert np.all(np.abs(np.array(lib) - want) <= 1e-13), target


# ------------------------------------------------------------------------------------------- the network
def make_network(num_rings, per_ring, bunching, spacing="custom", lanes=1, n_rl=1):
    v = P.VehicleParams()
    for i in range(num_rings):
        v.add("human_{}".format(i), acceleration_controller=(FC.IDMController, {"noise": 0.2}),
              routing_controller=(FC.ContinuousRouter, {}), num_vehicles=per_ring - n_rl)
        v.add("rl_{}".format(i), acceleration_controller=(FC.RLController, {}), routing_controller=(FC.ContinuousRouter, {}),
              num_vehicles=n_rl)
    add = dict(ADDITIONAL_NET_PARAMS, num_rings=num_rings, lanes=lanes)
    return MultiRingNetwork("rings", v, P.NetParams(additional_params=add), P.InitialConfig(bunching=bunching, spacing=spacing))


@pytest.mark.parametrize("num_rings,per_ring,bunching", [(1, 22, 20), (2, 22, 20), (4, 4, 0)])
def test_start_positions_are_the_literal_restatement_exactly(num_rings, per_ring, bunching):
    net = make_network(num_rings, per_ring, bunching)
    pos, lanes = NetworkKernel(net).generate_starting_positions(net.initial_config, num_rings * per_ring)
    want = M.literal_start_positions(num_rings, per_ring, bunching)
    assert pos == want and lanes == [0] * (num_rings * per_ring)
    for n, (edge, p) in enumerate(pos):                              # ring n // per_ring, ascending along the ring
        ring, x = net.ring_coordinate(edge, p)
        assert (ring, x) == M.loop_coordinate(edge, p) and ring == n // per_ring
        assert net.ring_locate(ring, x) == (edge, pytest.approx(p, abs=1e-12))
    if num_rings > 1:                                                # later rings start 1e-13 further along (230 + 1e-13 rounds within 2.9e-14)
        assert pos[per_ring] == ("bottom_1", pytest.approx(1e-13, abs=3e-14)) and pos[0] == ("bottom_0", 0)


def test_edge_starts_routes_and_internal_edges():
    net = make_network(3, 4, 0)
    assert net.edge_starts == [(e + "_%d" % i, q * 57.5 + i * 230.0) for i in range(3)
                               for q, e in enumerate(("bottom", "right", "top", "left"))]
    assert net.routes["top_2"] == ["top_2", "left_2", "bottom_2", "right_2"]
    assert net.routes["right_0"] == ["right_0", "top_0", "left_0", "bottom_0"] and len(net.routes) == 12
    assert [n["id"] for n in net.nodes][:5] == ["bottom_0", "right_0", "top_0", "left_0", "bottom_1"]
    assert [e["id"] for e in net.edges] == [t[0] for t in net.edge_starts] and net.edges[5]["to"] == "top_1"
    k = NetworkKernel(net)
    assert len(k.get_junction_list()) == 12 and k.edge_length(":right_1_0") == 0.1          # (as RingNetwork: 0.1 m each)
    assert k.length() == pytest.approx(3 * 230.4) and k.non_internal_length() == pytest.approx(690.0)
    assert net.ring_locate(1, 57.55) == (":right_1_0", pytest.approx(0.05)) and net.ring_coordinate(":right_1_0", 0.05)[1] == pytest.approx(57.55)
    with pytest.raises(KeyError):
        MultiRingNetwork("rings", P.VehicleParams(), P.NetParams(additional_params={"length": 230, "lanes": 1,
                                                                                     "speed_limit": 30, "resolution": 40}))


# ------------------------------------------------------------------------------------------- the environment's spec
class RecordingSim:
    """Stands in for FlowSim on the CPU: records the spec the env resolved."""
    last = None

    def __init__(self, spec, precision="f32", device=0):
        RecordingSim.last = (spec, precision)
        self.spec = spec
        self.R, self.N = spec["num_replicas"], spec["num_vehicles"]

    def close(self):
        pass


ENV_PARAMS = {"max_accel": 1, "max_decel": 1, "ring_length": [230, 230], "target_velocity": 4}


def build_env(monkeypatch, network, additional=ENV_PARAMS, replicas=1):
    import flow_amd.envs.base as base
    monkeypatch.setattr(base, "FlowSim", RecordingSim)
    env = MultiWaveAttenuationPOEnv.__new__(MultiWaveAttenuationPOEnv)
    env.num_replicas = replicas
    env.__init__(P.EnvParams(horizon=3000, warmup_steps=750, additional_params=dict(additional)),
                 P.SumoParams(sim_step=0.1, seed=5), network)
    return env, RecordingSim.last[0]


def test_spaces_ids_and_the_rows_of_the_spec(monkeypatch):
    net = make_network(2, 22, 20)
    env, spec = build_env(monkeypatch, net, replicas=3)
    assert env.observation_space.shape == (3,) and (env.observation_space.low[0], env.observation_space.high[0]) == (-1, 1)
    assert env.action_space.shape == (1,) and (env.action_space.low[0], env.action_space.high[0]) == (-1, 1)
    assert env.k.vehicle.get_rl_ids() == ["rl_0_0", "rl_1_0"] and env.k.vehicle.get_ids()[21:23] == ["rl_0_0", "human_1_0"]
    assert MultiWaveAttenuationPOEnv.gen_edges(1) == ["top_1", "left_1", "right_1", "bottom_1"]
    assert (spec["num_replicas"], spec["num_vehicles"], spec["num_rl"], spec["num_rings"], spec["num_envs"]) == (6, 22, 1, 2, 3)
    assert spec["env"] == L.FS_ENV_MULTI_WAVE_ATTENUATION_PO == 11 and spec["target_velocity"] == 4.0
    assert spec["po_max_length"] == 230 and spec["warmup_steps"] == 750 and spec["clip_actions"] is False
    assert len(spec["vehicles"]) == 22 and spec["vehicles"][21]["controller"] == L.FS_CTRL_RL
    assert spec["vehicles"][21]["rl_index"] == 0 and spec["vehicles"][0]["noise"] == 0.2
    # row = env * num_rings + ring, INIT_POS per row from the custom start positions
    want = np.zeros((2, 22))
    for n, (edge, p) in enumerate(M.literal_start_positions(2, 22, 20)):
        ring, x = M.loop_coordinate(edge, p)
        want[ring, n % 22] = x
    X = np.asarray(spec["init_pos"])
    assert X.shape == (6, 22)
    for e in range(3):
        for g in range(2):
            assert np.array_equal(X[e * 2 + g], want[g])
    assert np.array_equal(np.asarray(spec["ring_length"]), np.full(6, 230.0))
    assert env.initial_state["human_1_0"][1] == "bottom_1" and env.initial_state["rl_0_0"][1] == "left_0"
    assert env.k.vehicle.get_leader("rl_1_0") == "human_1_0" and env.k.vehicle.get_follower("human_1_0") == "rl_1_0"


def test_refusals_at_construction(monkeypatch):
    with pytest.raises(KeyError, match="target_velocity"):
        build_env(monkeypatch, make_network(2, 22, 20), additional={k: v for k, v in ENV_PARAMS.items() if k != "target_velocity"})
    with pytest.raises(KeyError, match="ring_length"):
        build_env(monkeypatch, make_network(2, 22, 20), additional={k: v for k, v in ENV_PARAMS.items() if k != "ring_length"})
    with pytest.raises(NotImplementedError, match="multi-lane MultiRingNetwork"):
        build_env(monkeypatch, make_network(2, 22, 20, lanes=2))
    with pytest.raises(NotImplementedError, match="exactly one RL vehicle on each ring"):
        build_env(monkeypatch, make_network(2, 22, 20, n_rl=2))
    # rings of different composition: the slot constants are shared by all rows
    v = P.VehicleParams()
    for i, noise in enumerate((0.2, 0.3)):
        v.add("human_{}".format(i), acceleration_controller=(FC.IDMController, {"noise": noise}),
              routing_controller=(FC.ContinuousRouter, {}), num_vehicles=21)
        v.add("rl_{}".format(i), acceleration_controller=(FC.RLController, {}), routing_controller=(FC.ContinuousRouter, {}),
              num_vehicles=1)
    net = MultiRingNetwork("rings", v, P.NetParams(additional_params=dict(ADDITIONAL_NET_PARAMS, num_rings=2)),
                           P.InitialConfig(bunching=20, spacing="custom"))
    with pytest.raises(NotImplementedError, match="same vehicles in the same slot order"):
        build_env(monkeypatch, net)
    # the environment and the network go together
    from flow_amd.envs import WaveAttenuationPOEnv
    import flow_amd.envs.base as base
    monkeypatch.setattr(base, "FlowSim", RecordingSim)
    with pytest.raises(NotImplementedError, match="go together"):
        WaveAttenuationPOEnv(P.EnvParams(additional_params=dict(ENV_PARAMS)), P.SumoParams(), make_network(1, 22, 20))


def lib_refuses(spec, precision="f32"):
    """fs_create's validation runs before any device call: the refusals need no GPU."""
    from flow_amd.sim import FlowSim
    with pytest.raises((NotImplementedError, ValueError)) as e:
        FlowSim(spec, precision=precision)
    return str(e.value)


def test_library_refusals_by_name():
    from helpers import figure_eight_spec, idm_vehicle
    from oracle import refsim as S
    ok = M.multi_ring_spec(R=2, N=22, noise=0.0)
    two = dict(ok, num_rl=2, vehicles=ok["vehicles"][:20] + [idm_vehicle(controller=S.CTRL_RL, rl_index=k) for k in range(2)])
    assert "num_rl = 1" in lib_refuses(two)
    assert "num_rl = 1" in lib_refuses(dict(ok, num_rl=0, vehicles=[idm_vehicle() for _ in range(22)]))
    assert "multi-lane ring" in lib_refuses(dict(ok, num_lanes=2, init_lane=np.zeros((2, 22), np.int32)))
    loop = figure_eight_spec(R=2, N=14)
    loop.update(env=M.ENV_MULTI_WAVE_ATTENUATION_PO, num_rl=1,
                vehicles=loop["vehicles"][:13] + [idm_vehicle(controller=S.CTRL_RL, rl_index=0)])
    assert "segment-table loop" in lib_refuses(loop)
    assert "FS_ENV_MULTI_WAVE_ATTENUATION_PO" in lib_refuses(ok, "mixed")


# ------------------------------------------------------------------------------------------- the experiment file
def test_the_experiment_file_has_the_references_values(train):
    with open(os.path.join(ROOT, "tests", "golden", "lord_of_the_rings_params.json")) as f:
        ref = json.load(f)
    module, multiagent = train.load_experiment("lord_of_the_rings")
    assert multiagent and module.__name__.endswith("multiagent.lord_of_the_rings")
    assert (module.HORIZON, module.NUM_RINGS, module.N_ROLLOUTS, module.N_CPUS) == \
        (ref["HORIZON"], ref["NUM_RINGS"], ref["N_ROLLOUTS"], ref["N_CPUS"])
    assert module.POLICIES_TO_TRAIN == ref["policies_to_train"] and module.policy_mapping_fn("rl_0_0") == "av"
    fp = module.flow_params
    assert fp["exp_tag"] == ref["exp_tag"] and fp["simulator"] == ref["simulator"]
    assert fp["env_name"].__name__ == ref["env_name"] and fp["env_name"] is MultiWaveAttenuationPOEnv
    assert fp["network"].__name__ == ref["network"] and fp["network"] is MultiRingNetwork
    assert fp["sim"].sim_step == ref["sim"]["sim_step"] and fp["sim"].render is ref["sim"]["render"]
    assert (fp["env"].horizon, fp["env"].warmup_steps) == (ref["env"]["horizon"], ref["env"]["warmup_steps"])
    assert fp["env"].additional_params == ref["env"]["additional_params"]
    assert fp["net"].additional_params == ref["net"]
    assert (fp["initial"].bunching, fp["initial"].spacing) == (ref["initial"]["bunching"], ref["initial"]["spacing"])
    types_ = fp["veh"].initial
    assert len(types_) == 2 * ref["NUM_RINGS"]
    for t, want in zip(types_, ref["vehicles_per_ring"]):
        assert t["veh_id"] == want["veh_id"].format(ring=0) and t["num_vehicles"] == want["num_vehicles"]
        assert t["acceleration_controller"][0].__name__ == want["controller"]
        assert (t["acceleration_controller"][1] or {}) == want["controller_params"]
        assert t["routing_controller"][0].__name__ == want["router"]


def test_num_rings_selects_the_experiment(train, monkeypatch):
    path = os.path.join(ROOT, "examples", "exp_configs", "rl", "multiagent", "lord_of_the_rings.py")
    with open(path) as f:
        text = f.read()
    assert text.count("NUM_RINGS = 1\n") == 1
    scope = {"__name__": "lord_of_the_rings_3"}
    exec(compile(text.replace("NUM_RINGS = 1\n", "NUM_RINGS = 3\n"), path, "exec"), scope)
    fp = scope["flow_params"]
    assert fp["exp_tag"] == "lord_of_numrings3" and fp["net"].additional_params["num_rings"] == 3
    assert [t["veh_id"] for t in fp["veh"].initial] == ["human_0", "rl_0", "human_1", "rl_1", "human_2", "rl_2"]
    network = fp["network"](name=fp["exp_tag"], vehicles=fp["veh"], net_params=fp["net"], initial_config=fp["initial"])
    import flow_amd.envs.base as base
    monkeypatch.setattr(base, "FlowSim", RecordingSim)
    env = fp["env_name"](fp["env"], fp["sim"], network)
    spec = RecordingSim.last[0]
    assert (spec["num_replicas"], spec["num_vehicles"], spec["num_rings"]) == (3, 22, 3) and env.action_space.shape == (1,)
