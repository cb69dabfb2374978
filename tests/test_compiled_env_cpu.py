"""flow_amd.envs.CompiledEnv without a GPU: the generated header and the cache key of a user environment head
(flow_amd.build.user_env_header / user_tag), the cross-compiled library copy, hipcc's message for a body that does not
compile, every refusal at construction by name, the observation shapes, and the ABI additions (FS_ENV_USER, fs_config.user_env_p)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))

HEAD = dict(obs="o[0] = v / max_speed;\n  o[1] = x / L;", terms="t[0] = v * v;", reward="return fail ? T(0) : sum[0];",
            obs_per_vehicle=2, rl_only=False, reward_terms=1)


def test_abi_has_the_user_head():
    import ctypes
    from flow_amd import _lib
    assert _lib.FS_ENV_USER == 12
    fields = dict(_lib.fs_config._fields_)
    assert fields["user_env_p"] is ctypes.c_double * 8
    assert _lib.fs_config._fields_[-1][0] == "user_env_p"          # appended: every older field keeps its offset
    text = open(os.path.join(ROOT, "include", "flowsim.h")).read()
    assert "FS_ENV_USER = 12" in text and "double user_env_p[8];" in text


def test_header_is_deterministic_and_the_cache_key_follows_every_input():
    from flow_amd import build
    h = build.user_env_header(HEAD)
    assert h == build.user_env_header(dict(HEAD))
    # indentation and surrounding blank lines are not part of the key (the bodies are normalised)
    assert h == build.user_env_header(dict(HEAD, obs="\n\n      o[0] = v / max_speed;\n o[1] = x / L;   \n"))
    for sig in build.USER_ENV_SIGNATURES.values():
        assert sig.split("(")[0] in h
    assert "constexpr int kUserObsPerVehicle = 2;" in h and "constexpr bool kUserObsRlOnly = false;" in h
    assert "constexpr int kUserRewardTerms = 1;" in h
    base = build.user_tag(env=HEAD)
    assert base == build.user_tag(env=dict(HEAD))
    changed = [dict(HEAD, obs=HEAD["obs"] + " o[1] = o[1] + T(1);"), dict(HEAD, terms="t[0] = v;"),
               dict(HEAD, reward="return sum[0];"), dict(HEAD, obs_per_vehicle=3), dict(HEAD, rl_only=True),
               dict(HEAD, reward_terms=2)]
    tags = [build.user_tag(env=c) for c in changed] + [build.user_tag("return T(0);", env=HEAD),
                                                      build.user_tag("return T(1);", env=HEAD)]
    assert len(set(tags + [base])) == len(tags) + 1
    # a controller alone keeps the key it had before there were environment heads
    import hashlib
    assert build.user_tag("return T(0);") == hashlib.sha256(
        (build.user_header("return T(0);") + build._stamp([])).encode()).hexdigest()[:16]
    # without terms neither t nor sum is declared
    h0 = build.user_env_header(dict(HEAD, reward_terms=0, terms="", reward="return T(0);"))
    assert "T* t)" not in h0 and "const T* sum" not in h0
    for bad in (dict(HEAD, obs_per_vehicle=0), dict(HEAD, obs_per_vehicle=9), dict(HEAD, reward_terms=5), dict(HEAD, reward_terms=-1),
                dict(HEAD, obs="  \n"), dict(HEAD, reward=""), dict(HEAD, terms="")):
        with pytest.raises(ValueError, match="user environment head"):
            build.user_env_header(bad)


def test_the_example_heads_compile_and_link_and_a_broken_body_raises_with_the_compiler_s_message():
    """hipcc cross-compiles for gfx950 without a GPU: the two library copies the GPU tests step on, and two bodies that do
    not compile -- a syntax error, and REWARD_TERMS = 0 with `sum` used."""
    from compiled_controller import TimeGap
    from compiled_env import AccelStyleEnv, HighwayStyleEnv, head_source
    from flow_amd import build
    a = build.build_user(env=head_source(AccelStyleEnv))
    b = build.build_user(TimeGap.SOURCE, env=head_source(HighwayStyleEnv))
    assert a != b and os.path.exists(a) and os.path.exists(b)
    assert os.path.dirname(a) == os.path.join(build.USER_DIR, build.user_tag(env=head_source(AccelStyleEnv)))
    assert os.path.exists(os.path.join(os.path.dirname(b), "user_env.h"))
    assert os.path.exists(os.path.join(os.path.dirname(b), "user_controller.h"))
    assert not os.path.exists(os.path.join(os.path.dirname(a), "user_controller.h"))
    with pytest.raises(RuntimeError, match=r"hipcc failed[\s\S]*error:"):
        build.build_user(env=dict(HEAD, obs="o[0] = v / ;"))
    with pytest.raises(RuntimeError, match=r"hipcc failed[\s\S]*undeclared identifier 'sum'"):
        build.build_user(env=dict(HEAD, reward_terms=0, terms=""))


def ring_parts(num_vehicles=14, num_rl=1, lanes=1, sort_vehicles=False, precision="f32"):
    from flow_amd.controllers import ContinuousRouter, IDMController, RLController
    from flow_amd.core.params import EnvParams, InitialConfig, NetParams, SumoParams, VehicleParams
    from flow_amd.networks import RingNetwork
    veh = VehicleParams()
    veh.add("human", acceleration_controller=(IDMController, {}), routing_controller=(ContinuousRouter, {}),
            num_vehicles=num_vehicles - num_rl)
    veh.add("rl", acceleration_controller=(RLController, {}), routing_controller=(ContinuousRouter, {}), num_vehicles=num_rl)
    net = RingNetwork("ring", veh, NetParams(additional_params={"length": 1000 if num_vehicles > 40 else 230, "lanes": lanes,
                                                                "speed_limit": 30, "resolution": 40}),
                      InitialConfig(bunching=20))
    add = {"max_accel": 1, "max_decel": 1, "target_velocity": 10}
    if sort_vehicles:
        add["sort_vehicles"] = True
    return EnvParams(horizon=50, additional_params=add), SumoParams(sim_step=0.1, precision=precision), net


def test_every_refusal_is_raised_at_construction_with_its_name():
    """Before anything is compiled and before a handle exists (no GPU here: a CompiledEnv that got as far as fs_create
    would raise FatalFlowError instead)."""
    from compiled_env import AccelStyleEnv, HighwayStyleEnv
    from flow_amd.controllers import ContinuousRouter, IDMController, RLController
    from flow_amd.core.params import EnvParams, InFlows, InitialConfig, NetParams, SumoParams, VehicleParams
    from flow_amd.envs import CompiledEnv
    from flow_amd.networks import MergeNetwork, MultiRingNetwork

    with pytest.raises(NotImplementedError, match="multi-lane rings"):
        HighwayStyleEnv(*ring_parts(lanes=2))
    with pytest.raises(NotImplementedError, match="sort_vehicles"):
        HighwayStyleEnv(*ring_parts(sort_vehicles=True))
    with pytest.raises(NotImplementedError, match="more than 64 vehicles"):
        HighwayStyleEnv(*ring_parts(num_vehicles=65))
    for prec in ("mixed", "f16s"):
        with pytest.raises(NotImplementedError, match="precisions f32 and f64"):
            HighwayStyleEnv(*ring_parts(precision=prec))

    # an open network
    veh = VehicleParams()
    veh.add("human", acceleration_controller=(IDMController, {}), num_vehicles=3)
    veh.add("rl", acceleration_controller=(RLController, {}), num_vehicles=1)
    from flow_amd.networks.merge import ADDITIONAL_NET_PARAMS as MERGE_PARAMS
    inflow = InFlows()
    inflow.add(veh_type="human", edge="inflow_highway", vehs_per_hour=1000, departLane="free", departSpeed=10)
    merge = MergeNetwork("merge", veh, NetParams(inflows=inflow, additional_params=dict(MERGE_PARAMS)), InitialConfig())
    env_params, sim_params, _ = ring_parts()
    with pytest.raises(NotImplementedError, match="open networks"):
        HighwayStyleEnv(env_params, sim_params, merge)

    # MultiRingNetwork
    veh = VehicleParams()
    for g in range(2):
        veh.add("human_%d" % g, acceleration_controller=(IDMController, {}), routing_controller=(ContinuousRouter, {}),
                num_vehicles=4)
        veh.add("rl_%d" % g, acceleration_controller=(RLController, {}), routing_controller=(ContinuousRouter, {}), num_vehicles=1)
    rings = MultiRingNetwork("rings", veh, NetParams(additional_params={"length": 230, "lanes": 1, "speed_limit": 30,
                                                                        "resolution": 40, "num_rings": 2}),
                             InitialConfig(bunching=20, spacing="custom"))
    with pytest.raises(NotImplementedError, match="MultiRingNetwork"):
        HighwayStyleEnv(env_params, sim_params, rings)

    # the head itself: shapes, parameters, sources
    def head(**attrs):
        cls = type("Head", (AccelStyleEnv,), attrs)
        init = attrs.pop("params", None)
        if init is not None:
            cls.__init__ = lambda self, *a: CompiledEnv.__init__(self, *a, params=init)
        return cls
    for attrs, name in ((dict(OBS_PER_VEHICLE=0), "OBS_PER_VEHICLE"), (dict(OBS_PER_VEHICLE=9), "OBS_PER_VEHICLE"),
                        (dict(REWARD_TERMS=5), "REWARD_TERMS"), (dict(REWARD_TERMS=-1), "REWARD_TERMS"),
                        (dict(params=list(range(9))), "params"), (dict(OBS_SOURCE="  \n "), "OBS_SOURCE"),
                        (dict(TERM_SOURCE=None), "TERM_SOURCE"), (dict(REWARD_SOURCE=""), "REWARD_SOURCE"),
                        (dict(OBSERVE="humans"), "OBSERVE")):
        with pytest.raises(ValueError, match=name):
            head(**attrs)(*ring_parts())


def test_observation_shapes_of_the_two_layouts():
    """obs_dim = 5 * num_rl ("rl") and 2 * N ("all"): what the class says before a handle exists (the handle's own
    fs_obs_dim is compared with it in tests/test_compiled_env_gpu.py)."""
    from compiled_env import AccelStyleEnv, HighwayStyleEnv, head_source
    assert HighwayStyleEnv.head_obs_dim(num_vehicles=22, num_rl=2) == 10
    assert HighwayStyleEnv.head_obs_dim(num_vehicles=22, num_rl=3) == 15
    assert AccelStyleEnv.head_obs_dim(num_vehicles=14, num_rl=1) == 28
    assert AccelStyleEnv.head_obs_dim(num_vehicles=7, num_rl=0) == 14
    assert head_source(HighwayStyleEnv)["rl_only"] and not head_source(AccelStyleEnv)["rl_only"]


def test_the_stock_library_refuses_a_user_head_before_it_touches_a_device():
    """fs_create validates the whole config first: env = 12 on the stock library is FS_ERR_UNSUPPORTED with the names of
    the head and of the class that brings one, with or without a GPU."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import idm_vehicle, ring_spec
    from flow_amd import _lib as L
    from flow_amd.sim import FlowSim
    spec = ring_spec(R=2, N=5, bunching=0, env=L.FS_ENV_USER, num_rl=1,
                     vehicles=[idm_vehicle()] * 4 + [idm_vehicle(controller=1, rl_index=0)])
    with pytest.raises(NotImplementedError, match=r"FS_ENV_USER[\s\S]*flow_amd\.envs\.CompiledEnv"):
        FlowSim(spec, "f32")
    with pytest.raises(ValueError, match="bad env"):
        FlowSim(dict(spec, env=13), "f32")
