"""Reference side of the multi-ring tests (not a test file): MultiWaveAttenuationPOEnv on MultiRingNetwork
(flow/envs/multiagent/ring/wave_attenuation.py:34-140, flow/networks/multi_ring.py).

* ``MultiRingOracle``: oracle.refsim.RingOracle with one ring per replica row; observation and crash handling are
  ENV_WAVE_ATTENUATION_PO_MA's (one column), ``compute_reward`` is the reference's, vectorised over the rows.
* ``literal_reward`` / ``literal_start_positions``: the reference's ``compute_reward`` (for one agent) and
  ``gen_custom_start_pos`` restated statement by statement in plain float64 Python, per vehicle."""
import math

import numpy as np

from helpers import idm_vehicle, ring_spec
from oracle import refsim as S
from oracle import rewards as Rw

ENV_MULTI_WAVE_ATTENUATION_PO = 11          # include/flowsim.h FS_ENV_MULTI_WAVE_ATTENUATION_PO


def max_cost_table(target, n_max, dtype):
    """np.linalg.norm([target] * n) for n = 0 .. n_max, float64 on the host, rounded to ``dtype``."""
    return np.array([np.linalg.norm(np.array([target] * n, dtype=np.float64)) for n in range(n_max + 1)]).astype(dtype)


class MultiRingOracle(S.RingOracle):
    """``spec['env']`` is ENV_MULTI_WAVE_ATTENUATION_PO; every row is one ring with its one RL vehicle."""

    def __init__(self, spec, dtype=np.float64):
        assert int(spec["env"]) == ENV_MULTI_WAVE_ATTENUATION_PO and int(spec["num_rl"]) == 1
        super().__init__(dict(spec, env=S.ENV_WAVE_ATTENUATION_PO_MA), dtype)
        self.target = float(spec["target_velocity"])
        self.max_cost = max_cost_table(self.target, self.N, self.dt_)
        self.seen_n = set()                 # every number of on-edge vehicles a rewarded step has seen
        self.last_n = None

    def on_edge(self):
        """vehs_on_edge: get_ids_by_edge(['top_g', 'left_g', 'right_g', 'bottom_g']) never lists a vehicle whose front is
        on an internal edge -- whatever junction_mode says."""
        return ~self.in_junction(self.x)

    def compute_reward(self, actions, fail):
        T = self.dt_.type
        if actions is None:                                          # the warm-up steps (:103-105)
            return np.zeros(self.R, dtype=self.dt_)
        on = self.on_edge()
        n = on.sum(axis=1)
        self.last_n = n
        self.seen_n.update(int(k) for k in n)
        d = np.where(on, self.v - T(self.target), T(0))              # :123
        cost = np.sqrt(Rw.tree_sum(d * d))                           # :124 (the kernels' summation order)
        mc = self.max_cost[n]                                        # :120-121
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.maximum(mc - cost, T(0)) / mc                     # :126 -- no epsilon: n = 0 gives 0 / 0
        bad = np.any(on & (self.v < T(-100)), axis=1)                # :116 (fail = crash = 0 in this fork's MultiEnv)
        return np.where(bad, T(0), r)


def literal_reward(x, v, ring_length, junction_length, target, have_actions=True):
    """compute_reward of the agent of ONE ring, per vehicle: ``x`` / ``v`` the ring's loop coordinates and speeds."""
    if not have_actions:
        return 0.0
    quarter = ring_length / 4
    q = quarter + junction_length
    vel = []
    for xi, vi in zip(x, v):
        u = xi - math.floor(xi / q) * q
        if u >= quarter:                      # front on ':right_g_0' ...: on none of the four edges
            continue
        vel.append(float(vi))
    vel = np.array(vel, dtype=np.float64)
    if any(vel < -100):
        return 0.
    max_cost = np.array([target] * len(vel), dtype=np.float64)
    max_cost = np.linalg.norm(max_cost)
    cost = vel - target
    cost = np.linalg.norm(cost)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.float64(max(max_cost - cost, 0)) / np.float64(max_cost))


VEHICLE_LENGTH = 5
RING_EDGES = ("bottom", "right", "top", "left")


def literal_start_positions(num_rings, per_ring, bunching, length=230, min_gap=0, x0=0, lanes_distribution=1):
    """gen_custom_start_pos (multi_ring.py:92-148) on one-lane rings: [(edge, position)] of the vehicles in id order."""
    num_vehicles = num_rings * per_ring
    edgelen = length / 4
    shift = 4 * edgelen
    edgestarts = []
    for i in range(num_rings):
        edgestarts += [("bottom_{}".format(i), 0 + i * shift), ("right_{}".format(i), edgelen + i * shift),
                       ("top_{}".format(i), 2 * edgelen + i * shift), ("left_{}".format(i), 3 * edgelen + i * shift)]

    def get_edge(x):
        for (edge, start_pos) in reversed(edgestarts):
            if x >= start_pos:
                return edge, x - start_pos

    # _get_start_pos_util (kernel/network/base.py:515-608)
    distribution_length = sum(edgelen * min(1, lanes_distribution) for _ in edgestarts if edgelen > min_gap + VEHICLE_LENGTH)
    available_length = distribution_length - lanes_distribution * bunching - num_vehicles * (min_gap + VEHICLE_LENGTH)
    increment = available_length / num_vehicles
    vehs_per_ring = num_vehicles / num_rings
    x = x0
    car_count = 0
    startpositions = []
    while car_count < num_vehicles:
        pos = get_edge(x)
        car_count += 1
        startpositions.append(pos)
        edge, pos = startpositions[-1]
        startpositions[-1] = edge, pos % length
        x = (x + increment + VEHICLE_LENGTH + min_gap) + 1e-13
        if (car_count % vehs_per_ring) == 0:
            ring_num = int(car_count / vehs_per_ring)
            x = length * ring_num + 1e-13
    return startpositions


def loop_coordinate(edge, position, length=230, junction_length=0.1):
    """(ring, coordinate on the ring's loop: four edges, a junction after each) of a start position."""
    name, ring = edge.split('_')
    return int(ring), RING_EDGES.index(name) * (0.25 * length + junction_length) + position


def multi_ring_spec(R=5, N=22, length=230.0, noise=0.2, warmup=0, horizon=400, target=4.0, seed=0, jitter=0.3,
                    speed_mode=25, **kw):
    """A handle of R rows, one ring each: N - 1 IDM humans and the RL vehicle last (lord_of_the_rings' slot order), the
    rows' start positions moved apart by ``jitter`` so that no two rows are alike."""
    rng = np.random.default_rng(seed)
    spec = ring_spec(R=R, N=N, length=length, bunching=20.0 if N * 7.5 < length else 0.0, junction_length=0.1,
                     horizon=horizon, env=ENV_MULTI_WAVE_ATTENUATION_PO, num_rl=1, action_low=-1.0, action_high=1.0,
                     po_max_length=length, warmup_steps=warmup, clip_actions=False, seed=4321 + seed, target_velocity=target)
    spec["init_pos"] = np.asarray(spec["init_pos"]) + np.abs(rng.normal(0, jitter, (R, N)))
    spec["vehicles"] = [idm_vehicle(noise=noise, speed_mode=speed_mode) for _ in range(N - 1)] + \
                       [idm_vehicle(controller=S.CTRL_RL, rl_index=0, speed_mode=speed_mode)]
    spec.update(kw)
    return spec
