"""The fast / slow rule of the hand-written FS_MIXED pair step (flow_amd/csrc/flowsim_pair.h: mixed_step_asm_b /
mixed_step_asm_slow), restated in numpy and held to the kernel's C twin step for step.

The kernel's common step carries no wrap selects: positions are left as x + v dt, the two gaps of a lane get a per-lane
addend W in {0.0, L} instead of the select `d < 0 ? d + L : d`, and the controller reads the headways unclamped.  A wave
(four consecutive replicas on 16-lane rows) redoes the step's tail in the full form when any of its lanes raises the
predicate; the full form also refreshes W from the real compare and clamps the headways in place.  `FastSlowModel` below
is that rule on float64 / float32 numpy arrays, one IEEE operation per kernel instruction; CRingIDMMixed is the bit-twin
of what the kernel computed before the rule existed.  Equality of positions, speeds, observations and dones on
  (a) the headline configuration (cars wrap),
  (b) the fuzz generator of tests/test_pair_gpu.py (per-slot parameters and lengths, speed modes, collisions),
  (c) rings so short that every step has a wrap,
  (d) addends made stale on purpose (no reachable trajectory has them: the guard is only testable here)
is the statement "no false negative".  (a) also pins the premise that makes the rule pay: few waves take the slow form.
"""
import numpy as np
import pytest

from helpers import idm_vehicle, ring_spec
from oracle import cbuild

f32, f64 = np.float32, np.float64
C1E3 = f32(1e-3)
C1E3_BITS = int(C1E3.view(np.uint32))                    # 0x3A83126F
THR_CAP = 0x457CED91                                     # 0x80000000 - C1E3_BITS: see flowsim_pair.h


def hi32(a):
    return (np.ascontiguousarray(a, f64).view(np.uint64) >> np.uint64(32)).astype(np.uint32)


class FastSlowModel:
    """numpy restatement of k_rollout_pair<double, 16, ...> with the hand-written step: state [R, N], one wave = `rpw`
    consecutive replicas.  `slow_groups` / `groups` count the wave-steps that took the slow form / all of them."""

    def __init__(self, spec, rpw=4):
        R, N = int(spec["num_replicas"]), int(spec["num_vehicles"])
        assert N % 2 == 0
        self.R, self.N, self.rpw = R, N, rpw
        veh = spec["vehicles"]
        p = np.array([list(v["p"][:6]) for v in veh], f64).T
        self.v0, self.T, self.a, self.b, self.delta, self.s0 = (p[q].astype(f32) for q in range(6))
        assert (self.delta == 4).all()
        self.tsab = f32(2.0) * np.sqrt(self.a * self.b)
        self.len_lead = np.roll(np.array([v.get("length", 5.0) for v in veh], f64), -1)       # length of the leader
        self.mode = np.array([int(v.get("speed_mode", 0)) & 7 for v in veh])
        self.sm = bool(self.mode.any())
        self.tau, self.min_gap, self.smax, self.ma, self.md = (
            np.array([v.get(k, d) for v in veh], f64) for k, d in
            (("sumo_tau", 1.0), ("sumo_min_gap", 2.5), ("sumo_max_speed", 30.0), ("max_accel", 2.6), ("max_decel", 4.5)))
        self.dt = float(spec["sim_step"])
        self.ramp = float(spec.get("slowdown_ramp", self.dt / (self.dt + 1e-3)))
        self.L = (np.broadcast_to(np.asarray(spec["ring_length"], f64), (R,)) + 4.0 * float(spec.get("junction_length", 0.1)))[:, None]
        self.rc_L, self.rc_ms = 1.0 / self.L, 1.0 / float(spec["max_speed"])
        self.thr = np.minimum(hi32(self.L), np.uint32(THR_CAP))
        self.gap = f32(spec.get("crash_gap", 0.0))
        self.step_limit = int(spec.get("warmup_steps", 0) + spec["horizon"])
        self.x = np.asarray(spec["init_pos"], f64).reshape(R, N).copy()
        iv = spec.get("init_vel")
        self.v = np.zeros((R, N)) if iv is None else np.asarray(iv, f64).reshape(R, N).copy()
        self.tc = np.zeros(R, np.int32)
        self.groups = self.slow_groups = 0
        self.prologue()

    # ---- the full form of the step's tail (today's selects): also what a launch's prologue does
    def full_tail(self, x_new, wrap):
        L = self.L
        x = np.where(np.signbit(x_new - L), x_new, x_new - L) if wrap else x_new
        d = np.roll(x, -1, axis=1) - x
        neg = np.signbit(d)
        W = np.where(neg, L, 0.0)
        d = np.where(neg, d + L, d)
        h = (d - self.len_lead).astype(f32)
        ct = np.fmin(h[:, 0::2] - self.gap, h[:, 1::2] - self.gap)
        H = np.where(~(np.abs(h) < C1E3), h, C1E3)
        return x, W, h, H, ct

    def prologue(self):
        _, self.W, _, self.H, _ = self.full_tail(self.x, wrap=False)

    def controller(self):
        """v' in float64 from the float32 controller on (float32 images of v, H)"""
        one = f32(1.0)
        vi = self.v.astype(f32)
        dvl = vi - np.roll(vi, -1, axis=1)
        num = vi * dvl
        dyn = vi * self.T + num / self.tsab
        s_star = self.s0 + np.maximum(dyn, f32(0))
        q = s_star / self.H
        r = vi / self.v0
        r2 = r * r
        acc = self.a * (one - r2 * r2 - q * q)
        nv = np.maximum(self.v + acc.astype(f64) * self.dt, 0.0)
        vc = self.v + (nv - self.v) * self.ramp
        if self.sm:
            G = np.maximum(self.H, C1E3)
            ts = f32(2.0) * np.sqrt(self.ma.astype(f32) * self.md.astype(f32))
            dyn_s = vi * self.tau.astype(f32) + num / ts
            ss = self.min_gap.astype(f32) + np.maximum(f32(0), dyn_s)
            qs = ss / G
            rs = vi / self.smax.astype(f32)
            rs2 = rs * rs
            acc_s = self.ma.astype(f32) * (one - rs2 * rs2 - qs * qs)
            vs = np.maximum(self.v + acc_s.astype(f64) * self.dt, 0.0)
            vc = np.where((self.mode & 1) != 0, np.minimum(vc, vs), vc)
            vc = np.where((self.mode & 2) != 0, np.minimum(vc, self.v + self.ma * self.dt), vc)
            vc = np.where((self.mode & 4) != 0, np.maximum(vc, self.v - self.md * self.dt), vc)
        return vc

    def step(self):
        """One env step; returns (obs [R, 2N] float32, done [R] bool, need [groups] bool)."""
        R, N = self.R, self.N
        self.v = self.controller()
        x_new = self.x + self.v * self.dt
        # ---- fast tail
        d1 = (np.roll(x_new, -1, axis=1) - x_new) + self.W
        h = (d1 - self.len_lead).astype(f32)
        m = np.fmin(h[:, 0::2], h[:, 1::2])                                                   # v_min_f32 of a lane's pair
        um = (m.view(np.uint32).astype(np.int64) - C1E3_BITS) % (1 << 32)
        u = np.maximum(np.maximum(hi32(x_new), hi32(d1)).reshape(R, N // 2, 2).max(axis=2).astype(np.int64), um)
        lane_need = u >= self.thr.astype(np.int64)
        G = -(-R // self.rpw)
        need = np.array([lane_need[g * self.rpw:(g + 1) * self.rpw].any() for g in range(G)])
        rows = np.repeat(need, self.rpw)[:R][:, None]
        # ---- slow tail for the waves that need it
        xs, Ws, _, Hs, cts = self.full_tail(x_new, wrap=True)
        self.x = np.where(rows, xs, x_new)
        self.W = np.where(rows, Ws, self.W)
        self.H = np.where(rows, Hs, h)
        ct = np.where(rows, cts, m - self.gap)
        self.groups += G
        self.slow_groups += int(need.sum())
        self.tc += 1
        obs = np.concatenate([(self.v * self.rc_ms).astype(f32), (self.x * self.rc_L).astype(f32)], axis=1)
        done = (self.tc >= self.step_limit) | np.signbit(ct).any(axis=1)
        return obs, done, need


def run_against_twin(spec, K, model=None, on_step=None):
    twin = cbuild.CRingIDMMixed(spec)
    model = model or FastSlowModel(spec)
    np.testing.assert_array_equal(model.x, twin.x)
    for k in range(K):
        if on_step is not None:
            on_step(k, model)
        o, d, need = model.step()
        to, _, td = twin.rollout(1, obs_every_step=True)
        np.testing.assert_array_equal(model.x, twin.x, err_msg="pos step %d" % k)
        np.testing.assert_array_equal(model.v, twin.v, err_msg="vel step %d" % k)
        np.testing.assert_array_equal(o, to[0], err_msg="obs step %d" % k)
        np.testing.assert_array_equal(d, td[0], err_msg="done step %d" % k)
    np.testing.assert_array_equal(model.tc, twin.tc)
    return model


def c2(R):
    from bench import c2_spec
    return c2_spec(R, seed=1000)


def fuzz_spec(seed):
    """the generator of tests/test_pair_gpu.py::test_pair_hand_written_steps_fuzz_f32_and_mixed (same draws, same order)"""
    rng = np.random.default_rng(seed)
    N = int(rng.choice([18, 20, 22, 24, 28, 32]))
    R = 9
    with_modes = seed % 2 == 0
    veh = []
    for i in range(N):
        veh.append(idm_vehicle(
            p=[float(rng.uniform(15, 35)), float(rng.uniform(0.6, 1.6)), float(rng.uniform(0.6, 2.5)),
               float(rng.uniform(0.8, 3.0)), 4, float(rng.uniform(0.5, 3.0)), 0, 0],
            length=float(rng.choice([3.5, 5.0, 7.0])),
            speed_mode=int(rng.choice([0, 1, 7, 25, 31, 6])) if with_modes else 0,
            max_accel=float(rng.uniform(0.8, 3.0)), max_decel=float(rng.uniform(1.0, 7.5)),
            sumo_tau=float(rng.uniform(0.4, 1.5)), sumo_min_gap=float(rng.uniform(0.2, 3.0)),
            sumo_max_speed=float(rng.uniform(6.0, 35.0))))
    L = float(rng.uniform(8.5, 14.0)) * N
    spec = ring_spec(R=R, N=N, length=L, bunching=0, junction_length=0.1, horizon=60, vehicles=veh)
    prng = np.random.default_rng(seed)
    spec["init_pos"] = np.asarray(spec["init_pos"]) + np.abs(prng.normal(0, 0.3, (R, N)))
    spec["init_vel"] = rng.uniform(0, 12, (R, N))
    return spec


def test_c2_cars_wrap_and_few_waves_take_the_slow_step():
    K = 600
    model = run_against_twin(c2(8), K)
    share = model.slow_groups / model.groups
    print("slow share of wave-steps: %.4f (%d of %d)" % (share, model.slow_groups, model.groups))
    assert model.slow_groups > 0, "no car wrapped: the case does not exercise the slow step"
    # the premise of the design (measured with the twin: 8.4 % at R = 512 over 1500 steps)
    assert share < 0.15, share


@pytest.mark.parametrize("seed", [11, 12, 13, 14, 15, 16])
def test_fuzz_generator_with_speed_modes_and_collisions(seed):
    run_against_twin(fuzz_spec(seed), 70)


def test_fuzz_cases_contain_collisions_and_clamped_headways():
    crashed = clamped = False
    for seed in (11, 12, 13, 14, 15, 16):
        spec = fuzz_spec(seed)
        model = FastSlowModel(spec)
        for k in range(70):
            _, d, _ = model.step()
            crashed = crashed or bool(d.any() and k < 59)
            clamped = clamped or bool((model.H == C1E3).any())
    assert crashed, "the fuzz cases are meant to contain collisions"
    print("a headway was clamped:", clamped)


def test_short_ring_wraps_in_every_step():
    # six short vehicles with a tight controller (T = 0.1 s, s0 = 0.2 m) on a 12.4 m ring run near 13 m/s at a spacing of
    # s = 2.07 m.  The four replicas of a wave start s / 4 apart in phase, so the wave sees a vehicle pass the seam every
    # s / (4 v) seconds: in every step while v > s / (4 dt) = 5.2 m/s.  Asked for: 0.9 of the wave-steps (the spacing is
    # not exactly even: +- 0.05 m of jitter, and the platoon breathes)
    R, N, K = 8, 6, 200
    rng = np.random.default_rng(3)
    veh = [idm_vehicle(p=[30, 0.1, 1.0, 3.0, 4, 0.2, 0, 0], length=0.5) for _ in range(N)]     # (a < b: a steady platoon)
    spec = ring_spec(R=R, N=N, length=60.0, bunching=0, junction_length=0.1, horizon=10 ** 6, vehicles=veh)
    spec["ring_length"] = np.full(R, 12.0)                 # (the start-position helper places 5 m vehicles: set by hand)
    spec["init_pos"] = np.arange(N) * (12.4 / N) + (np.arange(R) % 4)[:, None] * (12.4 / N / 4) + rng.uniform(0, 0.05, (R, N))
    spec["init_vel"] = rng.uniform(11, 13, (R, N))
    model = run_against_twin(spec, K)
    print("slow share of wave-steps: %d of %d" % (model.slow_groups, model.groups))
    assert model.slow_groups > 0.9 * model.groups, (model.slow_groups, model.groups)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_stale_addends_raise_the_predicate_in_the_same_step(seed):
    """W made wrong on purpose (0 <-> L for a random subset of one replica's vehicles) right before a random step: the
    wave of that replica must take the slow step in that very step, and the trajectory must not change."""
    rng = np.random.default_rng(100 + seed)
    spec = c2(8)
    K = 120
    at = int(rng.integers(5, K - 5))
    r = int(rng.integers(0, 8))
    fired = {}

    def inject(k, model):
        if k == at:
            pick = rng.random(model.N) < 0.3
            pick[int(rng.integers(0, model.N))] = True
            L = model.L[r, 0]
            model.W[r] = np.where(pick, np.where(model.W[r] == 0.0, L, 0.0), model.W[r])
            fired["before"] = model.slow_groups

    class Probe(FastSlowModel):
        def step(self):
            o, d, need = super().step()
            if self.tc[0] == at + 1:
                fired["need"] = bool(need[r // self.rpw])
            return o, d, need

    model = run_against_twin(spec, K, model=Probe(spec), on_step=inject)
    assert fired["need"], "stale addends went unnoticed"
    # the slow step rebuilt them: they agree with the sign of the raw gaps again
    d = np.roll(model.x, -1, axis=1) - model.x
    np.testing.assert_array_equal(model.W, np.where(d < 0, model.L, 0.0))
