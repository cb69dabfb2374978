"""`k_drop_queue` (flow_amd/csrc/flowsim_dropq.h) at its edges, against the float32 oracle (oracle/opennet.py, cell_sum =
'fixed') bit for bit through the C ABI: a path of exactly 64 vehicles, the refused 65th, several arrivals in one sub-step,
counts that move by more than the four-entry window of count_near3 holds, equal positions across paths, the hand-over
between the queue-order and the slot-order kernel on one handle, launch fragments of odd lengths, and pinned fuzz seeds.

Every test also asserts, on the ORACLE's side, that the event it is named for happened (`Watch`): a configuration that
stops reaching its edge fails instead of passing.  Those are conditions on the inputs, not tolerances."""
import numpy as np
import pytest

from conftest import seeds

from helpers import bottleneck_layout, bottleneck_spec
from oracle import opennet as O
from test_dropq_gpu import actions, run
from test_open_gpu import compare_state, compare_vmax, make

pytestmark = pytest.mark.gpu

PATH_LANES = 64                      # a wave holds a path: flowsim_dropq.h


class Watch:
    """Event counts of an oracle run (run(..., watch=Watch())): most vehicles on one path, most arrivals of one gym step and
    of one sub-step (the oracle's ring buffer of arrivals per sub-step), steps with a collision before the horizon,
    equal-position pairs of vehicles on different paths, and -- for sims_per_step = 1, where a gym step is one sub-step --
    `path_burst` = most vehicles of ONE path that arrived in a sub-step, `passed` = most other-path vehicles one vehicle
    passed or was passed by in a sub-step, `count_jump` = largest change of "vehicles of path q ahead of me" among vehicles
    that stayed (what count_near3's window, old count - 2 .. + 1, has to hold), `used_jump` = the same where the vehicle
    looks across the join with path q, so that the count picks its leader candidate there."""

    def __init__(self, passing=False):
        self.passing = passing
        self.on_path = []                # per call: [R, 4] vehicles per path
        self.burst = self.sub_burst = self.path_burst = self.crash_steps = self.ties = self.passed = 0
        self.count_jump = self.used_jump = 0
        self.prev = None

    def __call__(self, k, ora, done):
        alive, route, x = ora.alive, ora.route, ora.x
        sps = int(ora.spec["sims_per_step"])
        self.on_path.append(np.stack([(route == p).sum(axis=1) for p in range(4)], axis=1))
        ahead = None
        if self.passing:
            jj = np.arange(ora.N)
            ahead = (x[:, None, :] > x[:, :, None]) | ((x[:, None, :] == x[:, :, None]) & (jj[None, None, :] < jj[None, :, None]))
        if k >= 0:
            r0, o0, arrived0, ah0 = self.prev
            self.burst = max(self.burst, int((ora.total_arrived - arrived0).max()))
            rows = np.arange(ora.R)
            for j in range(sps):
                self.sub_burst = max(self.sub_burst, int(ora.arr_hist[rows, (ora.time_counter - 1 - j) % 20].max()))
            self.crash_steps += int((done & (ora.time_counter < sps * (int(ora.spec.get("warmup_steps", 0)) +
                                                                        int(ora.spec["horizon"])))).sum())
            if sps == 1:
                gone = (r0 >= 0) & ((route < 0) | (o0 != ora.origin))
                self.path_burst = max(self.path_burst, max(int((gone & (r0 == p)).sum(axis=1).max()) for p in range(4)))
            if self.passing and sps == 1:
                stay = (r0 >= 0) & alive & (o0 == ora.origin)
                both = stay[:, :, None] & stay[:, None, :] & (route[:, :, None] != route[:, None, :])
                self.passed = max(self.passed, int((both & (ahead != ah0)).sum(axis=2).max()))
                look = ora.shift(x + ora.zip_d)                          # joins I look across (M8)
                for p in range(4):
                    on_p = both & (route == p)[:, None, :]
                    jump = np.abs((on_p & ahead).sum(axis=2) - (on_p & ah0).sum(axis=2))
                    self.count_jump = max(self.count_jump, int(jump.max()))
                    used = np.where((route ^ 1) == p, look >= 1, look == 2)   # the count picks my candidate on path p
                    self.used_jump = max(self.used_jump, int(np.where(used, jump, 0).max()))
        pair = alive[:, :, None] & alive[:, None, :] & (route[:, :, None] != route[:, None, :])
        self.ties += int((pair & (x[:, :, None] == x[:, None, :])).sum()) // 2
        self.prev = (route.copy(), ora.origin.copy(), ora.total_arrived.copy(), ahead)

    @property
    def most_on_a_path(self):
        return int(np.max(self.on_path))


def fixed_lane_inflows(spec, lanes_and_periods):
    """Inflows on fixed entry lanes: [(vehicle type, entry lane, period in s)], begin 1 s."""
    human, rl = spec["inflows"][0], spec["inflows"][1]
    return [dict(rl if typ else human, route=lane, period=float(period)) for typ, lane, period in lanes_and_periods]


# ------------------------------------------------------------------ 1 / 2: a path at its 64 lanes
def full_path_spec(n0, head, inflows, horizon=200, seed=31):
    """Path 0: n0 humans at rest, 8.5 m apart, the first `head` m before the end of the network (slots 0 .. n0 - 1).
    Path 1: three humans behind the whole of path 0, inside the 120 m zipper zone of the first join: their leader is found by
    the count "all of path 0 is ahead".  Path 2: a human level with path 1's first and one level with path 0's 41st vehicle.
    Path 3: RL vehicles level with path 1's second and with path 0's 11th vehicle (beyond the second join: one physical
    lane) -- equal positions across paths, where they decide leaders."""
    R, cap_human, cap_rl = 2, 150, 10
    at = lambda i: head + 8.5 * i                                       # noqa: E731
    tail = at(n0 - 1)
    lay = {i: (at(i), 0.0, 0) for i in range(n0)}
    lay.update({64: (tail + 9.0, 0.0, 1), 65: (tail + 20.0, 0.0, 1), 66: (tail + 31.0, 0.0, 1),
                67: (tail + 9.0, 0.0, 2), 68: (at(40), 0.0, 2),
                cap_human: (tail + 20.0, 0.0, 3), cap_human + 1: (at(10), 0.0, 3)})
    spec = bottleneck_spec(R=R, cap_human=cap_human, cap_rl=cap_rl, zipper_distance=120.0, horizon=horizon, seed=seed,
                           **bottleneck_layout(R, cap_human + cap_rl, lay))
    spec["inflows"] = fixed_lane_inflows(spec, inflows)
    return spec


def test_drop_queue_a_path_of_exactly_64_vehicles():
    """Oracle side (asserted below): path 0 holds 64 at the start and for the first steps, no path ever holds more; equal
    positions across paths occur; vehicles arrive.  Reaches the `rank < 64` build with rank 63, count_ahead3's "a full path
    whose 64 vehicles are all ahead is one more" (path 1's vehicles), count_near3's window clamp at 60."""
    spec = full_path_spec(64, 8.0, [(0, 1, 3.0), (0, 2, 4.0), (1, 3, 5.0)])
    w = Watch()
    ora = run(spec, 120, actions(spec, 3, -1.5, 1.5), check_every=4, watch=w)
    on_path = np.array(w.on_path)                                        # [step + 1, R, 4]
    assert (on_path[0, :, 0] == PATH_LANES).all() and w.most_on_a_path == PATH_LANES
    assert (on_path[:4, :, 0] == PATH_LANES).all()                       # (measured: the first 4 steps of each replica)
    assert w.ties >= 10 and ora.total_arrived.min() >= 15 and ora.total_departed.min() >= 20


def test_drop_queue_accepts_the_64th_vehicle_and_refuses_the_65th_at_the_oracles_step():
    """63 vehicles on path 0, the head 60 m before the end (nothing arrives in the first dozen steps), one inflow on entry
    lane 0 every second: the oracle says when the 64th and the 65th vehicle are inserted (M3's gap rule delays the second);
    every step before the 65th equals the oracle bit for bit, the step of the 65th raises, and the handle stays unusable."""
    spec = full_path_spec(63, 60.0, [(0, 0, 1.0)])
    ora = O.MergeOracle(dict(spec, cell_sum="fixed"), np.float32)
    sim = make(spec, "f32")
    np.testing.assert_array_equal(sim.reset(), ora.reset().astype(np.float32))
    compare_state(sim, ora)
    act = actions(spec, 5, -1.5, 1.5)
    on0 = lambda: (ora.route == 0).sum(axis=1)                           # noqa: E731
    assert (on0() == 63).all()
    k64 = k65 = raised_at = -1
    for k in range(16):
        a = act(k)
        o_ref, r_ref, d_ref = ora.step(a)
        if k64 < 0 and on0().max() == 64:
            k64 = k
        if on0().max() == 65:
            k65 = k
        try:
            o_gpu, r_gpu, d_gpu = sim.step(a)
        except NotImplementedError as e:
            assert "k_drop_queue" in str(e) and "FLOWSIM_NO_QUEUE" in str(e)
            raised_at = k
            break
        assert sim.last_kernel == "k_drop_queue" and k65 < 0, "the kernel took the oracle's step %d of the 65th vehicle" % k65
        np.testing.assert_array_equal(o_gpu, o_ref.astype(np.float32), err_msg="obs, step %d" % k)
        np.testing.assert_array_equal(r_gpu, r_ref.astype(np.float32), err_msg="reward, step %d" % k)
        np.testing.assert_array_equal(d_gpu, d_ref, err_msg="done, step %d" % k)
        compare_state(sim, ora)
    assert 0 <= k64 < k65 and k65 - k64 >= 2                             # the oracle's steps (measured: 1 and 4)
    assert ora.total_arrived.max() == 0                                  # nobody left: the 65 are 63 + two insertions
    assert raised_at == k65
    with pytest.raises(NotImplementedError, match="k_drop_queue"):
        sim.pos                                          # (sticky: the handle stays unusable)
    sim.close()


# ------------------------------------------------------------------ 3: several arrivals in one sub-step
# slot -> (m before the end, m/s, path); slots 40, 41 are RL vehicles
BURST_TWO_PATHS = {0: (1.0, 20.0, 0), 1: (32.0, 16.0, 1), 40: (70.0, 18.0, 1), 2: (110.0, 18.0, 3), 41: (150.0, 18.0, 2)}
# the head of path 0 and its follower 26 m behind (21 m gap, 16 m/s: SUMO's model still accelerates it to 19 m/s) both pass
# the end in the first 2 s: na = 2 inside ONE wave
BURST_ONE_PATH = {0: (1.0, 20.0, 0), 1: (27.0, 16.0, 0), 2: (55.0, 16.0, 1), 40: (85.0, 18.0, 1), 3: (115.0, 18.0, 3),
                  41: (150.0, 18.0, 2)}


def burst_spec(layout, sims_per_step=1, sim_step=2.0):
    return bottleneck_spec(R=2, cap_human=40, cap_rl=8, sim_step=sim_step, sims_per_step=sims_per_step, horizon=50, seed=17,
                           **bottleneck_layout(2, 48, layout))


@pytest.mark.parametrize("sims_per_step", [1, 2])
@pytest.mark.parametrize("layout", ["two_paths", "one_path"])
def test_drop_queue_several_arrivals_in_one_sub_step(layout, sims_per_step):
    """sim_step = 2 s.  'two_paths': the heads of paths 0 and 1 pass the end of the network in the first sub-step (several
    arr_lab entries, slot-free masks with several bits, hist_l / the outflow sums with a burst), RL vehicles (slots 40, 41)
    arrive later.  'one_path': two vehicles of path 0 arrive in the first sub-step (`n -= na; gather_all(l + na, ..)` with
    na = 2).  Oracle side: two arrivals in one sub-step (of one path: counted with one sub-step per step; the first sub-step
    is the same with two), RL arrivals, no collision.  With sim_step = 1 s either layout gives at most one arrival."""
    lay = BURST_ONE_PATH if layout == "one_path" else BURST_TWO_PATHS
    first = Watch()
    probe = O.MergeOracle(dict(burst_spec(lay, 1), cell_sum="fixed"), np.float32)
    probe.reset()
    first(-1, probe, None)
    first(0, probe, probe.step(actions(probe.spec, 9, -1.5, 1.5)(0))[2])
    assert first.sub_burst == 2 and first.path_burst == (2 if layout == "one_path" else 1)
    spec = burst_spec(lay, sims_per_step)
    w = Watch()
    rl_arrivals = []
    ora = run(spec, 12, actions(spec, 9, -1.5, 1.5), check_every=1,
              watch=lambda k, o, d: (w(k, o, d), rl_arrivals.append(int(o.arrived_rl.sum()))))
    assert w.sub_burst >= 2 and w.burst >= 2 and w.crash_steps == 0
    assert sum(rl_arrivals) >= 2 and ora.total_arrived.min() >= 5


# ------------------------------------------------------------------ 4: the window miss
@pytest.mark.parametrize("sim_step,zipper_distance,q", [(1.0, 0.0, 3600.0), (1.0, 50.0, 5000.0), (2.0, 0.0, 5000.0),
                                                        (2.0, 50.0, 3600.0)])
def test_drop_queue_counts_that_leave_the_window_take_the_full_search(sim_step, zipper_distance, q):
    """count_near3 decides "vehicles of path q ahead of me" from the four mirror entries around the last count, which holds
    a change of -1 .. +1; a larger one sends the wave through count_ahead3.  With sub-steps of 0.5 s (every other lane-drop
    test) a vehicle passes at most two vehicles of the other paths per sub-step; with 1 s and 2 s it passes three and more, and
    its count of ONE other path moves by two and more (both asserted on the oracle's positions)."""
    spec = bottleneck_spec(R=2, cap_human=120, cap_rl=20, horizon=200, seed=41, q=q, sim_step=sim_step,
                           zipper_distance=zipper_distance)
    w = Watch(passing=True)
    run(spec, 100, actions(spec, 6, -1.5, 1.5), check_every=10, watch=w)
    assert w.passed >= 3 and w.count_jump >= 2, (w.passed, w.count_jump)
    assert w.most_on_a_path <= PATH_LANES


def test_drop_queue_one_launch_carries_the_counts_through_window_misses():
    """Stepping starts every launch from a full search (the counts of a launch start at 0); ONE launch of 60 steps carries
    them from sub-step to sub-step, less the arrivals, through every window miss of the run (sim_step = 2 s: counts that
    jump by 3): every row of the rollout equals the stepped oracle, and so does the state after it."""
    import torch
    spec = bottleneck_spec(R=2, cap_human=120, cap_rl=20, horizon=200, seed=41, q=3600.0, sim_step=2.0, zipper_distance=50.0)
    K, R, A = 60, 2, spec["num_rl"]
    acts = np.random.default_rng(6).uniform(-1.5, 1.5, (K, R, A)).astype(np.float32)
    ora = O.MergeOracle(dict(spec, cell_sum="fixed"), np.float32)
    sim = make(spec, "f32")
    np.testing.assert_array_equal(sim.reset(), ora.reset().astype(np.float32))
    dev = torch.device("cuda:0")
    out = (torch.empty((K, R, sim.obs_dim), dtype=torch.float32, device=dev),
           torch.empty((K, R), dtype=torch.float32, device=dev), torch.empty((K, R), dtype=torch.uint8, device=dev))
    sim.rollout_dev(K, *out, actions=torch.from_numpy(acts).to(dev))
    sim.sync()
    assert sim.last_kernel == "k_drop_queue"
    obs, rew, done = [t.cpu().numpy() for t in out]
    w = Watch(passing=True)
    w(-1, ora, None)
    for k in range(K):
        o_ref, r_ref, d_ref = ora.step(acts[k])
        w(k, ora, d_ref)
        np.testing.assert_array_equal(obs[k], o_ref.astype(np.float32), err_msg="obs, step %d" % k)
        np.testing.assert_array_equal(rew[k], r_ref.astype(np.float32), err_msg="reward, step %d" % k)
        np.testing.assert_array_equal(done[k].astype(bool), d_ref, err_msg="done, step %d" % k)
    compare_state(sim, ora)
    compare_vmax(sim, ora)
    assert w.count_jump >= 3 and w.most_on_a_path <= PATH_LANES and ora.total_arrived.min() >= 20
    sim.close()


# ------------------------------------------------------------------ 5: pinned fuzz
def random_drop_case(seed):
    """(spec, action function or None, steps) of a random lane-drop configuration within k_drop_queue's scope
    (Sim::dropq_ok); scripts/soak_fuzz_queue.py draws its lane-drop cases here too."""
    rng = np.random.default_rng(7700 + seed)
    R, N = int(rng.integers(1, 5)), int(rng.integers(36, 257))
    cap_rl = int(rng.integers(2, min(40, N - 33)))
    dv = bool(rng.integers(0, 4))
    spec = bottleneck_spec(R=R, cap_human=N - cap_rl, cap_rl=cap_rl, horizon=int(rng.integers(100, 400)), seed=seed,
                           q=float(rng.integers(1500, 5001)), av_frac=float(rng.choice([0.1, 0.3])),
                           zipper_distance=float(rng.choice([0.0, 25.0, 50.0, 120.0])),
                           warmup_steps=int(rng.choice([0, 20])), crash_gap=float(rng.choice([0.0, 1.0])),
                           sims_per_step=int(rng.integers(1, 4)), sim_step=float(rng.choice([0.2, 0.5, 1.0])),
                           **({} if dv else {"env": O.ENV_BOTTLENECK}))
    if rng.integers(0, 2):                                  # fixed entry lanes, two inflows on one of them, one random lane
        human, rl = spec["inflows"]
        lanes = rng.permutation(4)
        spec["inflows"] = [dict(human, route=int(lanes[0]), period=float(rng.uniform(2.0, 4.0))),
                           dict(rl, route=int(lanes[0]), period=float(rng.uniform(5.0, 9.0))),
                           dict(human, route=int(lanes[1]), period=float(rng.uniform(2.0, 4.0))),
                           dict(human, route=-1, period=float(rng.uniform(2.5, 5.0)))]
    steps = int(rng.integers(100, 161))
    return spec, (actions(spec, seed, -1.5, 1.5) if dv else None), steps


# What the fast seeds hold between them, by the oracle alone (asserted per seed below; the values reached are in brackets):
#   seed: (slots, env head, zipper_distance, steps with a collision >=, dropped random-lane vehicles >=)
# replicas 2 1 2 4 1 4, sub-steps per step 3 3 1 1 2 2, sim_step 0.2 0.5 1 1 0.2 0.2, crash_gap 1 0 1 1 0 0, warm-up in all
# but the first, fixed entry lanes with two inflows on one lane in seeds 1, 23, 29; most vehicles on a path 39 21 24 54 18 21
FUZZ_FACTS = {1: (86, O.ENV_BOTTLENECK_DV, 50.0, 0, 1),        # [12 dropped]
              10: (95, O.ENV_BOTTLENECK_DV, 0.0, 1, 1),        # [51 collision steps, 6 dropped]
              22: (229, O.ENV_BOTTLENECK_DV, 0.0, 1, 1),       # [63, 37]
              23: (103, O.ENV_BOTTLENECK_DV, 50.0, 0, 1),      # [35 dropped]
              28: (82, O.ENV_BOTTLENECK, 25.0, 0, 1),          # [16 dropped] no actions
              29: (47, O.ENV_BOTTLENECK_DV, 120.0, 0, 1)}      # [7 dropped] the 64-slot sizes
# (of seeds 100 .. 114 the oracle puts more than 64 vehicles on a path in 101, 105 and 108: replaced, not caught)
FUZZ_SLOW = [100, 102, 103, 104, 106, 107, 109, 110, 111, 112, 113, 114]


@pytest.mark.parametrize("seed", seeds(sorted(FUZZ_FACTS), FUZZ_SLOW))
def test_drop_queue_fuzz_random_lane_drop_configs_bit_exact(seed):
    spec, acts, steps = random_drop_case(seed)
    w = Watch()
    ora = run(spec, steps, acts, check_every=max(1, steps // 8), watch=w)
    assert w.most_on_a_path <= PATH_LANES          # (a seed that outgrows a path is replaced, not caught)
    if seed in FUZZ_FACTS:
        slots, env, zipper, crash_steps, dropped = FUZZ_FACTS[seed]
        assert (int(spec["num_vehicles"]), int(spec["env"]), float(spec["zipper_distance"])) == (slots, env, zipper)
        assert w.crash_steps >= crash_steps and int(ora.total_dropped.max()) >= dropped


# ------------------------------------------------------------------ 6: both kernels on one handle
def test_drop_queue_and_the_slot_order_kernel_alternate_on_one_handle():
    """Unmasked launches of at least one step run on k_drop_queue (the warm-up of a full reset too); a masked reset -- its
    zero-step launch and its masked warm-up -- runs on the slot-order kernel, and the next step rebuilds the queues from the
    slot arrays that kernel wrote.  Then maxSpeed values uploaded with set_state reach the queues the same way."""
    from flow_amd import _lib as L
    spec = bottleneck_spec(R=4, cap_human=100, cap_rl=12, warmup_steps=20, horizon=300, seed=23)
    ora = O.MergeOracle(dict(spec, cell_sum="fixed"), np.float32)
    sim = make(spec, "f32")
    act = actions(spec, 8, -1.5, 1.5)

    def steps(k0, n):
        for k in range(k0, k0 + n):
            a = act(k)
            o_ref, r_ref, d_ref = ora.step(a)
            o_gpu, r_gpu, d_gpu = sim.step(a)
            assert sim.last_kernel == "k_drop_queue"
            np.testing.assert_array_equal(o_gpu, o_ref.astype(np.float32), err_msg="obs, step %d" % k)
            np.testing.assert_array_equal(r_gpu, r_ref.astype(np.float32), err_msg="reward, step %d" % k)
            np.testing.assert_array_equal(d_gpu, d_ref, err_msg="done, step %d" % k)
        compare_state(sim, ora)
        compare_vmax(sim, ora)

    np.testing.assert_array_equal(sim.reset(), ora.reset().astype(np.float32))
    assert sim.last_kernel == "k_drop_queue"                # (the 20 unmasked warm-up steps)
    compare_state(sim, ora)
    steps(0, 40)
    before = ora.total_departed.copy()
    assert before.min() > 10
    mask = np.array([1, 0, 0, 1], dtype=bool)
    np.testing.assert_array_equal(sim.reset(mask), ora.reset(mask).astype(np.float32))
    assert sim.last_kernel == "k_steps_wide"
    compare_state(sim, ora)
    compare_vmax(sim, ora)
    assert (ora.total_departed[mask] < before[mask]).all() and (ora.total_departed[~mask] == before[~mask]).all()
    steps(40, 40)
    vm = sim.get_state(L.FS_FIELD_MAX_SPEED)
    vm[:, 100:] = np.random.default_rng(4).uniform(4.0, 22.0, (4, 12)).astype(np.float32)
    sim.set_state(L.FS_FIELD_MAX_SPEED, vm)
    ora.vmax[:, 100:] = vm[:, 100:]
    assert ora.alive[:, 100:].sum() >= 4                    # RL vehicles in the network take the new values along
    compare_vmax(sim, ora)
    steps(80, 20)
    sim.close()


# ------------------------------------------------------------------ 7: launch fragments
def test_drop_queue_rollout_in_odd_fragments_equals_stepping():
    """rollout_dev in fragments of 1, 2, 5, 16 and 3 steps (the observation accumulators and the collision flags are
    double-buffered by LAUNCH-relative parity: odd lengths first), the middle three emitting their last step only, against
    a second handle stepped 27 times and the oracle: every emitted row and every state field after each fragment."""
    import torch
    from flow_amd import _lib as L
    spec = bottleneck_spec(R=3, cap_human=64, cap_rl=12, horizon=300, seed=29, sims_per_step=2, q=3600.0)
    R, A = 3, spec["num_rl"]
    acts = np.random.default_rng(2).uniform(-1.5, 1.5, (27, R, A)).astype(np.float32)
    dev = torch.device("cuda:0")
    acts_dev = torch.from_numpy(acts).to(dev)
    ora = O.MergeOracle(dict(spec, cell_sum="fixed"), np.float32)
    a, b = make(spec, "f32"), make(spec, "f32")
    a.reset(), b.reset(), ora.reset()
    k0 = 0
    for K, every in ((1, True), (2, False), (5, False), (16, False), (3, True)):
        lead = (K,) if every else ()
        out = (torch.empty(lead + (R, a.obs_dim), dtype=torch.float32, device=dev),
               torch.empty(lead + (R,), dtype=torch.float32, device=dev), torch.empty(lead + (R,), dtype=torch.uint8, device=dev))
        a.rollout_dev(K, *out, actions=acts_dev[k0:k0 + K], obs_every_step=every)
        a.sync()
        assert a.last_kernel == "k_drop_queue"
        got = [t.cpu().numpy().reshape((-1,) + tuple(t.shape[len(lead):])) for t in out]     # rows: emitted steps
        for j in range(K):
            o_ref, r_ref, d_ref = ora.step(acts[k0 + j])
            o, r, d = b.step(acts[k0 + j])
            assert b.last_kernel == "k_drop_queue"
            np.testing.assert_array_equal(o, o_ref.astype(np.float32), err_msg="stepping vs oracle, step %d" % (k0 + j))
            if every or j == K - 1:
                row = j if every else 0
                np.testing.assert_array_equal(got[0][row], o, err_msg="obs, step %d" % (k0 + j))
                np.testing.assert_array_equal(got[1][row], r, err_msg="reward, step %d" % (k0 + j))
                np.testing.assert_array_equal(got[2][row].astype(bool), d, err_msg="done, step %d" % (k0 + j))
        k0 += K
        for f in (L.FS_FIELD_POS, L.FS_FIELD_VEL, L.FS_FIELD_PREV_VEL, L.FS_FIELD_ACCEL, L.FS_FIELD_ROUTE, L.FS_FIELD_SEQ,
                  L.FS_FIELD_ORIGIN, L.FS_FIELD_LEADER, L.FS_FIELD_HEADWAY, L.FS_FIELD_ARRIVED_RL, L.FS_FIELD_COUNTERS,
                  L.FS_FIELD_MAX_SPEED):
            np.testing.assert_array_equal(a.get_state(f), b.get_state(f), err_msg="field %d after %d steps" % (f, k0))
        compare_state(a, ora)
    assert k0 == 27 and ora.total_departed.min() >= 15 and (ora.get_state()[:, :35] > 0).any()
    a.close(), b.close()
