"""GPU parity of the fast / slow form of the hand-written FS_MIXED pair step (flow_amd/csrc/flowsim_pair.h:
mixed_step_asm_b / mixed_step_asm_slow) at the places where the two forms meet: `mixed` rollouts against the C twin
refsim_ring_idm_mixed, bit for bit, for obs, rew, done, pos, vel and the time counter.

Every case has exponent 4 and divisors (v0, 2 sqrt(a b), the ring length) for which the host's proof of the reciprocal
divisions succeeds (30, 2 sqrt(1.5), 8; 60.4, 189.4, 200.4, 230.4, 336.4), i.e. the hand-written instantiation runs.
What a case is meant to contain (wraps in most steps, none at all, a clamped headway in the step of a collision) is
asserted on the numpy restatement of the rule (tests/test_pair_fastpath_cpu.py: FastSlowModel), which the CPU suite holds
to the same twin."""
import numpy as np
import pytest

from helpers import idm_vehicle, ring_spec
from oracle import cbuild
from test_pair_fastpath_cpu import C1E3, FastSlowModel

pytestmark = pytest.mark.gpu


def mixed_launches(spec, Ks):
    """`mixed` rollouts of Ks[0], Ks[1], ... steps on one handle, observation every step; host copies + the handle."""
    import torch
    from flow_amd.sim import FlowSim
    sim = FlowSim(spec, precision="mixed")
    dev = torch.device("cuda", 0)
    K, R = sum(Ks), sim.R
    obs = torch.full((K, R, sim.obs_dim), float("nan"), dtype=torch.float32, device=dev)
    rew = torch.full((K, R), float("nan"), dtype=torch.float32, device=dev)
    done = torch.full((K, R), 7, dtype=torch.uint8, device=dev)
    sim.reset()
    torch.cuda.synchronize()          # the fills above run on torch's stream, the simulator on its own
    k0 = 0
    for k in Ks:
        sim.rollout_dev(k, obs[k0:k0 + k], rew[k0:k0 + k], done[k0:k0 + k], obs_every_step=True)
        k0 += k
    sim.sync()
    return sim, obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy().astype(bool)


def assert_equals_twin(spec, Ks, kernel="k_rollout_pair"):
    sim, obs, rew, done = mixed_launches(spec, Ks)
    assert sim.last_kernel == kernel, sim.last_kernel
    twin = cbuild.CRingIDMMixed(spec)
    to, tr, td = twin.rollout(sum(Ks), obs_every_step=True)
    for k in range(sum(Ks)):
        np.testing.assert_array_equal(obs[k], to[k], err_msg="obs step %d" % k)
        np.testing.assert_array_equal(rew[k], tr[k], err_msg="rew step %d" % k)
        np.testing.assert_array_equal(done[k], td[k], err_msg="done step %d" % k)
    np.testing.assert_array_equal(sim.pos, twin.x)
    np.testing.assert_array_equal(sim.vel, twin.v)
    np.testing.assert_array_equal(sim.time_counter, twin.tc)
    sim.close()


def short_ring(R=9, N=22, moving=True, seed=0, horizon=10 ** 6):
    """22 vehicles of 0.5 m on a 60.4 m ring that follow closely and pick up speed quickly (T = 0.1 s, s0 = 0.2 m, a = b =
    4 m/s^2), so that they keep moving at a spacing of 2.7 m.  R = 9: the third wave holds one replica and three clones."""
    rng = np.random.default_rng(seed)
    L = 60.4
    spec = ring_spec(R=R, N=N, length=230.0, bunching=0, junction_length=0.1, horizon=horizon,
                     vehicles=[idm_vehicle(p=[30, 0.1, 4, 4, 4, 0.2, 0, 0], length=0.5) for _ in range(N)])
    spec["ring_length"] = np.full(R, 60.0)                  # (the start-position helper places 5 m vehicles: set by hand)
    spec["init_pos"] = np.arange(N) * (L / N) + rng.uniform(0, 0.4, (R, N))
    if moving:
        spec["init_vel"] = rng.uniform(5, 12, (R, N))
    return spec


def slow_share(spec, K):
    model = FastSlowModel(spec)
    for _ in range(K):
        model.step()
    return model.slow_groups / model.groups


def test_short_ring_wraps_in_most_steps():
    spec = short_ring()
    assert slow_share(spec, 70) > 0.5, "the case is meant to take the slow step in most steps"
    assert_equals_twin(spec, [70])


def test_short_ring_from_rest_fast_steps_only():
    spec = short_ring(moving=False)
    assert slow_share(spec, 5) == 0.0, "the case is meant to contain fast steps only"
    assert_equals_twin(spec, [5])


def test_two_launches_equal_one():
    # 33 = 2 blocks of 16 + 1 remainder step, 37 = 2 blocks + 5: the remainder loop and the rebuild of the wrap addends
    # from the state a launch finds; the episode ends (horizon 50) inside the second launch
    spec = short_ring(seed=1, horizon=50)
    one = mixed_launches(spec, [70])
    two = mixed_launches(spec, [33, 37])
    for a, b in zip(one[1:], two[1:]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(one[0].pos, two[0].pos)
    np.testing.assert_array_equal(one[0].vel, two[0].vel)
    np.testing.assert_array_equal(one[0].time_counter, two[0].time_counter)
    one[0].close(), two[0].close()
    assert_equals_twin(spec, [33, 37])


def crash_spec():
    """Vehicle 7 starts 5.0005 m in front of vehicle 6 (length 5: a headway of 0.5 mm, clamped by the launch's prologue),
    vehicle 6 at 10.8 m/s: the first step leaves a headway of -0.6 mm -- the collision bit and the clamp |h| < 1e-3 in
    the same step."""
    R, N = 5, 22
    spec = ring_spec(R=R, N=N, length=230.0, bunching=0, junction_length=0.1, horizon=100)
    pos = np.asarray(spec["init_pos"], np.float64).copy()
    pos[:, 7] = pos[:, 6] + 5.0005
    vel = np.zeros((R, N))
    vel[:, 6] = 10.8
    spec["init_pos"], spec["init_vel"] = pos, vel
    return spec


def test_clamp_and_collision_in_the_same_step():
    spec = crash_spec()
    model = FastSlowModel(spec)
    assert model.H[0, 6] == C1E3                                   # the prologue's clamp
    _, d, need = model.step()
    h = np.float32(model.x[0, 7] - model.x[0, 6] - 5.0)
    assert -1e-3 < h < 0 and d.all() and need.all() and model.H[0, 6] == C1E3, (h, d, need, model.H[0, 6])
    assert_equals_twin(spec, [20])


@pytest.mark.parametrize("N", [18, 32])
def test_both_ends_of_the_16_lane_row_per_slot_lengths(N):
    # 9 and 16 occupied lanes of a 16-lane row; lengths 3.5 / 5 / 7 per slot (a lane's two leaders differ in length)
    R, K = 7, 90
    rng = np.random.default_rng(N)
    veh = [idm_vehicle(length=float(rng.choice([3.5, 5.0, 7.0]))) for _ in range(N)]
    spec = ring_spec(R=R, N=N, length=10.5 * N, bunching=0, junction_length=0.1, horizon=80, vehicles=veh)
    spec["init_pos"] = np.asarray(spec["init_pos"]) + np.abs(rng.normal(0, 0.3, (R, N)))
    spec["init_vel"] = rng.uniform(0, 12, (R, N))
    share = slow_share(spec, K)
    assert 0.0 < share < 1.0, "the case is meant to mix fast and slow steps"
    assert_equals_twin(spec, [K])


def test_speed_mode_25_part_a():
    R, N, K = 6, 22, 90
    rng = np.random.default_rng(25)
    veh = [idm_vehicle(speed_mode=25, max_decel=float(rng.choice([1.5, 4.5]))) for _ in range(N)]
    spec = ring_spec(R=R, N=N, length=200.0, bunching=0, junction_length=0.1, horizon=80, vehicles=veh)
    spec["init_pos"] = np.asarray(spec["init_pos"]) + np.abs(rng.normal(0, 0.3, (R, N)))
    spec["init_vel"] = rng.uniform(0, 12, (R, N))
    share = slow_share(spec, K)
    assert 0.0 < share < 1.0, "the case is meant to mix fast and slow steps"
    assert_equals_twin(spec, [K], kernel="k_rollout_pair+speed_mode")
