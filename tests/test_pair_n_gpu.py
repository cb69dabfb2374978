"""GPU parity of the vehicle-count-specialised pair rollout k_rollout_pair_n<T, 11> (flow_amd/csrc/flowsim_pair.h: the
observation rows of the reference's 22-vehicle ring leave through a 16-step LDS image of each wave) against the kernel it
replaces for that ring, k_rollout_pair, which a handle created with FLOWSIM_PAIR_GENERIC_N=1 keeps.  (Sim::launch_pair
takes the entry for launches of PAIR_N_MIN_STEPS = 512 steps or more; FLOWSIM_PAIR_N_ALWAYS=1 gives it every launch, which
is how the short shapes below reach it.)

The change moves data only, so everything a launch returns or leaves behind is compared byte for byte: obs, rew, done, and
the handle's positions, speeds and time counters.  The shapes are chosen for the paths of the image:
  * R in {1, 4, 5, 9}: a wave with rows past R (their pieces are redirected to replica R - 1), whole idle waves of a block;
  * K in {1, 15, 16, 17, 32, 33, 50}: no full block (the tail's per-step path alone), one block (drained after the loop only),
    two and three blocks (pieces leaving in place during the next block), tails behind them;
  * two launches back to back (16, then 17 steps): the second starts with nothing to drain;
  * rows behind the K the launch was given stay as the test filled them.
(Parity with the oracles is tests/test_pair_gpu.py's; its 1500-step launches of the 22-vehicle ring run on this entry.)"""
import os

import numpy as np
import pytest

from helpers import idm_vehicle, ring_spec

pytestmark = pytest.mark.gpu

KS = [1, 15, 16, 17, 32, 33, 50]
GUARD = 2                                  # step rows behind the launch's K, filled and checked
FILL = 0x7FC12345                          # a NaN pattern no observation, reward or flag byte run can be mistaken for

VARIANTS = {
    # name: (precision, vehicle keywords, fs_last_kernel)
    "mixed": ("mixed", {}, "k_rollout_pair"),
    "mixed_sm25": ("mixed", dict(speed_mode=25), "k_rollout_pair+speed_mode"),
    "f32": ("f32", {}, "k_rollout_pair"),
    "f32_sm25": ("f32", dict(speed_mode=25), "k_rollout_pair+speed_mode"),
    "f32_noise": ("f32", dict(noise=0.2), "k_rollout_pair+noise"),
}


def spec_for(R, veh_kw, N=22, ring_lengths=None):
    spec = ring_spec(R=R, N=N, length=230.0, bunching=0, junction_length=0.1, horizon=40,
                     vehicles=[idm_vehicle(**veh_kw) for _ in range(N)], seed=5)
    rng = np.random.default_rng(100 + R)
    spec["init_pos"] = np.asarray(spec["init_pos"]) + np.abs(rng.normal(0, 0.4, (R, N)))   # every replica its own start
    spec["init_vel"] = rng.uniform(0, 6, (R, N))
    if ring_lengths is not None:
        spec["ring_length"] = np.asarray(ring_lengths, dtype=np.float64)
    return spec


def make(spec, precision, **env):
    from flow_amd.sim import FlowSim
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return FlowSim(spec, precision=precision)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def launches(sim, steps):
    """reset, then one fs_rollout_dev launch per entry of `steps` into consecutive rows; returns the raw bytes of everything."""
    import torch
    dev = torch.device("cuda", 0)
    K, R = sum(steps), sim.R
    obs = torch.full((K + GUARD, R, sim.obs_dim), FILL, dtype=torch.int32, device=dev).view(torch.float32)
    rew = torch.full((K + GUARD, R), FILL, dtype=torch.int32, device=dev).view(torch.float32)
    done = torch.full((K + GUARD, R), 7, dtype=torch.uint8, device=dev)
    sim.reset()
    torch.cuda.synchronize()               # the fills run on torch's stream, the simulator on its own
    at = 0
    for k in steps:
        sim.rollout_dev(k, obs[at:at + k], rew[at:at + k], done[at:at + k], obs_every_step=True)
        at += k
    sim.sync()
    out = dict(obs=obs.view(torch.int32).cpu().numpy(), rew=rew.view(torch.int32).cpu().numpy(), done=done.cpu().numpy(),
               pos=np.asarray(sim.pos).copy(), vel=np.asarray(sim.vel).copy(), time=np.asarray(sim.time_counter).copy())
    assert (out["obs"][K:] == FILL).all() and (out["rew"][K:] == FILL).all() and (out["done"][K:] == 7).all(), \
        "the launch wrote behind its last step"
    assert (out["obs"][:K] != FILL).all() and (out["rew"][:K] != FILL).all() and (out["done"][:K] != 7).all(), \
        "the launch left a row unwritten"
    return out


def same(a, b, what):
    for key in ("obs", "rew", "done", "pos", "vel", "time"):
        x, y = a[key], b[key]
        assert x.dtype == y.dtype and x.shape == y.shape, (what, key)
        assert x.tobytes() == y.tobytes(), "%s: %s differs (%d elements)" % (what, key, int((x != y).sum()))


def check_pair(spec, precision, family, step_lists):
    new = make(spec, precision, FLOWSIM_KERNEL_DETAIL="1", FLOWSIM_PAIR_N_ALWAYS="1")
    old = make(spec, precision, FLOWSIM_KERNEL_DETAIL="1", FLOWSIM_PAIR_N_ALWAYS="1", FLOWSIM_PAIR_GENERIC_N="1")
    plain = make(spec, precision)
    try:
        for steps in step_lists:
            a, b = launches(new, steps), launches(old, steps)
            assert new.last_kernel == family + "[n11]", new.last_kernel
            assert old.last_kernel == family, old.last_kernel
            same(a, b, "steps %s" % (steps,))
        launches(plain, [step_lists[0][0]])
        assert plain.last_kernel == family, plain.last_kernel          # the name only changes when asked for
    finally:
        new.close(), old.close(), plain.close()


@pytest.mark.parametrize("R", [1, 4, 5, 9])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_specialised_entry_equals_the_generic_kernel_byte_for_byte(variant, R):
    precision, veh_kw, family = VARIANTS[variant]
    check_pair(spec_for(R, veh_kw), precision, family, [[k] for k in KS] + [[16, 17]])


@pytest.mark.parametrize("precision", ["mixed", "f32"])
def test_specialised_entry_with_a_ring_length_per_replica(precision):
    R = 9
    spec = spec_for(R, {}, ring_lengths=np.linspace(226.0, 262.0, R))
    check_pair(spec, precision, "k_rollout_pair", [[50], [16, 17]])


@pytest.mark.parametrize("precision", ["mixed", "f32"])
def test_long_launches_take_the_entry_by_themselves_short_ones_do_not(precision):
    """520 steps: 32 blocks leaving in place one behind the other, a tail of 8 -- on the handle's own choice of kernel."""
    spec = spec_for(5, {})
    new = make(spec, precision, FLOWSIM_KERNEL_DETAIL="1")
    old = make(spec, precision, FLOWSIM_KERNEL_DETAIL="1", FLOWSIM_PAIR_GENERIC_N="1")
    try:
        launches(new, [20])
        assert new.last_kernel == "k_rollout_pair", new.last_kernel
        a, b = launches(new, [520]), launches(old, [520])
        assert new.last_kernel == "k_rollout_pair[n11]" and old.last_kernel == "k_rollout_pair", (new.last_kernel, old.last_kernel)
        same(a, b, "520 steps")
    finally:
        new.close(), old.close()


@pytest.mark.parametrize("precision", ["mixed", "f32"])
def test_other_vehicle_counts_keep_their_kernel(precision):
    sim = make(spec_for(5, {}, N=20), precision, FLOWSIM_KERNEL_DETAIL="1", FLOWSIM_PAIR_N_ALWAYS="1")
    try:
        launches(sim, [17])
        assert sim.last_kernel == "k_rollout_pair", sim.last_kernel
    finally:
        sim.close()
