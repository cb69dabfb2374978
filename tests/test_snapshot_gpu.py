"""Snapshots of a handle (include/flowsim.h fs_snapshot_info; flow_amd/csrc/flowsim_snap.h k_snapshot).

The central property, per step-kernel family (``sim.last_kernel`` asserted): step ``a`` steps, snapshot, record ``b`` steps
(observations, rewards, done flags -- and the policy kernels' actions and log-probabilities -- then every fs_get_state field
and the whole host blob), restore, record ``b`` steps again: both records are equal bit for bit.  So that "equal" is not
"equally wrong", the first record is also held to a handle that never took or restored a snapshot (the path the parity tests
hold to the oracle) and, on the IDM ring, to the oracle itself.

Further: a masked restore with selected and unselected replicas in one group of the kernel, snapshot + steps + restore inside
one captured graph, a host blob carried into another handle (with a ring length that handle never had) and the refusals by
name, and the no-op.  The device blob k_snapshot writes is compared with the host blob fs_snapshot copies field by field."""
import ctypes
import re

import numpy as np
import pytest

from helpers import bottleneck_spec, figure_eight_spec, idm_vehicle, merge_spec, multilane_spec, nan_actions, ring_spec
from oracle import refsim as S
from test_policy_gpu import fig8_rl_spec, make_policy, make_policy_in
from test_ringrl_gpu import make, rl_ring_spec, rollout

pytestmark = pytest.mark.gpu

HEADER = 64                     # the host blob: a 64-byte header, then the device blob


def dev():
    import torch
    return torch.device("cuda", 0)


def fields_of(sim):
    from flow_amd import _lib as L
    names = ["POS", "VEL", "PREV_VEL", "ACCEL", "TIME", "INIT_POS", "INIT_VEL", "CTRL_STATE", "LANE", "LAST_LC", "INIT_LANE",
             "SORT_KEY", "HEADWAY", "LEADER"]
    if sim.open_net:
        names += ["ROUTE", "SEQ", "ORIGIN", "FOLLOWER", "CTL_SEQ", "COUNTERS", "ARRIVED_RL", "MAX_SPEED", "INFLOW_PERIOD",
                  "INIT_INFLOW_PERIOD"]
    else:
        names += ["RING_LENGTH", "INIT_RING_LENGTH"]
    return [(n, getattr(L, "FS_FIELD_" + n)) for n in names]


def end_state(sim):
    """Every fs_get_state field and the host blob (which holds what no field reaches: counters, histories, the draws)."""
    out = {"blob": np.frombuffer(sim.snapshot(), dtype=np.uint8)}      # (first: reading an FS_F16S field rewrites its staging)
    out.update({n: sim.get_state(f).copy() for n, f in fields_of(sim)})
    return out


def same_bits(x, y, what):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    assert x.shape == y.shape and x.dtype == y.dtype, what
    bad = np.flatnonzero(x.view(np.uint8).reshape(-1) != y.view(np.uint8).reshape(-1))
    assert bad.size == 0, "%s: %d bytes differ, the first at %d" % (what, bad.size, bad[0])


def same_record(r1, r2, what):
    assert len(r1) == len(r2)
    for i, (x, y) in enumerate(zip(r1, r2)):
        same_bits(x, y, "%s: output %d" % (what, i))


def new_blob(sim):
    import torch
    t = torch.zeros(int(sim.snapshot_info().bytes), dtype=torch.uint8, device=dev())
    torch.cuda.synchronize()              # (the handle launches on a stream of its own)
    return t


# ---------------------------------------------------------------------------------------------------------- the drivers
def tape_driver(tape):
    """drive(sim, k0, K): K steps in one rollout launch with the actions of global steps k0 .. k0 + K - 1 (None: no actions)."""
    def drive(sim, k0, K):
        return rollout(sim, K, None if tape is None else tape[k0:k0 + K])
    return drive


def policy_driver(policies):
    """K x (policy, step, reset of finished episodes) in one launch; ``policies[id(sim)]`` is the handle's own policy object."""
    def drive(sim, k0, K):
        import torch
        out = (torch.zeros((K + 1, sim.R, sim.obs_dim), device=dev()), torch.zeros((K, sim.R), device=dev()),
               torch.zeros((K, sim.R), device=dev()), torch.zeros((K, sim.R), device=dev()),
               torch.zeros((K, sim.R), dtype=torch.uint8, device=dev()))
        torch.cuda.synchronize()
        sim.policy_rollout_dev(policies[id(sim)].struct, K, *out, reset_done=True)
        sim.sync()
        return tuple(t.cpu().numpy() for t in out)
    return drive


def pair_driver(policies, w=0.5):
    def drive(sim, k0, K):
        import torch
        out = (torch.zeros((K + 1, sim.R, sim.obs_dim), device=dev()), torch.zeros((2, K, sim.R), device=dev()),
               torch.zeros((2, K, sim.R), device=dev()), torch.zeros((K, sim.R), device=dev()),
               torch.zeros((K, sim.R), dtype=torch.uint8, device=dev()))
        torch.cuda.synchronize()
        av, adv = policies[id(sim)]
        sim.policy_pair_rollout_dev(av.struct, adv.struct, w, K, *out, reset_done=True)
        sim.sync()
        return tuple(t.cpu().numpy() for t in out)
    return drive


def uniform_tape(K, R, A, seed, lo=-1.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, (K, R, A)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ the cases
def pis_ring_spec():
    spec = ring_spec(R=5, N=22, junction_length=0.1, horizon=400)
    spec["vehicles"][2] = idm_vehicle(controller=S.CTRL_PISATURATION, p=[0] * 8, max_accel=2.6, delay=1.0)
    return spec


def case(name):
    """(spec, precision, env switches, kernel names, a, b, driver factory, arrivals expected inside the window)"""
    A, B = 7, 10
    if name in ("idm_f32", "idm_mixed"):
        rng = np.random.default_rng(1)
        spec = ring_spec(R=6, N=22, junction_length=0.1, horizon=400)
        spec["init_pos"] = np.asarray(spec["init_pos"]) + np.abs(rng.normal(0, 0.5, (6, 22)))
        return spec, name[4:], {}, ("k_rollout_pair",), A, B, lambda sims: tape_driver(None), False
    if name == "ring_pair_noise":
        spec = rl_ring_spec(R=6, N=22, noise=0.2, horizon=400, seed=3)
        return spec, "f32", {}, ("k_ring_pair",), A, B, lambda sims: tape_driver(uniform_tape(A + B, 6, 1, 4)), False
    if name == "ring_policy":
        spec = rl_ring_spec(R=6, N=22, noise=0.2, horizon=12, seed=5)        # steps 12 (a reset) falls inside 7 .. 16
        return spec, "f32", {}, ("k_ring_policy",), A, B, \
            lambda sims: policy_driver({id(s): make_policy(3, False, seed=3) for s in sims}), False
    if name == "loop":
        spec = figure_eight_spec(R=4, horizon=400)
        return spec, "f32", {}, ("k_rollout_loop", "k_rollout_loop<FULL>"), A, B, lambda sims: tape_driver(None), False
    if name == "loop_policy":
        spec = fig8_rl_spec(4, "po", 0.2, horizon=12, seed=4)
        return spec, "f32", {}, ("k_loop_policy",), A, B, \
            lambda sims: policy_driver({id(s): make_policy_in(3, 3, False, seed=3) for s in sims}), False
    if name == "loop_pair":
        spec = fig8_rl_spec(4, "accel", 0.2, horizon=12, seed=4)
        return spec, "f32", {}, ("k_loop_policy<Adversarial>",), A, B, \
            lambda sims: pair_driver({id(s): (make_policy_in(28, 3, False, seed=3), make_policy_in(28, 1, True, seed=4))
                                      for s in sims}), False
    if name == "multilane":
        spec = multilane_spec(R=4, horizon=400)
        return spec, "f32", {}, ("k_steps_ml",), A, B, lambda sims: tape_driver(None), False
    if name == "pis":
        return pis_ring_spec(), "f32", {}, ("k_steps", "k_steps<CSET>", "k_steps<FAST>"), 30, 30, \
            lambda sims: tape_driver(None), False
    if name in ("merge_queue", "merge_open", "merge_f16s"):
        spec = merge_spec(R=4, horizon=400)                                  # the PO head: ctl_seq, the rl_veh list
        acts = nan_actions(4, spec["num_rl"], seed=2)
        tape = np.stack([acts(k) for k in range(220)])
        env = {"FLOWSIM_NO_QUEUE": 1} if name == "merge_open" else {}
        kern = {"merge_queue": ("k_merge_queue",), "merge_open": ("k_steps_open",),
                "merge_f16s": ("k_merge_queue", "k_steps_open")}[name]
        return spec, "f16s" if name == "merge_f16s" else "f32", env, kern, 120, 100, lambda sims: tape_driver(tape), True
    if name in ("drop_queue", "wide"):
        spec = bottleneck_spec(R=3, cap_human=40, cap_rl=8, horizon=400) if name == "drop_queue" else \
            bottleneck_spec(R=3, cap_human=70, cap_rl=10, horizon=400)
        tape = uniform_tape(160, 3, spec["num_rl"], 6, -1.5, 1.5)
        env = {"FLOWSIM_NO_QUEUE": 1} if name == "wide" else {}              # (the slot-order kernel of more than 64 slots)
        return spec, "f32", env, ("k_drop_queue",) if name == "drop_queue" else ("k_steps_wide",), 60, 100, \
            lambda sims: tape_driver(tape), True
    raise KeyError(name)


CASES = ["idm_f32", "idm_mixed", "ring_pair_noise", "ring_policy", "loop", "loop_policy", "loop_pair", "multilane", "pis",
         "merge_queue", "merge_open", "merge_f16s", "drop_queue", "wide"]


@pytest.mark.parametrize("name", CASES)
def test_a_restored_handle_repeats_its_future_bit_for_bit(name):
    from flow_amd import _lib as L
    spec, precision, env, kernels, a, b, driver_of, arrivals = case(name)
    sim, twin = make(spec, precision, **env), make(spec, precision, **env)
    drive = driver_of((sim, twin))
    if name == "ring_policy":                        # a pending ring length: the reset inside the window takes it
        for s in (sim, twin):
            s.reset()
            s.set_state(L.FS_FIELD_INIT_RING_LENGTH, s.get_state(L.FS_FIELD_RING_LENGTH) + 3.0)
    else:
        sim.reset(), twin.reset()
    drive(sim, 0, a)
    blob = new_blob(sim)
    sim.snapshot_dev(blob)
    at_snapshot = end_state(sim)
    same_bits(blob.cpu().numpy(), at_snapshot["blob"][HEADER:], "k_snapshot's blob against fs_snapshot's field copies")
    rec1 = drive(sim, a, b)
    assert any(re.fullmatch(re.escape(k) + r"([<+].*)?", sim.last_kernel) for k in kernels), sim.last_kernel
    end1 = end_state(sim)
    assert not np.array_equal(end1["POS"], at_snapshot["POS"])                 # the window moved the simulator
    if arrivals:                                      # vehicles left the network inside the window
        assert (end1["COUNTERS"][:, 5] > at_snapshot["COUNTERS"][:, 5]).all()
    if name in ("ring_policy", "loop_policy", "loop_pair"):
        assert (rec1[4] != 0).any(axis=0).all()       # every replica finished an episode (and was reset) inside the window
    sim.restore_dev(blob)
    back = end_state(sim)
    for key in at_snapshot:
        same_bits(back[key], at_snapshot[key], "%s: %s right after the restore" % (name, key))
    rec2 = drive(sim, a, b)
    end2 = end_state(sim)
    same_record(rec1, rec2, name)
    for key in end1:
        same_bits(end2[key], end1[key], "%s: %s after the replayed window" % (name, key))
    # the handle that never took a snapshot
    drive(twin, 0, a)
    rec_twin = drive(twin, a, b)
    same_record(rec1, rec_twin, name + " against the untouched handle")
    for key in ("POS", "VEL", "TIME"):
        same_bits(twin.get_state(getattr(L, "FS_FIELD_" + key)), end1[key], "%s: %s of the untouched handle" % (name, key))
    if name == "idm_f32":                             # ... and the oracle
        ora = S.RingOracle(spec, np.float32)
        ora.reset()
        for k in range(a + b):
            o_ref, r_ref, d_ref = ora.step(None)
            if k >= a:
                same_bits(rec1[0][k - a], o_ref.astype(np.float32), "obs against the oracle, step %d" % k)
                same_bits(rec1[1][k - a], r_ref.astype(np.float32), "reward against the oracle, step %d" % k)
        same_bits(end1["POS"], ora.x.astype(np.float32), "positions against the oracle")
    sim.close(), twin.close()


def test_masked_restore_moves_the_selected_replicas_only():
    """R = 6, mask {1, 4}: selected and unselected replicas share the kernel's group of 8 (and a wave of the step kernel)."""
    import torch
    a, b, R = 7, 10, 6
    spec = rl_ring_spec(R=R, N=22, noise=0.2, horizon=400, seed=3)
    tape = uniform_tape(a + 2 * b, R, 1, 4)
    sel = np.array([0, 1, 0, 0, 1, 0], dtype=bool)
    sim, twin = make(spec, "f32"), make(spec, "f32")
    sim.reset(), twin.reset()
    rollout(sim, a, tape[:a])
    blob = new_blob(sim)
    sim.snapshot_dev(blob)
    rec1 = rollout(sim, b, tape[a:a + b])
    mask = torch.as_tensor(sel.astype(np.uint8), device=dev())
    torch.cuda.synchronize()
    sim.restore_dev(blob, mask)
    mixed = tape[a + b:a + 2 * b].copy()              # the selected replicas see the window's actions again
    mixed[:, sel] = tape[a:a + b][:, sel]
    rec2 = rollout(sim, b, mixed)
    assert sim.last_kernel.startswith("k_ring_pair")
    rollout(twin, a + b, tape[:a + b])
    rec_twin = rollout(twin, b, tape[a + b:a + 2 * b])
    for i in range(3):
        same_bits(rec2[i][:, sel], rec1[i][:, sel], "selected replicas, output %d" % i)
        same_bits(rec2[i][:, ~sel], rec_twin[i][:, ~sel], "unselected replicas, output %d" % i)
    same_bits(sim.pos[~sel], twin.pos[~sel], "positions of the unselected replicas")
    assert not np.array_equal(sim.time_counter[sel], twin.time_counter[sel])
    sim.close(), twin.close()


def test_snapshot_steps_and_restore_inside_one_captured_graph():
    import torch
    K, R = 9, 6
    spec = ring_spec(R=R, N=22, junction_length=0.1, horizon=400)
    sim = make(spec, "f32")
    sim.reset()
    blob = new_blob(sim)
    o = torch.zeros((K, R, sim.obs_dim), device=dev())
    r = torch.zeros((K, R), device=dev())
    d = torch.zeros((K, R), dtype=torch.uint8, device=dev())
    st = torch.cuda.Stream(dev())
    torch.cuda.synchronize()

    def body():
        sim.snapshot_dev(blob)
        sim.rollout_dev(K, o, r, d)
        sim.restore_dev(blob)
    with torch.cuda.stream(st):
        sim.set_stream(st.cuda_stream)                # (synchronises: before the capture)
        body()                                        # eager once: the lazy host work of the first rollout happens here
        sim.sync()
        want = (o.clone(), r.clone(), d.clone())
    st.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        body()
    for _ in range(2):
        o.zero_(), r.zero_(), d.zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            g.replay()
        st.synchronize()
        for x, y in zip((o, r, d), want):
            same_bits(x.cpu().numpy(), y.cpu().numpy(), "a replay of the captured bracket")
    assert float(want[0].abs().sum()) > 0
    sim.use_own_stream()
    sim.close()


def test_a_host_blob_continues_in_another_handle_and_foreign_blobs_are_refused_by_name():
    from flow_amd import _lib as L
    a, b, R = 7, 10, 6
    spec_a = ring_spec(R=R, N=22, length=230.0, junction_length=0.1, horizon=400)
    spec_b = ring_spec(R=R, N=22, length=263.0, junction_length=0.1, horizon=400)      # B never had A's ring length
    A, B = make(spec_a, "f32"), make(spec_b, "f32")
    A.reset(), B.reset()
    rollout(A, a, None)
    rollout(B, 3, None)
    blob = A.snapshot()
    B.restore(blob)
    same_bits(np.frombuffer(B.snapshot(), np.uint8), np.frombuffer(blob, np.uint8), "B's state after taking A's blob")
    rec_a, rec_b = rollout(A, b, None), rollout(B, b, None)
    assert B.last_kernel.startswith("k_rollout_pair")
    same_record(rec_a, rec_b, "B continues as A does")
    same_bits(A.pos, B.pos, "positions")
    # another layout: refused by name, by the host pair and by the device pair
    C5 = make(ring_spec(R=5, N=22, junction_length=0.1, horizon=400), "f32")
    with pytest.raises(ValueError, match="layout|bytes"):
        C5.restore(blob)
    with pytest.raises(ValueError, match="layout"):
        C5.restore(blob[:int(C5.snapshot_info().host_bytes)], layout=A.snapshot_info().layout)
    # A's device blob into B: equal layout, another handle
    dblob = new_blob(A)
    A.snapshot_dev(dblob)
    A.sync()
    ia = A.snapshot_info()
    assert ia.layout == B.snapshot_info().layout and ia.nonce != B.snapshot_info().nonce and ia.nonce != 0
    rc = B.lib.fs_restore_dev(B._h, dblob.data_ptr(), int(ia.bytes), ia.layout, ia.nonce, None)
    assert rc == L.FS_ERR_INVALID and b"nonce" in B.lib.fs_last_error()
    rc = B.lib.fs_restore_dev(B._h, dblob.data_ptr(), int(ia.bytes) - 16, ia.layout, B.snapshot_info().nonce, None)
    assert rc == L.FS_ERR_INVALID and b"bytes" in B.lib.fs_last_error()
    rc = B.lib.fs_restore_dev(B._h, dblob.data_ptr(), int(ia.bytes), ia.layout ^ 1, B.snapshot_info().nonce, None)
    assert rc == L.FS_ERR_INVALID and b"layout" in B.lib.fs_last_error()
    rc = B.lib.fs_snapshot_dev(B._h, None, int(ia.bytes), None)
    assert rc == L.FS_ERR_INVALID and b"dst_dev" in B.lib.fs_last_error()
    info = L.fs_snapshot_info()
    assert B.lib.fs_snapshot_info(B._h, ctypes.byref(info)) == 0 and info.host_bytes == info.bytes + HEADER
    A.close(), B.close(), C5.close()


@pytest.mark.parametrize("name", ["ring_pair_noise", "merge_queue"])
def test_snapshot_followed_by_restore_changes_no_bit(name):
    spec, precision, env, kernels, a, b, driver_of, arrivals = case(name)
    sim = make(spec, precision, **env)
    drive = driver_of((sim,))
    sim.reset()
    drive(sim, 0, a)
    before = end_state(sim)
    blob = new_blob(sim)
    sim.snapshot_dev(blob)
    sim.restore_dev(blob)
    after = end_state(sim)
    for key in before:
        same_bits(after[key], before[key], key)
    sim.close()
