"""Per-replica inflow periods on the open networks (FS_FIELD_INFLOW_PERIOD / FS_FIELD_INIT_INFLOW_PERIOD) on the GPU: every
kernel family that reads the schedule against the oracle, bit for bit; pending periods and masked resets; resets inside a
fused launch and inside a captured graph; what is refused; VecFlowEnv's ``reset_inflow``; the capacity example.

The frozen oracle takes one period per inflow: row r of a handle is compared with an R = 1 oracle that carries replica r's
global index, initial state and periods (test_inflow_rates_cpu.py proves the method on the CPU)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import bottleneck_spec, merge_spec, ring_spec
from oracle import opennet as O
from test_inflow_rates_cpu import load_example, period_table, quiet, row_oracles, row_spec
from test_open_gpu import compare_state, make

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELD_NAMES = ("FS_FIELD_POS", "FS_FIELD_VEL", "FS_FIELD_PREV_VEL", "FS_FIELD_ROUTE", "FS_FIELD_SEQ", "FS_FIELD_ORIGIN",
               "FS_FIELD_CTL_SEQ", "FS_FIELD_COUNTERS", "FS_FIELD_TIME", "FS_FIELD_ARRIVED_RL", "FS_FIELD_INFLOW_PERIOD",
               "FS_FIELD_INIT_INFLOW_PERIOD")


def full_periods(P):
    from flow_amd import _lib as L
    full = np.zeros((P.shape[0], L.FS_MAX_INFLOWS))
    full[:, :P.shape[1]] = P
    return full


def own_periods(spec):
    return np.tile(np.array([float(f["period"]) for f in spec["inflows"]]), (int(spec["num_replicas"]), 1))


def state_of(sim):
    from flow_amd import _lib as L
    return {name: sim.get_state(getattr(L, name)).copy() for name in FIELD_NAMES}


def assert_same_state(a, b, msg=""):
    sa, sb = state_of(a), state_of(b)
    for name in FIELD_NAMES:
        np.testing.assert_array_equal(sa[name], sb[name], err_msg=msg + name)


class Rows:
    """One read of the handle's state, looked at one replica at a time by test_open_gpu.compare_state."""

    def __init__(self, sim):
        self.sim, self.cache = sim, {}

    def field(self, f):
        if f not in self.cache:
            self.cache[f] = self.sim.get_state(f)
        return self.cache[f]

    def row(self, r):
        return Row(self, r)


class Row:
    def __init__(self, rows, r):
        self.rows, self.r = rows, r

    def get_state(self, f):
        return self.rows.field(f)[self.r:self.r + 1]

    @property
    def pos(self):
        from flow_amd import _lib as L
        return self.get_state(L.FS_FIELD_POS)

    @property
    def vel(self):
        from flow_amd import _lib as L
        return self.get_state(L.FS_FIELD_VEL)

    @property
    def headway(self):
        from flow_amd import _lib as L
        return self.get_state(L.FS_FIELD_HEADWAY)


def compare_rows(sim, oracles, rows=None):
    snap = Rows(sim)
    for r in (range(len(oracles)) if rows is None else rows):
        compare_state(snap.row(r), oracles[r])


def step_against_oracles(sim, oracles, acts, kernel=None, check_every=10, first=0):
    """Observation, reward and done of every replica against its oracle at every step, the state every few steps."""
    for k in range(acts.shape[0]):
        o_gpu, r_gpu, d_gpu = sim.step(acts[k])
        if kernel is not None:
            assert sim.last_kernel.startswith(kernel), "step %d ran on %s" % (first + k, sim.last_kernel)
        for r, ora in enumerate(oracles):
            o_ref, r_ref, d_ref = ora.step(acts[k][r:r + 1])
            where = "step %d, replica %d" % (first + k, r)
            np.testing.assert_array_equal(o_gpu[r], o_ref[0].astype(np.float32), err_msg="obs, " + where)
            assert r_gpu[r] == np.float32(r_ref[0]), "reward, " + where
            assert bool(d_gpu[r]) == bool(d_ref[0]), "done, " + where
        if k % check_every == 0 or k == acts.shape[0] - 1:
            compare_rows(sim, oracles)


def random_actions(spec, K, seed, lo=-1.0, hi=1.5):
    return np.random.default_rng(seed).uniform(lo, hi, (K, int(spec["num_replicas"]), int(spec["num_rl"]))).astype(np.float32)


# ---- 1. every kernel family ---------------------------------------------------------------------------------------------
def family(name, R=None, **kw):
    """(spec, environment, kernel, oracle keywords); ``R`` / ``kw`` override the replica count / entries of the spec"""
    if name == "merge_queue_po":
        return (quiet(merge_spec(R=R or 3, cap_human=24, cap_rl=5, num_rl=2, horizon=300, seed=3, **kw)), {}, "k_merge_queue",
                {})
    if name == "merge_queue_ma":
        return (quiet(merge_spec(R=3, cap_human=24, cap_rl=5, num_rl=5, horizon=300, seed=4, env=O.ENV_MERGE_MA,
                                 ma_apply_actions=True)), {}, "k_merge_queue", {})
    if name == "steps_open_merge":            # 16 slots: four replicas to a wave, the second wave holds two
        return (quiet(merge_spec(R=6, cap_human=12, cap_rl=4, num_rl=2, horizon=300, seed=5, q_highway=1500.0)),
                {"FLOWSIM_NO_QUEUE": "1"}, "k_steps_open", {})
    if name == "steps_open_drop":
        return bottleneck_spec(R=6, cap_human=40, cap_rl=8, horizon=300, seed=6), {"FLOWSIM_NO_QUEUE": "1"}, "k_steps_open", {}
    if name == "drop_queue":
        return (bottleneck_spec(R=R or 3, cap_human=40, cap_rl=8, horizon=300, seed=7, **kw), {}, "k_drop_queue",
                dict(cell_sum="fixed"))
    if name == "steps_wide":
        return bottleneck_spec(R=3, cap_human=70, cap_rl=10, horizon=300, seed=8), {"FLOWSIM_NO_QUEUE": "1"}, "k_steps_wide", {}
    raise KeyError(name)


FAMILIES = ["merge_queue_po", "merge_queue_ma", "steps_open_merge", "steps_open_drop", "drop_queue", "steps_wide"]


@pytest.mark.parametrize("name", FAMILIES)
def test_every_replica_follows_the_oracle_with_its_own_periods(name, monkeypatch):
    from flow_amd import _lib as L
    spec, env, kernel, okw = family(name)
    for key, value in env.items():
        monkeypatch.setenv(key, value)
    K = 80
    P = period_table(spec)
    assert len({tuple(row) for row in P}) >= min(P.shape[0], 4)
    acts = random_actions(spec, K, 11)
    sim = make(spec, "f32")
    np.testing.assert_array_equal(sim.get_state(L.FS_FIELD_INFLOW_PERIOD), full_periods(own_periods(spec)))
    np.testing.assert_array_equal(sim.get_state(L.FS_FIELD_INIT_INFLOW_PERIOD), full_periods(own_periods(spec)))
    sim.set_state(L.FS_FIELD_INFLOW_PERIOD, full_periods(P))
    oracles = row_oracles(spec, P, **okw)
    obs = sim.reset()
    for r, ora in enumerate(oracles):
        np.testing.assert_array_equal(obs[r], ora.reset()[0].astype(np.float32), err_msg="reset, replica %d" % r)
    compare_rows(sim, oracles)
    step_against_oracles(sim, oracles, acts, kernel)
    departed = [int(o.total_departed[0]) for o in oracles]
    print(name, "departed per replica", departed)
    assert len(set(departed)) > 1 and min(departed) >= 1, departed
    for fld in (L.FS_FIELD_INFLOW_PERIOD, L.FS_FIELD_INIT_INFLOW_PERIOD):
        np.testing.assert_array_equal(sim.get_state(fld), full_periods(P))
    sim.close()


@pytest.mark.parametrize("name", FAMILIES)
def test_a_handle_written_with_its_own_periods_is_the_untouched_handle(name, monkeypatch):
    import torch
    from flow_amd import _lib as L
    spec, env, kernel, _ = family(name)
    for key, value in env.items():
        monkeypatch.setenv(key, value)
    K, R = 80, int(spec["num_replicas"])
    dev = torch.device("cuda", 0)
    acts = torch.from_numpy(random_actions(spec, K, 12)).to(dev)
    outs, sims = [], []
    for write in (False, True):
        sim = make(spec, "f32")
        if write:
            sim.set_state(L.FS_FIELD_INFLOW_PERIOD, sim.get_state(L.FS_FIELD_INFLOW_PERIOD))
        out = (torch.empty((K, R, sim.obs_dim), device=dev), torch.empty((K, R), device=dev),
               torch.empty((K, R), dtype=torch.uint8, device=dev))
        sim.reset()
        sim.rollout_dev(K, *out, actions=acts)
        sim.sync()
        assert sim.last_kernel.startswith(kernel), sim.last_kernel
        outs.append([t.cpu().numpy() for t in out])
        sims.append(sim)
    for what, x, y in zip(("obs", "rew", "done"), *outs):
        np.testing.assert_array_equal(x, y, err_msg=what)
    assert_same_state(*sims)
    assert int(sims[0].get_state(L.FS_FIELD_COUNTERS)[:, 6].min()) >= 2
    for sim in sims:
        sim.close()


# ---- 2. pending periods -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["merge_queue_po", "drop_queue"])
def test_pending_periods_wait_for_the_reset_of_their_replica(name):
    import torch
    from flow_amd import _lib as L
    R, K1, K2 = 4, 20, 40
    spec, _, kernel, okw = family(name, R=R, warmup_steps=3)
    dev = torch.device("cuda", 0)
    own, P2 = own_periods(spec), period_table(spec, shift=1)
    assert (P2 != own).any(axis=1).all()
    acts = random_actions(spec, K1 + K2, 13)
    plain, sim = make(spec, "f32"), make(spec, "f32")
    oracles = row_oracles(spec, None, **okw)
    o_plain, o_sim = plain.reset(), sim.reset()
    np.testing.assert_array_equal(o_plain, o_sim)
    sim.set_state(L.FS_FIELD_INIT_INFLOW_PERIOD, full_periods(P2))
    np.testing.assert_array_equal(sim.get_state(L.FS_FIELD_INFLOW_PERIOD), full_periods(own))
    np.testing.assert_array_equal(sim.get_state(L.FS_FIELD_INIT_INFLOW_PERIOD), full_periods(P2))
    for r, ora in enumerate(oracles):
        np.testing.assert_array_equal(o_plain[r], ora.reset()[0].astype(np.float32))
    # pending periods change nothing while the episode runs
    for k in range(K1):
        a, b = plain.step(acts[k]), sim.step(acts[k])
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y, err_msg="step %d" % k)
        for r, ora in enumerate(oracles):
            o_ref, r_ref, d_ref = ora.step(acts[k][r:r + 1])
            np.testing.assert_array_equal(b[0][r], o_ref[0].astype(np.float32), err_msg="obs, step %d, replica %d" % (k, r))
    for fld in ("FS_FIELD_POS", "FS_FIELD_VEL", "FS_FIELD_ROUTE", "FS_FIELD_SEQ", "FS_FIELD_ORIGIN", "FS_FIELD_COUNTERS"):
        np.testing.assert_array_equal(plain.get_state(getattr(L, fld)), sim.get_state(getattr(L, fld)), err_msg=fld)
    plain.close()
    # a masked reset, warm-up steps included: replicas 0 and 2 start again on their new periods, 1 and 3 go on
    mask = np.array([1, 0, 1, 0], dtype=np.uint8)
    obs = torch.zeros((R, sim.obs_dim), device=dev)
    torch.cuda.synchronize()
    sim.reset_dev(obs, torch.from_numpy(mask).to(dev))
    sim.sync()
    obs = obs.cpu().numpy()
    for r in np.flatnonzero(mask):
        ora = oracles[r]
        for f in range(P2.shape[1]):
            ora.inflows[f]["period"] = float(P2[r, f])
        if name == "drop_queue":        # up to 64 slots a masked reset's observation is written by k_steps_open: float sums
            ora.spec["cell_sum"] = "slot"
        o_ref = ora.reset()
        if name == "drop_queue":
            ora.spec["cell_sum"] = "fixed"
        np.testing.assert_array_equal(obs[r], o_ref[0].astype(np.float32), err_msg="masked reset, replica %d" % r)
    want = np.where(mask[:, None] != 0, P2, own)
    np.testing.assert_array_equal(sim.get_state(L.FS_FIELD_INFLOW_PERIOD), full_periods(want))
    np.testing.assert_array_equal(sim.get_state(L.FS_FIELD_INIT_INFLOW_PERIOD), full_periods(P2))
    compare_rows(sim, oracles)
    step_against_oracles(sim, oracles, acts[K1:], kernel, first=K1)
    departed = [int(o.total_departed[0]) for o in oracles]
    print(name, "departed per replica", departed)
    assert min(departed) >= 1
    np.testing.assert_array_equal(sim.get_state(L.FS_FIELD_INFLOW_PERIOD), full_periods(want))
    sim.close()


# ---- 3. resets inside a launch ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", ["po", "wide", "ma"])
def test_resets_inside_a_fused_launch_take_the_pending_periods(head):
    """k_merge_policy<PO> (MergePOEnv, two places), k_merge_policy<PO,WIDE> (13 places: the form that keeps its schedule
    in the LDS table) and the multi-agent policy form of k_merge_queue (fs_last_kernel "k_merge_policy"): horizon 12, 30
    steps, every replica reset at least twice inside the launch."""
    import torch
    from flow_amd import _lib as L
    from test_policy_gpu import eager_obs0, make_policy_in
    import test_policy_merge_gpu as MA
    import test_policy_merge_po_gpu as PO
    import test_policy_merge_wide_gpu as WIDE
    K, R = 30, 6
    dev = torch.device("cuda", 0)
    if head == "po":
        spec = merge_spec(R=R, cap_human=24, cap_rl=5, num_rl=2, horizon=12, seed=12, sims_per_step=5, q_rl=1200.0,
                          q_highway=1500.0)
        pols = [PO.make_vec_policy(2, 2, False, seed=3) for _ in range(2)]
        kernel, buffers, stagger, n_col = "k_merge_policy<PO>", (lambda: PO.buffers(K, R, 10, 2)), PO.stagger, 2
    elif head == "wide":
        spec = WIDE.wide_spec(13, R=R, seed=23, sims_per_step=5, horizon=12)
        pols = [PO.make_vec_policy(13, 2, False, seed=3) for _ in range(2)]
        kernel, buffers, stagger, n_col = WIDE.KERNEL, (lambda: PO.buffers(K, R, 65, 13)), PO.stagger, 13
        assert kernel == "k_merge_policy<PO,WIDE>"
    else:
        spec = merge_spec(R=R, cap_human=24, cap_rl=5, num_rl=5, horizon=12, seed=12, sims_per_step=5, q_rl=1200.0,
                          q_highway=1500.0, env=O.ENV_MERGE_MA, ma_apply_actions=True)
        pols = [make_policy_in(5, 2, False, seed=3) for _ in range(2)]
        kernel, buffers, stagger, n_col = "k_merge_policy", (lambda: MA.buffers(K, R, 25, 5)), MA.stagger, 5
    P1, P2 = period_table(spec, shift=1), period_table(spec, shift=2)
    assert (P1 != P2).any(axis=1).all() and (P1 != own_periods(spec)).any(axis=1).all()
    fused, eager = make(spec, "f32"), make(spec, "f32")
    for sim in (fused, eager):
        sim.set_state(L.FS_FIELD_INFLOW_PERIOD, full_periods(P1))
        stagger(sim, 3)                                   # (a reset, nine steps, a masked reset of every other replica)
        sim.set_state(L.FS_FIELD_INIT_INFLOW_PERIOD, full_periods(P2))
        np.testing.assert_array_equal(sim.get_state(L.FS_FIELD_INFLOW_PERIOD), full_periods(P1))
    f = buffers()
    fused.policy_rollout_dev(pols[0].struct, K, *f, reset_done=True)
    fused.sync()
    assert fused.last_kernel == kernel, fused.last_kernel
    e = buffers()
    eo, ea, elp, er, ed = e
    eo[0].copy_(torch.as_tensor(eager_obs0(eager), device=dev))
    torch.cuda.synchronize()
    for s in range(K):
        eager.policy_act_dev(pols[1].struct, eo[s], ea[s], elp[s])
        eager.step_dev(eo[s + 1], er[s], ed[s], ea[s])
        eager.reset_dev(eo[s + 1], ed[s])
    eager.sync()
    for what, x, y in zip(("obs", "act", "logp", "rew", "done"), f, e):
        np.testing.assert_array_equal(x.cpu().numpy(), y.cpu().numpy(), err_msg=what)
    assert_same_state(fused, eager)
    dn = f[4].cpu().numpy()
    assert ((dn != 0).sum(axis=0) >= 2).all(), "a replica was reset fewer than twice inside the launch"
    for sim in (fused, eager):
        np.testing.assert_array_equal(sim.get_state(L.FS_FIELD_INFLOW_PERIOD), full_periods(P2))
        np.testing.assert_array_equal(sim.get_state(L.FS_FIELD_INIT_INFLOW_PERIOD), full_periods(P2))
    # the periods decide what the fragment computes: the same fragment without the pending write differs
    other = make(spec, "f32")
    other.set_state(L.FS_FIELD_INFLOW_PERIOD, full_periods(P1))
    stagger(other, 3)
    g = buffers()
    pol = make_policy_in(5, 2, False, seed=3) if head == "ma" else PO.make_vec_policy(n_col, 2, False, seed=3)
    other.policy_rollout_dev(pol.struct, K, *g, reset_done=True)
    other.sync()
    assert not np.array_equal(other.get_state(L.FS_FIELD_COUNTERS), fused.get_state(L.FS_FIELD_COUNTERS))
    for sim in (fused, eager, other):
        sim.close()


def test_resets_inside_a_captured_fragment_take_the_pending_periods():
    """VecFlowEnv.capture(K, policy=DevicePolicy, reset_done=True) on the lane drop (StepGraph over a spec-built handle, as
    tests/test_policy_wide_gpu.py builds it) against the same calls made eagerly."""
    import torch
    from flow_amd import _lib as L
    import test_policy_wide_gpu as W
    K = 30
    dev = torch.device("cuda", 0)
    spec = W.quiet(W.wide_spec(6, 141, 20, horizon=12, warmup_steps=3, seed=4))
    P1, P2 = period_table(spec, shift=1), period_table(spec, shift=2)
    pol_g, pol_e = W.fragment_policies(True, 2)
    vec = W.SpecVec(spec)
    vec.sim.set_state(L.FS_FIELD_INFLOW_PERIOD, full_periods(P1))
    vec.reset()
    g = vec.capture(K, pol_g, True)
    g.synchronize()
    obs0 = vec.reset()
    vec.sim.sync()
    vec.sim.set_state(L.FS_FIELD_INIT_INFLOW_PERIOD, full_periods(P2))
    g.begin(obs0)
    o, a, r, d = g.replay()
    g.synchronize()
    torch.cuda.synchronize()
    frag = tuple(t.cpu().numpy().copy() for t in (o, a, g.logp, r, d))
    # the same calls in the same order on a twin handle
    sim = make(spec, "f32")
    R, D, A = sim.R, sim.obs_dim, sim.num_rl
    eo = torch.zeros((K + 1, R, D), device=dev)
    ea, elp, er = torch.zeros((K, R, A), device=dev), torch.zeros((K, R), device=dev), torch.zeros((K, R), device=dev)
    ed = torch.zeros((K, R), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    sim.set_state(L.FS_FIELD_INFLOW_PERIOD, full_periods(P1))
    sim.reset_dev(eo[0], None)
    for s in range(2):                                     # (the graph's warm-up; its outputs are overwritten below)
        sim.policy_act_dev(pol_e.struct, eo[s], ea[s], elp[s])
        sim.step_dev(eo[s + 1], er[s], ed[s], ea[s])
        sim.reset_dev(eo[s + 1], ed[s])
    sim.reset_dev(eo[0], None)
    sim.sync()
    sim.set_state(L.FS_FIELD_INIT_INFLOW_PERIOD, full_periods(P2))
    for s in range(K):
        sim.policy_act_dev(pol_e.struct, eo[s], ea[s], elp[s])
        assert sim.last_kernel == W.KERNEL
        sim.step_dev(eo[s + 1], er[s], ed[s], ea[s])
        assert sim.last_kernel == "k_drop_queue"
        sim.reset_dev(eo[s + 1], ed[s])
    sim.sync()
    for what, x, y in zip(("obs", "act", "logp", "rew", "done"), frag, (eo, ea, elp, er, ed)):
        np.testing.assert_array_equal(x, y.cpu().numpy(), err_msg=what)
    assert_same_state(vec.sim, sim)
    assert ((frag[4] != 0).sum(axis=0) >= 1).all(), "a replica went through the fragment without a reset"
    np.testing.assert_array_equal(sim.get_state(L.FS_FIELD_INFLOW_PERIOD), full_periods(P2))
    np.testing.assert_array_equal(vec.sim.get_state(L.FS_FIELD_INFLOW_PERIOD), full_periods(P2))
    vec.sim.close(), sim.close()


# ---- 4. refusals --------------------------------------------------------------------------------------------------------
def test_refusals_name_the_field_and_leave_the_handle_usable():
    from flow_amd import _lib as L
    fields = (("FS_FIELD_INFLOW_PERIOD", L.FS_FIELD_INFLOW_PERIOD), ("FS_FIELD_INIT_INFLOW_PERIOD", L.FS_FIELD_INIT_INFLOW_PERIOD))
    ok = np.full((2, L.FS_MAX_INFLOWS), 3.0)
    spec = quiet(merge_spec(R=2, cap_human=12, cap_rl=4, num_rl=2, horizon=100, seed=1))
    # closed networks, open ones without inflows
    for closed in (make(ring_spec(R=2), "f32"), make(dict(spec, inflows=[]), "f32")):
        for name, fld in fields:
            with pytest.raises(ValueError, match=name + ":"):
                closed.get_state(fld)
            with pytest.raises(ValueError, match=name + ":"):
                closed.set_state(fld, ok)
        closed.reset()
        closed.step(None)
        closed.close()
    # a probabilistic inflow
    fl = spec["inflows"]
    prob = make(dict(spec, inflows=[dict(fl[0], probability=0.3)] + fl[1:]), "f32")
    for name, fld in fields:
        with pytest.raises(NotImplementedError, match=name + ":.*scheduled"):
            prob.set_state(fld, ok)
        with pytest.raises(NotImplementedError, match=name + ":"):
            prob.get_state(fld)
    prob.reset()
    prob.step(None)
    prob.close()
    # periods that are no periods: nothing is written, the handle goes on as the untouched one does
    sim, twin = make(spec, "f32"), make(spec, "f32")
    before = sim.get_state(L.FS_FIELD_INFLOW_PERIOD)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        for name, fld in fields:
            val = ok.copy()
            val[1, 2] = bad
            with pytest.raises(ValueError, match=name + ":.*finite and > 0"):
                sim.set_state(fld, val)
    val = ok.copy()
    val[:, 3:] = [0.0, -1.0, float("nan"), float("inf"), -0.0]            # columns >= num_inflows are ignored ...
    sim.set_state(L.FS_FIELD_INIT_INFLOW_PERIOD, val)
    got = sim.get_state(L.FS_FIELD_INIT_INFLOW_PERIOD)
    np.testing.assert_array_equal(got[:, :3], 3.0)
    np.testing.assert_array_equal(got[:, 3:], 0.0)                         # ... and read as 0
    rc = sim.lib.fs_set_state(sim._h, L.FS_FIELD_INFLOW_PERIOD, ok.ctypes.data, ok.nbytes - 8)
    with pytest.raises(ValueError, match="FS_FIELD_INFLOW_PERIOD: wrong byte count"):
        L.check(rc, sim.lib)
    np.testing.assert_array_equal(sim.get_state(L.FS_FIELD_INFLOW_PERIOD), before)
    sim.set_state(L.FS_FIELD_INIT_INFLOW_PERIOD, before)
    np.testing.assert_array_equal(sim.reset(), twin.reset())
    acts = random_actions(spec, 30, 2)
    for k in range(30):
        for x, y in zip(sim.step(acts[k]), twin.step(acts[k])):
            np.testing.assert_array_equal(x, y)
    sim.close(), twin.close()


# ---- 5. VecFlowEnv ------------------------------------------------------------------------------------------------------
def reset_inflow_params(**kw):
    from test_bottleneck_env_gpu import c4_flow_params
    kw.setdefault("horizon", 10)
    kw.setdefault("warmup_steps", 2)
    return c4_flow_params(reset_inflow=True, **kw)


def test_vec_env_draws_an_inflow_per_replica_and_reset():
    import torch
    import warnings
    from flow_amd import _lib as L
    from flow_amd.envs import VecFlowEnv
    R = 8
    vec = VecFlowEnv(reset_inflow_params(), num_replicas=R, device=0, seed=5)
    np.testing.assert_allclose(vec.inflow_rates().sum(axis=1), 2300.0, rtol=1e-12)
    assert vec.inflow_rates().shape == (R, 2)

    def check(rates):
        tot = rates.sum(axis=1)
        assert ((tot >= 1000.0 * (1 - 1e-12)) & (tot <= 2000.0 * (1 + 1e-12))).all(), tot    # inflow_range * scaling (1)
        np.testing.assert_allclose(rates[:, 0] / tot, 0.9, rtol=1e-12)                        # human, then followerstopper
        np.testing.assert_allclose(rates[:, 1] / tot, 0.1, rtol=1e-12)
        return tot

    vec.reset()
    first = vec.inflow_rates()
    tot = check(first)
    assert len(np.unique(tot)) == R
    np.testing.assert_array_equal(vec.inflow_rates(pending=True), first)
    # a masked reset: only its replicas draw
    zeros = torch.zeros((R, vec.act_dim), device=vec.device)
    for _ in range(5):
        vec.step(zeros)
    mask = torch.tensor([1, 0] * (R // 2), dtype=torch.uint8, device=vec.device)
    vec.reset(mask)
    second = vec.inflow_rates()
    check(second)
    m = mask.cpu().numpy() != 0
    assert (second[m] != first[m]).all() and (second[~m] == first[~m]).all()
    # reset_done: the replicas that were not reset reach the horizon five steps before the others
    for _ in range(5):
        _, _, done = vec.step(zeros)
    done = done.cpu().numpy() != 0
    assert done[~m].all() and not done.all()
    vec.reset_done()
    third = vec.inflow_rates()
    check(third)
    assert (third[done] != second[done]).all() and (third[~done] == second[~done]).all()
    # redraw_inflow_rates: pending only
    vec.redraw_inflow_rates()
    np.testing.assert_array_equal(vec.inflow_rates(), third)
    pending = vec.inflow_rates(pending=True)
    check(pending)
    assert (pending != third).all()
    # set_inflow_rates: totals or one rate per inflow, now or pending
    vec.set_inflow_rates(np.linspace(1200.0, 1900.0, R), pending=True)
    np.testing.assert_array_equal(vec.inflow_rates(), third)
    np.testing.assert_allclose(vec.inflow_rates(pending=True).sum(axis=1), np.linspace(1200.0, 1900.0, R), rtol=1e-12)
    per_flow = np.column_stack([np.linspace(900.0, 1100.0, R), np.linspace(50.0, 400.0, R)])
    vec.set_inflow_rates(per_flow)
    np.testing.assert_allclose(vec.inflow_rates(), per_flow, rtol=1e-14)
    np.testing.assert_allclose(vec.inflow_rates(pending=True), per_flow, rtol=1e-14)
    for bad in (np.ones(R + 1), np.ones((R, 3)), np.zeros(R), np.full((R, 2), np.nan)):
        with pytest.raises(ValueError):
            vec.set_inflow_rates(bad)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        vec.reset()
        g = vec.capture(3, policy=None, reset_done=True)
        g.synchronize()
        vec.capture(3, policy=None, reset_done=True).synchronize()
    assert sum("redraw_inflow_rates" in str(w.message) for w in seen) == 1
    vec.close()
    # without reset_inflow nothing is drawn
    quiet_vec = VecFlowEnv(no_reset_inflow_params(), num_replicas=4, device=0, seed=5)
    quiet_vec.reset()
    quiet_vec.redraw_inflow_rates()
    np.testing.assert_allclose(quiet_vec.inflow_rates().sum(axis=1), 2300.0, rtol=1e-12)
    np.testing.assert_array_equal(quiet_vec.inflow_rates(pending=True), quiet_vec.inflow_rates())
    quiet_vec.close()


def no_reset_inflow_params():
    from test_bottleneck_env_gpu import c4_flow_params
    return c4_flow_params(horizon=10, warmup_steps=2, reset_inflow=False)


def test_train_on_device_redraws_the_inflow_between_fragments(monkeypatch):
    import math
    from flow_amd.envs import VecFlowEnv
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_vec
    seen = {}
    redraw, close = VecFlowEnv.redraw_inflow_rates, VecFlowEnv.close

    def redraw_and_note(self):
        seen.setdefault("first", self.inflow_rates())
        seen["redraws"] = seen.get("redraws", 0) + 1
        return redraw(self)

    def note_and_close(self):
        seen["last"] = self.inflow_rates()
        return close(self)

    monkeypatch.setattr(VecFlowEnv, "redraw_inflow_rates", redraw_and_note)
    monkeypatch.setattr(VecFlowEnv, "close", note_and_close)
    hist = train_vec.train_on_device(reset_inflow_params(), iterations=2, fragment=12, replicas=32,
                                     fuse_action_vector=True, log=lambda line: None)
    assert len(hist) == 2 and all(math.isfinite(h) for h in hist)
    assert seen["redraws"] == 2 and seen["first"].shape == (32, 2)
    assert (seen["last"] != seen["first"]).any(axis=1).any(), "no replica ended the run at another rate than its first"
    tot = seen["last"].sum(axis=1)
    assert ((tot >= 1000.0 * (1 - 1e-12)) & (tot <= 2000.0 * (1 + 1e-12))).all()


# ---- 6. the example -----------------------------------------------------------------------------------------------------
def test_capacity_example_runs_one_rate_per_replica(tmp_path):
    out = tmp_path / "sweep"
    argv = ["--rates", "600", "2400", "--trials", "2", "--steps", "120", "--max_vehicles", "64", "--out", str(out)]
    run = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "bottleneck_capacity.py")] + argv, cwd=str(tmp_path),
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    io = np.loadtxt(str(out / "inflows_outflows.csv"), delimiter=",", ndmin=2)
    rets = np.loadtxt(str(out / "rets.csv"), delimiter=",", ndmin=2)
    assert io.shape == (4, 2) and rets.shape == (2, 2)
    np.testing.assert_array_equal(io[:, 0], [600, 600, 2400, 2400])
    np.testing.assert_array_equal(rets[:, 0], [600, 2400])
    np.testing.assert_allclose(rets[:, 1], io[:, 1].reshape(2, 2).mean(axis=1), rtol=1e-15)
    # the same sweep in this process: what the handle holds, and every replica against its own oracle
    ex = load_example()
    res = ex.run_sweep([600.0, 2400.0], 2, 120, seed=0, max_vehicles=64)
    np.testing.assert_array_equal(res["outflow"], io[:, 1])
    np.testing.assert_allclose(res["rates_read_back"], [600, 600, 2400, 2400], rtol=1e-14)
    spec = res["spec"]
    assert int(spec["num_replicas"]) == 4 and len(spec["inflows"]) == 1
    rep = np.loadtxt(open(str(out / "replicas.csv")).read().splitlines()[1:], delimiter=",", ndmin=2)
    for r in range(4):
        ora = O.MergeOracle(row_spec(spec, r, res["periods"][r]), np.float32)
        ora.reset()
        for _ in range(120):
            ora.step(None)
        assert int(ora.total_departed[0]) == int(res["entered"][r]) == int(rep[r, 3]), "departed, replica %d" % r
        assert int(ora.total_arrived[0]) * 60.0 == res["outflow"][r], "arrived, replica %d" % r      # 3600 / (120 * 0.5 s)
        assert int(ora.total_dropped[0]) == int(res["dropped"][r]) == int(rep[r, 4])
    assert res["entered"][2:].min() > res["entered"][:2].max()
