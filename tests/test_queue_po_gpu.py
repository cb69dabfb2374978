"""MergePOEnv (FS_ENV_MERGE_PO, the single-agent merge head) on the queue-order kernel k_merge_queue: bit for bit against
oracle/opennet.py (float32, through the C ABI) and against the slot-order kernel k_steps_open.  What the head adds to
the kernel -- the list rl_veh (ctl_seq, the join counter, ghosts, the skipping removal pass), the place -> action column
mapping that moves between sub-steps, the observation by place, the reward summed in list order, collisions that end
the env step -- is what these runs are chosen to exercise; every run asserts that it stepped on k_merge_queue."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from helpers import idm_vehicle, merge_spec                                             # noqa: E402
from oracle import opennet as O                                                         # noqa: E402
from oracle import refsim as S                                                          # noqa: E402
from test_open_gpu import compare_state, make, quiet, uniform_actions                   # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_queue(spec, steps, action_fn=None, check_every=10, stats=None):
    """test_open_gpu.run_pair (reset, then `steps` steps against the oracle: observation, reward, done every step, the
    state every `check_every`-th) with the kernel of every step asserted; `stats` collects what the run exercised."""
    ora = O.MergeOracle(spec, np.float32)
    sim = make(spec, "f32")
    np.testing.assert_array_equal(sim.reset(), ora.reset().astype(np.float32))
    compare_state(sim, ora)
    limit = spec.get("sims_per_step", 1) * (spec.get("warmup_steps", 0) + spec["horizon"])
    for k in range(steps):
        a = None if action_fn is None else action_fn(k)
        o_ref, r_ref, d_ref = ora.step(a)
        o_gpu, r_gpu, d_gpu = sim.step(a)
        assert sim.last_kernel == "k_merge_queue", "step %d ran on %s" % (k, sim.last_kernel)
        np.testing.assert_array_equal(o_gpu, o_ref.astype(np.float32), err_msg="obs, step %d" % k)
        np.testing.assert_array_equal(r_gpu, r_ref.astype(np.float32), err_msg="reward, step %d" % k)
        np.testing.assert_array_equal(d_gpu, d_ref, err_msg="done, step %d" % k)
        if stats is not None:
            crashed = d_ref & (ora.time_counter < limit)
            stats["crashed"] = stats.get("crashed", 0) + int(crashed.sum())
            stats["ghost_steps"] = stats.get("ghost_steps", 0) + int((o_ref[:, 0::5] < -30).any())
            if crashed.any():
                np.testing.assert_array_equal(r_gpu[crashed], 0.0)
                assert ((sim.last_done_flags[crashed] & 2) != 0).all()      # the collision bit of the flag byte
        if k % check_every == 0 or k == steps - 1:
            compare_state(sim, ora)
    np.testing.assert_array_equal(sim.time_counter, ora.time_counter)
    sim.close()
    return ora


def test_po_life_cycle_three_generations_of_a_two_place_list():
    spec = quiet(merge_spec(R=5, cap_human=26, cap_rl=5, num_rl=2, horizon=500, seed=3))
    stats = {}
    ora = run_queue(spec, 500, uniform_actions(spec, 7, 0.0, 1.5), stats=stats)
    assert (ora.ctl_ctr > 2).all()                       # RL vehicles joined and left rl_veh
    assert ora.total_departed.min() > 20 and ora.total_arrived.min() > 5
    assert stats["ghost_steps"] >= 1                     # a listed vehicle had left when the observation was taken


@pytest.mark.parametrize("seed", [3, 4, 5])
def test_po_collisions_end_the_env_step(seed):
    """Speed mode 0 everywhere: nothing keeps the vehicles apart.  A collision freezes the replica's remaining sub-steps
    of the env step (sims_per_step 1 / 2 / 3), gives reward 0 and the crash bit; the re-sort runs with the list in place."""
    spec = quiet(merge_spec(R=4, cap_human=18 + seed, cap_rl=4, num_rl=3, horizon=300, seed=seed, pre=150.0,
                            q_highway=1500 + 100 * seed, q_merge=200 + 80 * seed, sims_per_step=1 + seed % 3))
    spec["vehicles"] = [dict(v, speed_mode=0) for v in spec["vehicles"]]
    rng = np.random.default_rng(seed)
    stats = {}
    run_queue(spec, 300, lambda k: rng.uniform(-1.0, 1.5, (4, 3)).astype(np.float32), check_every=7, stats=stats)
    assert stats["crashed"] >= 100


def test_po_the_experiment_s_shape_64_slots_five_sub_steps():
    spec = quiet(merge_spec(R=2, cap_human=54, cap_rl=10, num_rl=5, pre=500.0, merge=200.0, post=100.0, horizon=600, seed=1,
                            q_highway=1800.0, q_rl=200.0, q_merge=100.0, n_init=5, sims_per_step=5))
    rng = np.random.default_rng(9)
    ora = run_queue(spec, 300, lambda k: rng.uniform(-1.5, 1.5, (2, 5)).astype(np.float32))
    assert ora.total_departed.min() > 50 and ora.total_arrived.min() > 30


def test_po_rl_veh_survives_reset_and_skips_while_removing():
    """tests/test_open_gpu.py::test_merge_po_rl_veh_survives_reset_and_skips_while_removing_bit_exact on the queue kernel:
    the list outlives reset() (k_reset_open keeps the entries), the next launch loads it, and the removal pass skips."""
    spec = quiet(merge_spec(R=7, cap_human=10, cap_rl=8, num_rl=4, horizon=10 ** 6, seed=5, q_rl=1500.0, q_highway=600.0))
    ora = O.MergeOracle(spec, np.float32)
    sim = make(spec, "f32")
    act = uniform_actions(spec, 3, lo=-0.5, hi=1.0)
    np.testing.assert_array_equal(sim.reset(), ora.reset().astype(np.float32))
    ghost_steps = 0
    for episode in range(3):
        for k in range(200):
            a = act(k)
            o_ref, r_ref, d_ref = ora.step(a)
            o_gpu, r_gpu, d_gpu = sim.step(a)
            assert sim.last_kernel == "k_merge_queue"
            np.testing.assert_array_equal(o_gpu, o_ref.astype(np.float32), err_msg="episode %d step %d" % (episode, k))
            np.testing.assert_array_equal(r_gpu, r_ref.astype(np.float32))
            if episode > 0 and k < 4:
                ghost_steps += int((o_ref[:, 0::5] < -30).any())
        compare_state(sim, ora)
        assert ((ora.ctl_seq >= 0).sum(axis=1) == 4).all()
        o_reset = ora.reset().astype(np.float32)
        np.testing.assert_array_equal(sim.reset(), o_reset)
        assert (o_reset[:, 0::5] < -30).all()                      # four stale entries: four rows of error values
        compare_state(sim, ora)
    assert ghost_steps >= 2                                        # the skipped entries outlive the first pass
    sim.close()


def test_po_rollout_equals_stepping_and_the_slot_order_kernel_with_noise(monkeypatch):
    """One K-step launch == K one-step launches == the slot-order kernel, noise included (GPU against GPU: every array,
    free slots too; the list and its counter in every slot)."""
    import torch
    from flow_amd import _lib as L
    spec = merge_spec(R=6, cap_human=24, cap_rl=5, num_rl=3, horizon=300, seed=14, sims_per_step=2)
    K, R, A = 150, 6, 3
    rng = np.random.default_rng(3)
    acts = rng.uniform(-1.0, 1.5, (K, R, A)).astype(np.float32)
    dev = torch.device("cuda:0")

    def rollout(sim):
        out = (torch.empty((K, R, sim.obs_dim), dtype=torch.float32, device=dev),
               torch.empty((K, R), dtype=torch.float32, device=dev), torch.empty((K, R), dtype=torch.uint8, device=dev))
        sim.reset()
        sim.rollout_dev(K, *out, actions=torch.from_numpy(acts).to(dev))
        sim.sync()
        return [t.cpu().numpy() for t in out]

    a = make(spec, "f32")
    ra = rollout(a)
    assert a.last_kernel == "k_merge_queue"
    b = make(spec, "f32")
    b.reset()
    for k in range(K):
        o, r, d = b.step(acts[k])
        np.testing.assert_array_equal(ra[0][k], o, err_msg="obs %d" % k)
        np.testing.assert_array_equal(ra[1][k], r)
        np.testing.assert_array_equal(ra[2][k].astype(bool), d)
    assert b.last_kernel == "k_merge_queue"
    monkeypatch.setenv("FLOWSIM_NO_QUEUE", "1")
    c = make(spec, "f32")
    rc = rollout(c)
    assert c.last_kernel == "k_steps_open"
    for x, y in zip(ra, rc):
        np.testing.assert_array_equal(x, y)
    fields = (L.FS_FIELD_POS, L.FS_FIELD_VEL, L.FS_FIELD_PREV_VEL, L.FS_FIELD_ACCEL, L.FS_FIELD_ROUTE, L.FS_FIELD_SEQ,
              L.FS_FIELD_ORIGIN, L.FS_FIELD_FOLLOWER, L.FS_FIELD_LEADER, L.FS_FIELD_HEADWAY, L.FS_FIELD_ARRIVED_RL,
              L.FS_FIELD_COUNTERS, L.FS_FIELD_MAX_SPEED, L.FS_FIELD_CTL_SEQ)
    alive = a.get_state(L.FS_FIELD_ROUTE) >= 0
    assert (a.get_state(L.FS_FIELD_COUNTERS)[:, 2] > 0).all()          # the list was in use
    for f in fields:
        fa, fb, fc = a.get_state(f), b.get_state(f), c.get_state(f)
        np.testing.assert_array_equal(fa, fb, err_msg="rollout vs stepping, field %d" % f)
        if f in (L.FS_FIELD_COUNTERS, L.FS_FIELD_ROUTE, L.FS_FIELD_ARRIVED_RL, L.FS_FIELD_CTL_SEQ):
            np.testing.assert_array_equal(fa, fc, err_msg="queue vs slot order, field %d" % f)
        else:
            np.testing.assert_array_equal(fa[alive], fc[alive], err_msg="queue vs slot order, field %d" % f)
    a.close(), b.close(), c.close()


def test_po_half_precision_state_on_both_kernels(monkeypatch):
    """FS_F16S (fp16 state between launches, float32 inside): the head comes along with the kernel's load / store of the
    halves -- the same 100-step launch on k_merge_queue and on k_steps_open."""
    import torch
    from flow_amd import _lib as L
    spec = merge_spec(R=4, cap_human=24, cap_rl=5, num_rl=3, horizon=200, seed=9, sims_per_step=5)
    K, R = 100, 4
    dev = torch.device("cuda:0")
    acts = torch.from_numpy(np.random.default_rng(5).uniform(-1.0, 1.5, (K, R, 3)).astype(np.float32)).to(dev)
    res = []
    for no_queue in ("0", "1"):
        monkeypatch.setenv("FLOWSIM_NO_QUEUE", no_queue)
        sim = make(spec, "f16s")
        out = (torch.empty((K, R, sim.obs_dim), dtype=torch.float32, device=dev),
               torch.empty((K, R), dtype=torch.float32, device=dev), torch.empty((K, R), dtype=torch.uint8, device=dev))
        sim.reset()
        sim.rollout_dev(K, *out, actions=acts)
        sim.sync()
        res.append(([t.cpu().numpy() for t in out], None, None, sim.get_state(L.FS_FIELD_CTL_SEQ),
                    sim.get_state(L.FS_FIELD_COUNTERS), sim.last_kernel))
        sim.close()
    assert res[0][5] == "k_merge_queue" and res[1][5] == "k_steps_open"
    for x, y in zip(res[0][0], res[1][0]):
        np.testing.assert_array_equal(x, y)
    for i in (3, 4):                                   # the list and the counters, every slot
        np.testing.assert_array_equal(res[0][i], res[1][i])
    assert (res[0][4][:, 2] > 0).all()


def test_po_dispatch_edges_stay_bit_exact():
    """Warm-up and masked resets (their launches carry a replica mask: k_steps_open), evaluate = True, one controlled
    place over pools that overflow: bit-exact against the oracle whichever kernel a launch takes, and the plain steps in
    between are k_merge_queue's."""
    spec = quiet(merge_spec(R=4, cap_human=12, cap_rl=4, num_rl=3, horizon=60, seed=9, sims_per_step=5, warmup_steps=7))
    run_queue(spec, 60, uniform_actions(spec, 2, 0.2, 1.5), check_every=5)
    spec = quiet(merge_spec(R=3, cap_human=14, cap_rl=4, num_rl=2, horizon=150, seed=2, evaluate=True))
    run_queue(spec, 150, uniform_actions(spec, 8))
    spec = quiet(merge_spec(R=19, cap_human=6, cap_rl=2, num_rl=1, horizon=300, seed=5, pre=120.0, q_highway=1500.0))
    run_queue(spec, 300, uniform_actions(spec, 11))
    # a masked reset in the middle of a run
    spec = quiet(merge_spec(R=6, cap_human=12, cap_rl=3, num_rl=2, horizon=100, seed=2))
    ora = O.MergeOracle(spec, np.float32)
    sim = make(spec, "f32")
    np.testing.assert_array_equal(sim.reset(), ora.reset().astype(np.float32))
    acts = uniform_actions(spec, 4, 0.0, 1.5)
    for k in range(80):
        a = acts(k)
        ora.step(a), sim.step(a)
    mask = np.array([1, 0, 0, 1, 0, 1], dtype=bool)
    np.testing.assert_array_equal(sim.reset(mask), ora.reset(mask).astype(np.float32))
    compare_state(sim, ora)
    for k in range(60):
        a = acts(k)
        o_ref, r_ref, d_ref = ora.step(a)
        o_gpu, r_gpu, d_gpu = sim.step(a)
        assert sim.last_kernel == "k_merge_queue"
        np.testing.assert_array_equal(o_gpu, o_ref.astype(np.float32))
        np.testing.assert_array_equal(r_gpu, r_ref.astype(np.float32))
        np.testing.assert_array_equal(d_gpu, d_ref)
    compare_state(sim, ora)
    sim.close()


def test_po_no_actions_means_sumo_drives_the_rl_vehicles():
    spec = quiet(merge_spec(R=3, cap_human=12, cap_rl=4, num_rl=2, horizon=200, seed=1))
    run_queue(spec, 200, None)


def test_po_fused_policy_is_refused_by_name():
    import torch
    from test_policy_gpu import make_policy_in
    spec = quiet(merge_spec(R=4, cap_human=12, cap_rl=3, num_rl=2, horizon=100, seed=1))
    sim = make(spec, "f32")
    sim.reset()
    pol = make_policy_in(5, 2, False, seed=1)
    dev = torch.device("cuda", 0)
    K, R = 3, 4
    out = (torch.zeros((K + 1, R, sim.obs_dim), device=dev), torch.zeros((K, R, 2), device=dev),
           torch.zeros((K, R, 2), device=dev), torch.zeros((K, R), device=dev),
           torch.zeros((K, R), dtype=torch.uint8, device=dev))
    # (flow_amd._lib.check raises NotImplementedError for FS_ERR_UNSUPPORTED alone, with fs_last_error as its text)
    with pytest.raises(NotImplementedError, match="FS_ENV_MERGE_PO"):
        sim.policy_rollout_dev(pol.struct, K, *out, reset_done=True)
    assert "FS_ENV_MERGE_PO" in sim.lib.fs_last_error().decode()
    with pytest.raises(NotImplementedError, match="FS_ENV_MERGE_PO"):
        sim.policy_act_dev(pol.struct, out[0][0], out[1][0], out[2][0])
    sim.close()


def singleagent_merge_params():
    import copy
    import importlib
    import flow_amd
    flow_amd.install_as_flow()                     # the experiment files import `flow.*` as the reference's do
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    fp = dict(importlib.import_module("exp_configs.rl.singleagent.singleagent_merge").flow_params)
    fp["sim"] = copy.deepcopy(fp["sim"])
    return fp


def test_singleagent_merge_full_size_sampled_replicas_equal_the_oracle():
    """examples/exp_configs/rl/singleagent/singleagent_merge.py as shipped (IDM noise 0.2; noise_math = 'exact' makes the
    Box-Muller draws fixed float32 sequences, the same in the numpy oracle) at 1024 replicas, 350 steps in one launch,
    two sampled replicas bit for bit.  The oracle reports 163 / 104 departures and 139 / 92 arrivals for the two replicas
    (fewer than the multi-agent C5 run's 150 / 60 floor allows for: a collision ends the env step on this head, so a
    replica that collides often runs fewer sub-steps); the floor asserted is two thirds of the smaller figures."""
    from test_full_size_gpu import sampled_parity
    fp = singleagent_merge_params()
    fp["sim"].noise_math = "exact"
    fp["sim"].seed = 11
    kernel, ora = sampled_parity(fp, R=1024, K=350, rows=[301, 1023], act_seed=4)
    assert kernel == "k_merge_queue"
    print("departed", ora.total_departed, "arrived", ora.total_arrived, "ctl_ctr", ora.ctl_ctr)
    assert ora.total_departed.min() >= 69 and ora.total_arrived.min() >= 61 and (ora.ctl_ctr >= 3).all()


def test_train_singleagent_merge_on_device_rolls_out_through_the_captured_graph():
    """`python examples/train.py singleagent_merge --rl_trainer device`: no fused policy for this head, so the fragment
    is the captured graph of single steps around the torch GaussianPolicy(25, 5); two PPO iterations run."""
    import math
    singleagent_merge_params()                     # (sys.path, flow_amd as `flow`)
    train = __import__("train")
    log = []
    module, multiagent = train.load_experiment("singleagent_merge")
    flags = train.parse_args(["singleagent_merge", "--rl_trainer", "device", "--num_steps", "2", "--rollout_size", "12",
                              "--replicas", "48"])
    from train_vec import train_on_device
    fp = module.flow_params
    history = train_on_device(fp, replicas=flags.replicas, fragment=flags.rollout_size, iterations=flags.num_steps,
                              shared_agents=multiagent, log=log.append)
    assert not multiagent and len(history) == 2 and all(math.isfinite(h) for h in history)
    assert log[0].startswith("rollout: HIP graph of 12 single steps around the torch policy"), log[0]


# ---------------------------------------------------------------------------------------------------------------------
def random_po_spec(seed):
    """The knobs of test_open_gpu.random_open_spec's merge branch on the MergePOEnv head, with the human slots drawn from
    what Sim::queue_ok takes (IDM with delta = 4, SimCarFollowingController, no fail-safe) and warmup_steps = 0."""
    rng = np.random.default_rng(7000 + seed)
    R = int(rng.integers(1, 9))
    cap_rl = int(rng.integers(1, 6))
    cap_h = int(rng.choice([6, 11, 14, 27, 40]))
    num_rl = int(rng.integers(1, cap_rl + 1))
    spec = quiet(merge_spec(R=R, cap_human=cap_h, cap_rl=cap_rl, num_rl=num_rl, pre=float(rng.choice([80, 200, 500])),
                            merge=float(rng.choice([60, 100])), post=float(rng.choice([50, 100])),
                            horizon=int(rng.integers(40, 200)), seed=seed,
                            q_highway=float(rng.choice([600, 1500, 2400])), q_rl=float(rng.choice([150, 400, 900])),
                            q_merge=float(rng.choice([100, 400, 900])), n_init=int(rng.integers(0, 4)),
                            time_gap=float(rng.choice([0.5, 1.0, 3.0])), sims_per_step=int(rng.choice([1, 1, 2, 5])),
                            crash_gap=float(rng.choice([0.0, 0.5])), slowdown_ramp=float(rng.choice([1.0, 0.2 / 0.201]))))
    spec["junction"]["enabled"] = int(rng.integers(0, 2))
    veh = spec["vehicles"]
    for i in range(cap_h):
        if int(rng.integers(0, 4)) == 1:
            veh[i] = idm_vehicle(controller=S.CTRL_SIM, speed_mode=int(rng.choice([0, 1, 7, 25, 31])), type=0)
        else:
            veh[i] = idm_vehicle(p=[float(rng.uniform(15, 30)), 1, float(rng.uniform(0.8, 2)), 1.5, 4, 2, 0, 0],
                                 speed_mode=int(rng.choice([0, 1, 3])), type=0)
    acts = (lambda k, r=np.random.default_rng(seed): r.uniform(-1.0, 1.5, (R, num_rl)).astype(np.float32))
    return spec, acts


@pytest.mark.parametrize("seed", range(10))
def test_po_fuzz_random_configs_on_the_queue_kernel_bit_exact(seed):
    spec, acts = random_po_spec(seed)
    steps = int(spec["horizon"])
    run_queue(spec, steps, acts if seed % 5 else None, check_every=max(1, steps // 4))
