"""Policy populations (include/flowsim.h fs_population; flowsim_policy.h policy_member_weights): M weight sets in ONE
launch of the scalar-head policy kernels, a workgroup loading the set of its member.

* rows [m group, (m + 1) group) of a population fragment equal, bit for bit, the same rows of fs_policy_rollout_dev with
  weight set m on an identically created handle -- the single-agent ring (sampling and greedy), the shared-agent ring,
  lord_of_the_rings' head, the figure eight with the AccelEnv head (28 inputs: the WIDE first layer) and the PO head;
* stride 0 and members = 1 equal fs_policy_rollout_dev on every row; K x (population_act, step, reset(done)) equals the
  fused fragment; two runs give the same bits; fs_last_kernel names the population kernel;
* every refusal is made by name before anything launches and leaves the handle as it was.

Shapes: R = 64 replicas, group = the granule (16), M = 4 random weight sets, K = 12 steps, horizon 7 with warm-up steps
where the head allows them, so that resets and warm-up fall inside the fragment."""
import ctypes as C

import numpy as np
import pytest

from oracle import opennet as O
from oracle import refsim as S
from helpers import merge_spec
from multi_ring_ref import multi_ring_spec
from test_multiagent_ring_gpu import ma_ring_experiment_spec
from test_policy_gpu import eager_obs0, fig8_rl_spec, make_policy_in
from test_ringrl_gpu import make, rl_ring_spec

pytestmark = pytest.mark.gpu

R, M, G, K = 64, 4, 16, 12
NAMES = ("obs", "act", "logp", "rew", "done")


def ring():
    return rl_ring_spec(R=R, N=22, noise=0.2, warmup=3, horizon=7, seed=21)


def ma_ring():
    spec = ma_ring_experiment_spec(S.ENV_WAVE_ATTENUATION_PO_MA, R, (0, 11), noise=0.2, N=22)
    spec["warmup_steps"], spec["horizon"] = 3, 7
    return spec


def lord():
    return multi_ring_spec(R=R, N=22, noise=0.2, warmup=3, horizon=7, seed=5)


def fig8(head):
    return fig8_rl_spec(R, head, 0.2, horizon=7, seed=4)        # (resets inside a fragment: warmup_steps = 0 on loops)


def policies(in_dim, num_hidden=3, free=False, seed=0):
    """M policies of one model class, one seed of the sampling streams, and their weight sets [M, stride] with a stride
    that is neither the policy's size nor a multiple of four."""
    import torch
    pols = [make_policy_in(in_dim, num_hidden, free, seed=seed + 10 * m) for m in range(M)]
    for p in pols:
        p.struct.seed = 4242
    P = pols[0].buf.numel()
    stride = P + 5
    w = torch.full((M, stride), float("nan"), device=pols[0].buf.device)      # (the padding is never read)
    for m, p in enumerate(pols):
        w[m, :P] = p.buf
    torch.cuda.synchronize()
    return pols, w.contiguous()


def buffers(sim, n_ag):
    import torch
    dev = torch.device("cuda", 0)
    per = (K, sim.R) if n_ag == 1 else (K, sim.R, n_ag)
    out = (torch.zeros((K + 1, sim.R, sim.obs_dim), device=dev), torch.zeros(per, device=dev), torch.zeros(per, device=dev),
           torch.zeros((K, sim.R), device=dev), torch.zeros((K, sim.R), dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()          # (the handles launch on streams of their own)
    return out


def host(out):
    return [t.cpu().numpy() for t in out]


def fragment(spec, pol, n_ag, pop=None):
    """One fragment of K steps with resets on a fresh handle: fs_population_rollout_dev (pop = (population, weights)) or
    fs_policy_rollout_dev; returns the five arrays, the final state and the kernel's name."""
    sim = make(spec, "f32")
    sim.reset()
    out = buffers(sim, n_ag)
    if pop is None:
        sim.policy_rollout_dev(pol.struct, K, *out, reset_done=True)
    else:
        sim.population_rollout_dev(pop.policy_struct(), pop.struct, K, *out, reset_done=True)
    sim.sync()
    res = host(out), (sim.pos.copy(), sim.vel.copy(), sim.time_counter.copy()), sim.last_kernel
    sim.close()
    return res


def check_members(spec, in_dim, n_ag, kernel, num_hidden=3, free=False, greedy=False):
    pols, w = policies(in_dim, num_hidden, free)
    for p in pols:
        p.greedy = greedy
    sim = make(spec, "f32")
    assert sim.population_granule(pols[0].struct) == G
    sim.close()
    got, state, name = fragment(spec, pols[0], n_ag, pop=pols[0].population(w, M, G))
    assert name == kernel
    assert (got[4] != 0).sum() >= R                           # episodes ended (and were reset) inside the fragment
    for m in range(M):
        want, wstate, wname = fragment(spec, pols[m], n_ag)
        assert wname + "<Population>" == kernel or wname[:-1] + ",Population>" == kernel
        rows = slice(m * G, (m + 1) * G)
        for nm, x, y in zip(NAMES, got, want):
            np.testing.assert_array_equal(x[:, rows], y[:, rows], err_msg="%s of member %d" % (nm, m))
        for x, y in zip(state, wstate):
            np.testing.assert_array_equal(x[rows], y[rows])
    # the members differ: the rows of member 1 are not what member 0's weights give
    want0 = fragment(spec, pols[0], n_ag)[0]
    assert not np.array_equal(got[1][:, G:2 * G], want0[1][:, G:2 * G])
    return got


@pytest.mark.parametrize("greedy", [False, True])
def test_singleagent_ring_members_equal_their_own_rollouts(greedy):
    check_members(ring(), 3, 1, "k_ring_policy<Population>", greedy=greedy)


@pytest.mark.parametrize("case", ["shared_ring", "lord", "fig8_accel", "fig8_po"])
def test_other_heads_members_equal_their_own_rollouts(case):
    if case == "shared_ring":
        check_members(ma_ring(), 3, 2, "k_ring_policy<POMA,Population>", num_hidden=2)
    elif case == "lord":
        check_members(lord(), 3, 1, "k_ring_policy<MultiRing,Population>", num_hidden=2, free=True)
    elif case == "fig8_accel":
        check_members(fig8("accel"), 28, 1, "k_loop_policy<Population>")
    else:
        check_members(fig8("po"), 3, 1, "k_loop_policy<Population>", num_hidden=1, free=True)


def test_shared_weights_equal_the_single_policy_rollout():
    import torch
    spec = ring()
    pols, w = policies(3)
    want = fragment(spec, pols[0], 1)[0]
    shared = pols[0].population(pols[0].buf, M, G)             # stride 0: all members share set 0
    assert shared.struct.stride == 0
    one = pols[0].population(w[:1].contiguous(), 1, R)         # members = 1, group = R
    torch.cuda.synchronize()
    for pop in (shared, one):
        got = fragment(spec, pols[0], 1, pop=pop)[0]
        for nm, x, y in zip(NAMES, got, want):
            np.testing.assert_array_equal(x, y, err_msg=nm)


def test_eager_population_act_equals_the_fused_fragment_and_runs_repeat():
    import torch
    dev = torch.device("cuda", 0)
    spec = ring()
    pols, w = policies(3)
    pop = pols[0].population(w, M, G)
    got, state, name = fragment(spec, pols[0], 1, pop=pop)
    again, state2, _ = fragment(spec, pols[0], 1, pop=pop)
    for nm, x, y in zip(NAMES, got, again):                    # determinism: the same bits twice
        np.testing.assert_array_equal(x, y, err_msg=nm)
    assert name == "k_ring_policy<Population>"
    eager = make(spec, "f32")
    eager.reset()
    eo, ea, elp, er, ed = buffers(eager, 1)
    eo[0].copy_(torch.as_tensor(eager_obs0(eager), device=dev))
    torch.cuda.synchronize()
    for k in range(K):
        eager.population_act_dev(pop.policy_struct(), pop.struct, eo[k], ea[k], elp[k])
        assert eager.last_kernel == "k_policy_act<Population>"
        eager.step_dev(eo[k + 1], er[k], ed[k], ea[k].reshape(R, 1))
        eager.reset_dev(eo[k + 1], ed[k])
    eager.sync()
    for nm, x, y in zip(NAMES, got, host((eo, ea, elp, er, ed))):
        np.testing.assert_array_equal(x, y, err_msg=nm)
    np.testing.assert_array_equal(state[0], eager.pos)
    np.testing.assert_array_equal(state[1], eager.vel)
    eager.close()


def test_refusals_are_made_by_name_and_leave_the_handle_alone():
    import torch
    from flow_amd import _lib as L
    from test_policy_wide_gpu import wide_spec
    spec = ring()
    pols, w = policies(3)
    P = pols[0].buf.numel()
    want = fragment(spec, pols[0], 1, pop=pols[0].population(w, M, G))[0]
    sim = make(spec, "f32")
    sim.reset()
    before = (sim.pos.copy(), sim.vel.copy(), sim.time_counter.copy())
    out = buffers(sim, 1)
    ps = pols[0].population(w, M, G).policy_struct()

    def pop(members, group, stride):
        return L.fs_population(struct_size=C.sizeof(L.fs_population), members=members, group=group, reserved=0, stride=stride)
    stride = int(w.shape[1])
    for bad, exc, text in ((pop(8, 8, stride), ValueError, "fs_population: group is not a multiple of the granule"),
                           (pop(3, G, stride), ValueError, "fs_population: members * group != num_replicas"),
                           (pop(M, G, P - 1), ValueError, "fs_population: stride is smaller than the policy's own size"),
                           (pop(M, G, 1), ValueError, "fs_population: stride is smaller than the policy's own size")):
        with pytest.raises(exc, match=text.replace("*", r"\*")):
            sim.population_rollout_dev(ps, bad, K, *out, reset_done=True)
        with pytest.raises(exc, match=text.replace("*", r"\*")):
            sim.population_act_dev(ps, bad, out[0][0], out[1][0], out[2][0])
    bad_size = pop(M, G, stride)
    bad_size.struct_size = 8
    with pytest.raises(ValueError, match="fs_population: struct_size mismatch"):
        sim.population_rollout_dev(ps, bad_size, K, *out, reset_done=True)
    # what fs_policy_rollout_dev refuses on this handle: a policy of another observation
    wrong = make_policy_in(5, 3, False, seed=1)
    with pytest.raises(NotImplementedError, match=r"fs_policy: not built for this handle: fs_policy.obs_dim \(3\)"):
        sim.population_rollout_dev(wrong.struct, pop(M, G, wrong.buf.numel()), K, *out, reset_done=True)
    with pytest.raises(NotImplementedError, match="fs_policy: not built for this handle"):
        sim.population_granule(wrong.struct)
    sim.sync()
    for x, y in zip(before, (sim.pos, sim.vel, sim.time_counter)):
        np.testing.assert_array_equal(x, y)
    assert float(out[0].abs().sum()) == 0.0 and int(out[4].sum()) == 0          # nothing was written
    # ... and the handle's streams and counters are where they were: the fragment it runs now is the fresh handle's
    sim.population_rollout_dev(ps, pop(M, G, stride), K, *out, reset_done=True)
    sim.sync()
    for nm, x, y in zip(NAMES, host(out), want):
        np.testing.assert_array_equal(x, y, err_msg=nm)
    sim.close()
    # the heads that give a wave to a replica: refused by name, whatever the policy
    heads = ((merge_spec(R=R, cap_human=12, cap_rl=3, num_rl=2, horizon=100, seed=1), "FS_ENV_MERGE_PO"),
             (merge_spec(R=R, cap_human=12, cap_rl=3, num_rl=3, horizon=100, seed=1, env=O.ENV_MERGE_MA, ma_apply_actions=True),
              "FS_ENV_MERGE_MA"),
             (wide_spec(R), "FS_ENV_BOTTLENECK_DV"))
    for hspec, head in heads:
        hsim = make(hspec, "f32")
        hsim.reset()
        n = hsim.obs_dim
        hout = (torch.zeros((K + 1, R, n), device="cuda:0"), torch.zeros((K, R, 64), device="cuda:0"),
                torch.zeros((K, R, 64), device="cuda:0"), torch.zeros((K, R), device="cuda:0"),
                torch.zeros((K, R), dtype=torch.uint8, device="cuda:0"))
        with pytest.raises(NotImplementedError, match="fs_population: not built for .*" + head):
            hsim.population_rollout_dev(ps, pop(M, G, stride), K, *hout, reset_done=True)
        with pytest.raises(NotImplementedError, match="fs_population: not built for .*" + head):
            hsim.population_act_dev(ps, pop(M, G, stride), hout[0][0], hout[1][0], hout[2][0])
        with pytest.raises(NotImplementedError, match="fs_population: not built for .*" + head):
            hsim.population_granule(ps)
        hsim.close()
