"""The PPO update on the device at the batch sizes it is run at (flow_amd/csrc/flowsim_learn.h), past one round of
workgroups in every kernel: tests/test_device_ppo_gpu.py and tests/test_device_adam_gpu.py stop at five 64-sample tiles, one
per workgroup; the measured workload is 1024 replicas x 100 steps = 102 400 samples, 1600 tiles.

* k_ppo_grad, the composition of tiles BIT FOR BIT.  A gradient is a sum, in one fixed order, of per-tile block sums: every
  element of the packed gradient and of the two loss sums receives one float32 add per tile, workgroup g takes tiles g,
  g + G, ... in ascending order, k_ppo_reduce adds the G partials in ascending order (tests/device_ppo_ref.py compose_ref).
  The tile sums come from the kernel itself -- a call on the 64 rows of one tile alone has G = 1 and returns them -- so the
  whole-batch call must equal compose_ref of them exactly, at the smallest n that reaches each branch of the cap on G
  (one, three, four workgroups per CU) with three tiles in workgroups 0 and 1, two in all the others, and a partial last
  tile: n = 64 (2 G + 1) + 5.  A fifth of the rows are absent, a whole tile of the second round among them.
* the same batches against torch float64 autograd of ppo_update's own loss: the composition proves nothing if a tile is
  wrong in a way five tiles do not show.  The yardstick is torch FLOAT32's error on THESE inputs (its error grows with n),
  taken from the reference in the test run; the kernel may be MARGIN = 10 times that, as everywhere in the project.
* k_ppo_eval past its 1024 workgroups (n > 65 536): the bits of calls on consecutive slices of 65 536 rows; float64.
* k_gae past one 256-lane workgroup, bit for bit train_vec.gae on CPU torch.
* k_adv_stats against the ORDER the header states (tests/device_ppo_ref.py adv_stats_ref), bit for bit, where the number
  of workgroups changes, past the 256 lanes that add the partial sums, and past saturation at 512 workgroups; the
  single-row statistics through k_adv_finish.
* fs_ppo_grad_dev / fs_ppo_grad_n_dev refuse a workspace one float short, by name, and touch nothing."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "examples"))
sys.path.insert(0, HERE)

import device_adam_ref as adam_ref  # noqa: E402
import device_ppo_ref as ref  # noqa: E402
from helpers import ring_spec  # noqa: E402
from test_device_ppo_gpu import CLIP, MARGIN, Net, case, learner_of, rel_err, run_gradients, split_grad  # noqa: E402

pytestmark = pytest.mark.gpu

TILE = 64
# (D, A, layers), the workgroups G at the cap -- 256 x {1, 3, 4 per CU}: tests/test_device_ppo_cpu.py pins them without a GPU
CAPS = [((160, 32, 3), 256), ((3, 1, 2), 768), ((1, 1, 1), 1024)]


def scale_n(G):
    return TILE * (2 * G + 1) + 5


SCALE = [pytest.param(D, A, layers, G, scale_n(G), id="%d-%d-%d-n%d" % (D, A, layers, scale_n(G)))
         for (D, A, layers), G in CAPS]
assert [p.values[4] for p in SCALE] == [32837, 98373, 131141]


@pytest.fixture(scope="module")
def sim():
    from flow_amd.sim import FlowSim
    s = FlowSim(ring_spec(R=2, N=5, bunching=0), "f32")
    yield s
    s.close()


def groups_of(learner, n):
    """G of one fs_ppo_grad_dev call on n samples, as the library sizes its workspace."""
    floats = int(learner.sim.lib.fs_ppo_workspace(ctypes.byref(learner.struct), n))
    assert floats > 0 and floats % (learner.P + 2) == 0
    return floats // (learner.P + 2)


# ------------------------------------------------------------------------------- k_ppo_grad: the composition of tiles
def absent_rows(n, G, last_row):
    """A fifth of the rows, the whole tile G + 3 (second round, workgroup 3), and -- `last_row` -- the final row of the
    partial last tile."""
    absent = torch.rand(n, generator=torch.Generator().manual_seed(n)) < 0.2
    absent[TILE * (G + 3):TILE * (G + 4)] = True
    absent[n - 1] = last_row
    assert 0.15 <= float(absent.double().mean()) <= 0.25 and not bool(absent[n - 5:].all())
    return absent


def holed_actions(c, absent):
    n, A = c["act"].shape
    act = c["act"].clone()
    col = torch.randint(0, A, (n,), generator=torch.Generator().manual_seed(n + 1))
    act[absent, col[absent]] = float("nan")                                         # one NaN in the row is enough
    return act


def tile_sums(learner, dev, n, n_total, mean, std):
    """[tiles, P + 2] on the device: {grad, loss} of one call per tile, on the tile's rows alone (G = 1: the kernel's
    own block sums of the tile) with the statistics and the sample count of the whole batch.  Nothing in the loop waits
    for the device."""
    P, tiles = learner.P, (n + TILE - 1) // TILE
    out = torch.empty(tiles, P + 2, dtype=torch.float32, device=learner.device)
    for t in range(tiles):
        lo, hi = TILE * t, min(TILE * t + TILE, n)
        learner.gradients(*(x[lo:hi] for x in dev), mean, std, clip=CLIP, vf_coef=0.5, n_total=n_total)
        out[t, :P] = learner.grad
        out[t, P:] = learner.loss
    return out


@pytest.mark.parametrize("D,A,layers,G,n", SCALE)
def test_gradient_of_a_batch_is_the_stated_composition_of_its_tile_sums_bit_for_bit(sim, D, A, layers, G, n):
    c = case(D, A, layers, n)
    learner, _ = learner_of(sim, c["net"])
    tiles = (n + TILE - 1) // TILE
    assert groups_of(learner, n) == G and groups_of(learner, TILE) == 1
    assert tiles == 2 * G + 2 > G and n % TILE == 5          # workgroups 0 and 1: three tiles, the others two; a partial last tile
    absent = absent_rows(n, G, last_row=(D == 3))
    act = holed_actions(c, absent)
    n_present = int((~absent).sum())
    dev = [c["obs"].cuda(), act.cuda(), c["logp_old"].cuda(), c["adv"].cuda(), c["ret"].cuda()]
    mean, std = c["mean"].cuda(), c["std"].cuda()            # (device scalars: setting them does not wait for the host)
    stack = tile_sums(learner, dev, n, n_present, mean, std)
    grad, loss = run_gradients(learner, c, n_total=n_present, act=act)
    assert sim.last_kernel == "k_ppo_grad"
    whole, stack = torch.cat([grad, loss]), stack.cpu()
    assert bool(torch.isfinite(whole).all()) and bool(torch.isfinite(stack).all()) and float(grad.abs().max()) > 0
    assert not bool(stack[G + 3].any())                      # the absent tile adds zeros
    assert bool(stack[tiles - 1].any())                      # the partial tile does count
    want = ref.compose_ref(stack, G)
    differ = int((whole != want).sum())
    print("composition (%d, %d, %d): n=%d, tiles=%d, G=%d, %d of %d rows present; %d of %d elements differ"
          % (D, A, layers, n, tiles, G, n_present, n, differ, whole.numel()))
    assert torch.equal(whole, want), "%d of %d elements differ from the stated order" % (differ, whole.numel())
    if G > 1:
        assert not torch.equal(whole, ref.compose_ref(stack, 1))                    # (another order is other bits)
    if D != 3:
        return
    # ---- the sample count on the device: the same bits; and again after the buffers held NaN
    msn = torch.tensor([float(c["mean"]), float(c["std"]), float(n_present)], dtype=torch.float64).cuda()
    for fill in (float("nan"), 3.0):
        learner.grad.fill_(fill)
        learner.loss.fill_(fill)
        loss_n = learner.gradients_n(*dev, msn, clip=CLIP, vf_coef=0.5)
        torch.cuda.synchronize()
        assert torch.equal(learner.grad.cpu(), grad) and torch.equal(loss_n.cpu(), loss)
    learner.grad.fill_(float("nan"))
    learner.loss.fill_(float("nan"))
    if learner._work is not None:
        learner._work.fill_(float("nan"))
    again, lagain = run_gradients(learner, c, n_total=n_present, act=act)
    assert torch.equal(again, grad) and torch.equal(lagain, loss)


# --------------------------------------------------------------------------- k_ppo_grad at those sizes against float64
def scale_gradient_errors(sim, D, A, layers, n):
    """({tensor: kernel error}, {tensor: torch float32's error}, case): both against torch float64 autograd of
    ppo_update's loss on the same n inputs, by rel_err."""
    c = case(D, A, layers, n)
    learner, net = learner_of(sim, c["net"])
    run_gradients(learner, c)
    got, want = split_grad(learner, net), c["grads"]["f64"]
    return {k: rel_err(got[k], want[k]) for k in want}, {k: rel_err(c["grads"]["f32"][k], want[k]) for k in want}, c


@pytest.mark.parametrize("D,A,layers,G,n", SCALE)
def test_gradient_at_full_batch_sizes_agrees_with_float64_autograd_of_ppo_update(sim, D, A, layers, G, n):
    kern, f32, c = scale_gradient_errors(sim, D, A, layers, n)
    assert sim.last_kernel == "k_ppo_grad"
    assert 0.10 <= c["clipped"] <= 0.60, "%.0f %% of the samples are clipped" % (100 * c["clipped"])
    y = max(f32.values())                                    # torch float32 on THESE inputs: the largest over the tensors
    worst = max(kern, key=kern.get)
    print("gradient (%d, %d, %d) n=%d: kernel %.3g (%s), torch float32 on the same inputs %.3g, ratio %.2f"
          % (D, A, layers, n, kern[worst], worst, y, kern[worst] / y))
    for k, e in kern.items():
        assert e <= MARGIN * y, "%s: %.3g against 10 x %.3g" % (k, e, y)


# ------------------------------------------------------------------------------------ k_ppo_eval beyond 1024 workgroups
EVAL_N = TILE * (2 * 1024 + 1) + 5
EVAL_SLICE = 65536                                           # 1024 tiles: the most one call gives one tile per workgroup


@functools.lru_cache(maxsize=None)
def forward_case(D, A, layers, n):
    """Inputs of a forward pass, drawn on the CPU, and torch's float64 / float32 results on them (computed once)."""
    g = torch.Generator().manual_seed(31 * D + 7 * A + layers + n)
    net, net64 = Net(D, A, layers, seed=1), Net(D, A, layers, seed=1).double()
    obs = torch.randn(n, D, generator=g)
    with torch.no_grad():
        act = (net64.mu(obs.double()) + net64.log_std.exp() * torch.randn(n, A, generator=g, dtype=torch.float64)).float()
        logp64, val64 = net64.logp_value(obs.double(), act.double())
        logp32, val32 = net.logp_value(obs, act)
    return dict(net=net, obs=obs, act=act, logp64=logp64, val64=val64, logp32=logp32, val32=val32)


@pytest.mark.parametrize("D,A,layers", [(3, 1, 2), (160, 32, 3)])
def test_forward_past_1024_tiles_equals_its_slices_bit_for_bit_and_agrees_with_float64(sim, D, A, layers):
    n = EVAL_N
    assert n == 131141 and (n + TILE - 1) // TILE == 2 * 1024 + 2 and EVAL_SLICE % TILE == 0
    c = forward_case(D, A, layers, n)
    learner, _ = learner_of(sim, c["net"])
    obs, act = c["obs"].cuda(), c["act"].cuda()
    logp, val = learner.evaluate(obs, act)
    val_only = learner.evaluate(obs, None)[1]
    parts = [learner.evaluate(obs[lo:lo + EVAL_SLICE], act[lo:lo + EVAL_SLICE]) for lo in range(0, n, EVAL_SLICE)]
    torch.cuda.synchronize()
    assert sim.last_kernel == "k_ppo_eval" and [int(p[0].numel()) for p in parts] == [65536, 65536, 69]
    assert torch.equal(logp, torch.cat([p[0] for p in parts])) and torch.equal(val, torch.cat([p[1] for p in parts]))
    assert torch.equal(val, val_only)                                               # act=None: the same values
    # ---- absent rows in the second and third round change no present row's bits
    g = torch.Generator().manual_seed(9)
    absent = torch.rand(n, generator=g) < 0.2
    absent[:EVAL_SLICE] = False
    absent[EVAL_SLICE + 7 * TILE:EVAL_SLICE + 8 * TILE] = True                      # a whole tile of the second round
    absent[n - 2] = True                                                            # (the partial tile of the third)
    assert bool(absent[EVAL_SLICE:2 * EVAL_SLICE].any()) and bool(absent[2 * EVAL_SLICE:].any())
    holed = c["act"].clone()
    holed[absent, torch.randint(0, A, (n,), generator=g)[absent]] = float("nan")
    lp_a, v_a = learner.evaluate(obs, holed.cuda())
    torch.cuda.synchronize()
    keep = (~absent).cuda()
    assert torch.equal(lp_a[keep], logp[keep]) and torch.equal(v_a, val)
    # ---- float64 on the CPU; the yardstick is torch float32 on these same inputs
    e_logp, e_val = rel_err(logp, c["logp64"]), rel_err(val, c["val64"])
    y = max(rel_err(c["logp32"], c["logp64"]), rel_err(c["val32"], c["val64"]))
    print("forward (%d, %d, %d) n=%d: kernel logp %.3g val %.3g; torch float32 on the same inputs %.3g, ratio %.2f"
          % (D, A, layers, n, e_logp, e_val, y, max(e_logp, e_val) / y))
    assert e_logp <= MARGIN * y and e_val <= MARGIN * y


# --------------------------------------------------------------------------------------- k_gae past one workgroup
@pytest.mark.parametrize("K,R", [(3, 256), (3, 257), (2, 1027)])
def test_gae_past_one_workgroup_equals_torch_on_the_cpu_bit_for_bit(sim, K, R):
    import train_vec
    learner, _ = learner_of(sim, Net(3, 1, 1, seed=0))
    g = torch.Generator().manual_seed(K * 1000 + R)
    rew, val, last = torch.randn(K, R, generator=g), torch.randn(K, R, generator=g) * 3, torch.randn(R, generator=g) * 3
    done = torch.randint(0, 4, (K, R), generator=g).to(torch.uint8) * (torch.rand(K, R, generator=g) < 0.3).to(torch.uint8)
    first, lastc = torch.arange(0, R, 256), torch.arange(255, R, 256)               # the edges of every 256-lane workgroup
    done[0, first], done[K - 1, first] = 1, 2
    done[0, lastc], done[K - 1, lastc] = 0, 3
    if R % 256:
        done[K - 1, R - 1] = 1                                                      # (and the last lane of the partial one)
    assert set(done.unique().tolist()) == {0, 1, 2, 3}
    adv_ref, ret_ref = train_vec.gae(rew, val, done, last)
    adv, ret = learner.gae(rew.cuda(), val.cuda(), last.cuda(), done.cuda())
    torch.cuda.synchronize()
    assert sim.last_kernel == "k_gae"
    assert torch.equal(adv.cpu(), adv_ref) and torch.equal(ret.cpu(), ret_ref)


# ----------------------------------------------------------------------------- k_adv_stats against its stated order
@functools.lru_cache(maxsize=None)
def stats_case(n, A=3):
    """Advantages that make the ORDER of a double sum visible in its bits: float32 values of like magnitude add exactly in
    double (24-bit terms, 53-bit sums), so an order test on N(0.7, 3) draws passes in any order.  Here the magnitudes
    spread over 1e-8 .. 1e8, so most adds round, and every value comes with its negative at another place, so the sum is
    what the roundings leave.  (On the CPU, adv_stats_ref with a lane's rows taken in DESCENDING order gives other bits of
    the sum at every n >= 262144 of the test below, with and without absent rows; on N(0.7, 3) draws at none.)"""
    g = torch.Generator().manual_seed(11 * n + A)
    half = (n + 1) // 2
    x = torch.randn(half, generator=g) * 10.0 ** (16 * torch.rand(half, generator=g) - 8)
    adv = torch.cat([x, -x])[torch.randperm(2 * half, generator=g)][:n].contiguous()
    act = torch.randn(n, A, generator=g)
    absent = torch.rand(n, generator=g) < 0.25
    absent[n - 1] = False
    if n > 2:
        absent[0] = absent[n // 2] = True
    holed = act.clone()
    holed[absent, torch.randint(0, A, (n,), generator=g)[absent]] = float("nan")
    return adv, act, holed, absent


# 1: a single row; 1024 | 1025: G goes from 1 to 2; 262144 | 262145: from 256 to 257, the first second partial sum of a lane;
# 524289: the first n at which G would be 513; 525317: saturated, five rows in some lanes
@pytest.mark.parametrize("n", [1, 1024, 1025, 262144, 262145, 524289, 525317])
def test_adv_stats_equal_the_stated_order_bit_for_bit(sim, n):
    learner, _ = learner_of(sim, Net(3, 3, 1, seed=0))
    adv, act, holed, absent = stats_case(n)
    everyone = np.ones(n, dtype=np.bool_)
    for a, present in ((None, everyone), (act, everyone), (holed, (~absent).numpy())):
        adv64, stats = learner.adv_stats(adv.cuda(), None if a is None else a.cuda())
        torch.cuda.synchronize()
        assert sim.last_kernel == "k_adv_stats"
        want = ref.adv_stats_ref(adv.numpy(), present)
        got = stats.cpu().numpy()
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (n, a is None, got, want)
        assert got[2] == present.sum()
        assert torch.equal(adv64.cpu(), torch.where(torch.from_numpy(present), adv.double(), torch.zeros(n, dtype=torch.float64)))
    if n > 2:
        assert 0 < got[2] < n
        adv2 = adv.clone()
        adv2[absent] = float("nan")                                                 # whatever the absent rows hold
        _, stats = learner.adv_stats(adv2.cuda(), holed.cuda())
        torch.cuda.synchronize()
        assert stats.cpu().numpy().tobytes() == want.tobytes()


def test_adv_finish_of_a_single_row_is_numpy_s_nan(sim):
    """n = 1: the variance is 0 / 0, a NaN, and stays one through the clamp and the square root -- as in finish_ref."""
    learner, _ = learner_of(sim, Net(3, 3, 1, seed=0))
    adv, act, _, _ = stats_case(1)
    for a in (None, act):
        _, stats = learner.adv_stats(adv.cuda(), None if a is None else a.cuda())
        out = learner.adv_finish(stats)
        torch.cuda.synchronize()
        assert sim.last_kernel == "k_adv_finish"
        got = out.cpu().numpy()
        with np.errstate(all="ignore"):
            want = adam_ref.finish_ref(stats.cpu().numpy())
        assert np.isnan(want[1]) and bool(np.isnan(got[1])) == bool(np.isnan(want[1]))
        assert got[[0, 2]].tobytes() == want[[0, 2]].tobytes(), (got, want)
        assert got[0] == float(adv[0]) and got[2] == 1.0


# ------------------------------------------------------------------------------------------- the workspace, one float short
@pytest.mark.parametrize("n", [259, scale_n(768)])
def test_a_workspace_one_float_short_is_refused_by_name_and_nothing_is_touched(sim, n):
    from flow_amd import _lib as L
    c = case(3, 1, 2, n)
    learner, _ = learner_of(sim, c["net"])
    lib, h, model = sim.lib, sim._h, ctypes.byref(learner.struct)
    need = int(lib.fs_ppo_workspace(model, n))
    assert need == groups_of(learner, n) * (learner.P + 2) and groups_of(learner, n) == min((n + TILE - 1) // TILE, 768)
    t = [c[k].cuda() for k in ("obs", "act", "logp_old", "adv", "ret")]
    work = torch.zeros(need, dtype=torch.float32).cuda()     # the whole workspace is there: only the count passed is short
    ms = torch.tensor([float(c["mean"]), float(c["std"]), float(n)], dtype=torch.float64).cuda()
    sim.set_stream(torch.cuda.current_stream().cuda_stream)
    ptrs = [x.data_ptr() for x in t] + [ms.data_ptr()]

    def grad(floats):
        return lib.fs_ppo_grad_dev(h, model, n, *ptrs, CLIP, 0.5, 1.0 / n, 0, learner.grad.data_ptr(),
                                   learner.loss.data_ptr(), work.data_ptr(), floats)

    def grad_n(floats):
        return lib.fs_ppo_grad_n_dev(h, model, n, *ptrs, CLIP, 0.5, 0, learner.grad.data_ptr(), learner.loss.data_ptr(),
                                     work.data_ptr(), floats)
    for name, call in (("fs_ppo_grad_dev", grad), ("fs_ppo_grad_n_dev", grad_n)):
        learner.grad.fill_(7.5)
        learner.loss.fill_(-7.5)
        for floats in (need - 1, 0):
            with pytest.raises(ValueError, match=name + ": ") as e:
                L.check(call(floats), lib)
            assert "fs_ppo_workspace" in str(e.value)
        torch.cuda.synchronize()
        assert bool((learner.grad == 7.5).all()) and bool((learner.loss == -7.5).all()) and not bool(work.any())
        L.check(call(need), lib)                             # exactly fs_ppo_workspace(model, n) floats: accepted
        torch.cuda.synchronize()
        assert sim.last_kernel == "k_ppo_grad"
        assert not bool((learner.grad == 7.5).any()) and bool(torch.isfinite(learner.grad).all()) and bool(work.any())
        work.zero_()
