"""The float32 bits of the in-kernel policy network (flow_amd/csrc/flowsim_policy.h): `act` and `logp` of the two eager
kernels, k_policy_act and k_policy_act_vec, compared as uint32 patterns with tests/golden/policy_bits.json.  The fused
kernels (k_ring_policy, k_loop_policy, k_merge_queue<POLICY>, k_merge_policy) equal eager stepping bit for bit
(test_policy_gpu.py, test_policy_ma_gpu.py, test_policy_merge_gpu.py, test_policy_merge_po_gpu.py), so this file pins the
arithmetic of all six: a change of the network's operations or of their order shows here, whichever kernel it is made in.

Weights and observations come from numpy.random.RandomState (a frozen stream), the weights scaled as make_policy of
test_policy_gpu.py, the observations in [-1, 1].  Every case has R = 9 replicas (three waves of the row kernel, the last
a quarter full) and is called twice: the second call pins the advance of the per-replica draw counter.

The golden file is recorded on an MI355X, at the commit whose arithmetic is to be kept:
    python tests/test_policy_bits_gpu.py [COMMIT] > tests/golden/policy_bits.json
(COMMIT: the commit's hash, where the tree is not a git checkout)."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "policy_bits.json")
R = 9

# (name, handle, in_dim, num_hidden, free log std, action columns of ONE network)
CASES = [("narrow_h%d_%s" % (nh, "free" if free else "two"), "ring", 3, nh, free, 0)
         for nh in (1, 2, 3) for free in (False, True)]
CASES += [("wide6_h3_two", "fig8_ma", 6, 3, False, 0), ("wide6_h1_free", "fig8_ma", 6, 1, True, 0),
          ("wide5_h2_two", "merge_ma", 5, 2, False, 0), ("wide5_h3_free", "merge_ma", 5, 3, True, 0),
          ("wide28_h3_two", "fig8_accel", 28, 3, False, 0), ("wide28_h1_free", "fig8_accel", 28, 1, True, 0)]
CASES += [("vec%d_h%d_%s" % (A, nh, "free" if free else "two"), "merge_po", 5 * A, nh, free, A)
          for A, nh in ((1, 1), (5, 3), (6, 2)) for free in (False, True)]


def numpy_policy(rs, in_dim, num_hidden, free, A):
    """make_policy's network (weights 0.4 N(0, 1), biases 0.2 N(0, 1), the head's weights 0.3 of that) from the stream rs."""
    import torch
    from flow_amd.utils.device_policy import DevicePolicy
    cols = max(A, 1)
    dims = [in_dim] + [32] * num_hidden
    hidden = [torch.nn.Linear(dims[i], dims[i + 1]) for i in range(num_hidden)]
    head = torch.nn.Linear(32, cols if free else 2 * cols)
    for l in hidden + [head]:
        w = rs.standard_normal(tuple(l.weight.shape)) * 0.4 * (0.3 if l is head else 1.0)
        b = rs.standard_normal(tuple(l.bias.shape)) * 0.2
        with torch.no_grad():
            l.weight.copy_(torch.from_numpy(w.astype(np.float32)))
            l.bias.copy_(torch.from_numpy(b.astype(np.float32)))
        l.to("cuda:0")
    ls = None
    if free:
        ls = torch.nn.Parameter(torch.from_numpy((-0.7 + 0.05 * np.arange(cols)).astype(np.float32)).to("cuda:0"))
    return DevicePolicy(hidden, head, log_std=ls, seed=77, act_dim=cols)


def handle(kind, A):
    """The handle of a case, in the state the policy is asked about; its agents per replica."""
    from flow_amd.sim import FlowSim
    from helpers import merge_spec
    if kind == "ring":
        from test_ringrl_gpu import rl_ring_spec
        sim, n_ag = FlowSim(rl_ring_spec(R=R, N=22, seed=5), precision="f32"), 1
    elif kind == "fig8_ma":                                 # two agents: the Philox columns 0 and 1
        from test_policy_ma_gpu import fig8_ma_spec
        sim, n_ag = FlowSim(fig8_ma_spec(R, horizon=100, seed=4), precision="f32"), 2
    elif kind == "fig8_accel":                              # AccelEnv on the 14-vehicle figure eight
        from test_policy_gpu import fig8_rl_spec
        sim, n_ag = FlowSim(fig8_rl_spec(R, "accel", 0.0, horizon=100, seed=1), precision="f32"), 1
    elif kind == "merge_ma":                                # staggered: RL slots filled in some replicas only
        from test_policy_merge_gpu import ma_spec, stagger
        n_ag = 6
        sim = FlowSim(ma_spec(R=R, cap_human=24, cap_rl=n_ag, num_rl=n_ag, horizon=400, seed=2, sims_per_step=2,
                              q_rl=1500.0), precision="f32")
        stagger(sim, 2, steps=40)
        return sim, n_ag
    else:
        sim, n_ag = FlowSim(merge_spec(R=R, cap_human=12, cap_rl=A, num_rl=A, horizon=100, seed=1), precision="f32"), 1
    sim.reset()
    return sim, n_ag


def run_case(index):
    """{"act": [call][...] uint32, "logp": ...} of case `index`: two calls with the same observations."""
    import torch
    name, kind, in_dim, num_hidden, free, A = CASES[index]
    rs = np.random.RandomState(1000 + index)
    dev = torch.device("cuda", 0)
    pol = numpy_policy(rs, in_dim, num_hidden, free, A)
    sim, n_ag = handle(kind, A)
    obs = torch.from_numpy(rs.uniform(-1.0, 1.0, (R, n_ag * in_dim)).astype(np.float32)).to(dev)
    out = {"act": [], "logp": []}
    for _ in range(2):
        act = torch.zeros((R, A if A else n_ag), device=dev)
        logp = torch.zeros((R,) if A else (R, n_ag), device=dev)
        torch.cuda.synchronize()                            # (the handle launches on a stream of its own)
        sim.policy_act_dev(pol.struct, obs, act, logp)
        sim.sync()
        assert sim.last_kernel == ("k_policy_act_vec" if A else "k_policy_act")
        out["act"].append(act.cpu().numpy().view(np.uint32).reshape(-1).tolist())
        out["logp"].append(logp.cpu().numpy().view(np.uint32).reshape(-1).tolist())
    sim.close()
    return out


def bits_to_float(x):
    return np.asarray(x, dtype=np.uint32).view(np.float32)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("index", range(len(CASES)), ids=[c[0] for c in CASES])
def test_eager_policy_bits(index, golden):
    name = CASES[index][0]
    got, want = run_case(index), golden["cases"][name]
    for key in ("act", "logp"):
        for call in range(2):
            g, w = np.asarray(got[key][call], dtype=np.uint32), np.asarray(want[key][call], dtype=np.uint32)
            np.testing.assert_array_equal(g, w, err_msg="%s: %s, call %d (as float32: %s against the golden %s)"
                                          % (name, key, call, bits_to_float(g), bits_to_float(w)))
    # the second call drew again (the counter advanced); an absent agent's NaN action is the same both times
    a0, a1 = bits_to_float(got["act"][0]), bits_to_float(got["act"][1])
    here = ~np.isnan(a0)
    assert here.any() and (a0[here] != a1[here]).all()
    np.testing.assert_array_equal(np.isnan(a1), ~here)
    if CASES[index][1] == "merge_ma":                       # absent agents: no action, log-probability 0
        lp0 = bits_to_float(got["logp"][0])
        assert (~here).any() and (lp0[~here] == 0).all() and np.isfinite(lp0[here]).all()
    else:
        assert here.all()


def test_golden_covers_the_cases(golden):
    assert sorted(golden["cases"]) == sorted(c[0] for c in CASES)


def record(commit):
    import subprocess
    import torch
    if commit is None:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    doc = {"what": "act / logp of k_policy_act and k_policy_act_vec as uint32 bit patterns, two calls per case "
                   "(tests/test_policy_bits_gpu.py)",
           "commit": commit or "unknown", "rocm": torch.version.hip, "device": torch.cuda.get_device_name(0),
           "cases": {CASES[i][0]: run_case(i) for i in range(len(CASES))}}
    print(json.dumps(doc, separators=(",", ":")))


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    record(sys.argv[1] if len(sys.argv) > 1 else None)
