"""Per-replica inflow rates (FS_FIELD_INFLOW_PERIOD / FS_FIELD_INIT_INFLOW_PERIOD), the parts that need no GPU: the field
numbers, the rate -> period helper, the example's argument parsing and CSV layout, and the method the GPU tests
(test_inflow_rates_gpu.py) check parity with -- the frozen oracle takes one period per inflow, so row r of a handle whose
replicas have periods of their own is compared with an R = 1 oracle carrying replica r's global index (`replica_ids`, which
keys its random streams), row r of the initial state and replica r's periods."""
import os
import re
import sys

import numpy as np
import pytest

from helpers import bottleneck_spec, merge_spec
from oracle import opennet as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the periods the GPU tests hand out besides the handle's own: an exact multiple of sim_step, the period of the rate the
# reference's own reset_inflow test draws (1719.47 veh/h), and one so long that the flow emits once (begin, then past end)
PERIOD_POOL = (None, 2.0, 3600.0 / 1719.468969785563, 1.0e6)


def quiet(spec):
    spec = dict(spec)
    spec["vehicles"] = [dict(v, noise=0.0) for v in spec["vehicles"]]
    return spec


def period_table(spec, shift=0):
    """[R, num_inflows]: replica r, inflow f takes entry (r + f + shift) % 4 of PERIOD_POOL (None: the handle's own)."""
    R, fl = int(spec["num_replicas"]), spec["inflows"]
    P = np.zeros((R, len(fl)))
    for r in range(R):
        for f in range(len(fl)):
            p = PERIOD_POOL[(r + f + shift) % len(PERIOD_POOL)]
            P[r, f] = float(fl[f]["period"]) if p is None else p
    return P


def row_spec(spec, r, periods=None):
    """The R = 1 spec of replica r: its global index, its rows of the init_* arrays, its periods."""
    R = int(spec["num_replicas"])
    s = dict(spec, num_replicas=1, replica_ids=[int(spec.get("replica_offset", 0)) + r])
    s.pop("replica_offset", None)
    for key in ("init_alive", "init_pos", "init_vel", "init_route"):
        a = np.asarray(spec[key])
        assert a.shape[0] == R
        s[key] = a[r:r + 1].copy()
    per = [f["period"] for f in spec["inflows"]] if periods is None else periods
    s["inflows"] = [dict(f, period=float(p)) for f, p in zip(spec["inflows"], per)]
    return s


def row_oracles(spec, P=None, **kw):
    return [O.MergeOracle(dict(row_spec(spec, r, None if P is None else P[r]), **kw), np.float32)
            for r in range(int(spec["num_replicas"]))]


ORACLE_STATE = ("x", "v", "prev_v", "h", "route", "seq", "origin", "lead", "foll", "ctl_seq", "arrived_rl", "alive",
                "sim_steps", "seq_ctr", "ctl_ctr", "num_arrived", "num_departed", "total_arrived", "total_departed",
                "total_dropped", "time_counter")


def header_fields():
    text = open(os.path.join(ROOT, "include", "flowsim.h")).read()
    body = text[text.index("enum fs_field {"):]
    body = body[:body.index("};")]
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(FS_FIELD_[A-Z_]+)\s*=\s*(\d+)", body)}


def test_field_numbers_agree_between_the_header_and_the_binding():
    from flow_amd import _lib as L
    hdr = header_fields()
    assert hdr["FS_FIELD_INFLOW_PERIOD"] == 24 and hdr["FS_FIELD_INIT_INFLOW_PERIOD"] == 25
    for name, value in hdr.items():
        assert getattr(L, name) == value, name
    assert sorted(hdr.values()) == list(range(26))
    assert L.FS_ABI_VERSION == 8 and L.FS_MAX_INFLOWS == 8


def test_inflow_periods_reproduces_the_spec_s_periods_and_keeps_the_shares():
    from flow_amd.envs.spec import inflow_base_rates, inflow_periods
    # the values build_open_spec turns into periods: 3600.0 / float(vehsPerHour), or the period as given
    for flows in ([dict(vehsPerHour=2300 * 0.9), dict(vehsPerHour=2300 * 0.1)],
                  [dict(vehsPerHour=1719.468969785563 * .1), dict(vehsPerHour=1719.468969785563 * .9)],
                  [dict(vehsPerHour=2000), dict(vehsPerHour=100), dict(vehsPerHour=1.0 / 3.0)], [dict(vehsPerHour=2300)]):
        base = inflow_base_rates(flows)
        own = np.array([3600.0 / float(f["vehsPerHour"]) for f in flows])
        total = float(np.asarray(base, dtype=np.float64).sum())
        P = inflow_periods([total, total / 2, 1000.0, total], base)
        assert P.dtype == np.float64 and P.shape == (4, len(flows))
        np.testing.assert_array_equal(P[0], own)                       # bit for bit
        np.testing.assert_array_equal(P[3], own)
        rate = 3600.0 / P
        np.testing.assert_allclose(rate.sum(axis=1), [total, total / 2, 1000.0, total], rtol=1e-14)
        np.testing.assert_allclose(rate / rate.sum(axis=1, keepdims=True), np.broadcast_to(np.asarray(base) / total, rate.shape),
                                   rtol=1e-14)           # (a handful of float64 roundings, 1.1e-16 each)
    assert inflow_base_rates([dict(period=7.2), dict(vehsPerHour=100)]) == [3600.0 / 7.2, 100.0]
    with pytest.raises(NotImplementedError, match="scheduled"):
        inflow_base_rates([dict(probability=0.1)])
    for bad in (0.0, -5.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            inflow_periods([bad], [100.0, 900.0])


@pytest.mark.parametrize("network", ["merge", "bottleneck"])
def test_rows_of_a_batched_oracle_are_single_replica_oracles(network):
    """The parity method itself: three R = 1 oracles equal the rows of the R = 3 oracle bit for bit, and periods of
    x0.5 / x1 / x2 make the three replicas differ."""
    steps = 60
    if network == "merge":
        spec = quiet(merge_spec(R=3, cap_human=20, cap_rl=4, num_rl=2, horizon=200, seed=3))
    else:
        spec = bottleneck_spec(R=3, cap_human=40, cap_rl=8, horizon=200, seed=3)
    A = int(spec["num_rl"])
    acts = np.random.default_rng(5).uniform(-1.0, 1.0, (steps, 3, A)).astype(np.float32)

    def run(oracles, rows):
        outs = []
        for ora, sl in zip(oracles, rows):
            out = [ora.reset()]
            for k in range(steps):
                out.extend(ora.step(acts[k][sl]))
            outs.append(out)
        return outs

    whole = O.MergeOracle(spec, np.float32)
    (ref,) = run([whole], [slice(0, 3)])
    singles = row_oracles(spec)
    outs = run(singles, [slice(r, r + 1) for r in range(3)])
    for r in range(3):
        for a, b in zip(ref, outs[r]):
            np.testing.assert_array_equal(np.asarray(a)[r:r + 1], np.asarray(b))
        for name in ORACLE_STATE:
            np.testing.assert_array_equal(getattr(whole, name)[r:r + 1], getattr(singles[r], name), err_msg=name)
    own = np.array([f["period"] for f in spec["inflows"]])
    scaled = row_oracles(spec, np.stack([0.5 * own, own, 2.0 * own]))
    run(scaled, [slice(r, r + 1) for r in range(3)])
    departed = [int(o.total_departed[0]) for o in scaled]
    assert departed[0] > departed[1] > departed[2] >= 1, departed
    np.testing.assert_array_equal(scaled[1].total_departed, whole.total_departed[1:2])


def load_example():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import importlib
    return importlib.import_module("bottleneck_capacity")


def test_capacity_example_arguments_and_csv_layout(tmp_path):
    ex = load_example()
    args = ex.parse_args(["--out", "x"])
    assert args.rates == list(range(400, 3000, 100)) and len(args.rates) == 26
    assert (args.trials, args.steps, args.out) == (10, 2000, "x")
    args = ex.parse_args(["--rates", "600", "2400", "--trials", "2", "--steps", "120", "--out", str(tmp_path)])
    assert args.rates == [600.0, 2400.0] and (args.trials, args.steps) == (2, 120)
    for bad in (["--out", "x", "--trials", "0"], ["--out", "x", "--rates", "-1"], []):
        with pytest.raises(SystemExit):
            ex.parse_args(bad)
    np.testing.assert_array_equal(ex.replica_rates([600, 2400], 2), [600, 600, 2400, 2400])
    cnt = np.zeros((4, 8), dtype=np.int32)
    cnt[:, 5], cnt[:, 6], cnt[:, 7] = [5, 7, 20, 22], [9, 10, 38, 40], [0, 0, 1, 2]
    res = ex.summarise([600, 2400], 2, 120, 0.5, cnt)
    np.testing.assert_array_equal(res["outflow"], np.array([5, 7, 20, 22]) * 60.0)           # 3600 / (120 * 0.5 s)
    np.testing.assert_array_equal(res["mean_outflow"], [360.0, 1260.0])
    with pytest.raises(ValueError):
        ex.summarise([600, 2400], 2, 120, 0.5, cnt[:3])
    ex.write_csv(str(tmp_path / "out"), res)
    rets = np.loadtxt(str(tmp_path / "out" / "rets.csv"), delimiter=",", ndmin=2)
    np.testing.assert_array_equal(rets, [[600.0, 360.0], [2400.0, 1260.0]])
    io = np.loadtxt(str(tmp_path / "out" / "inflows_outflows.csv"), delimiter=",", ndmin=2)
    np.testing.assert_array_equal(io, [[600, 300], [600, 420], [2400, 1200], [2400, 1320]])
    lines = open(str(tmp_path / "out" / "replicas.csv")).read().splitlines()
    assert lines[0] == "rate,trial,outflow,entered,dropped" and len(lines) == 5
    np.testing.assert_array_equal(np.loadtxt(lines[1:], delimiter=",", ndmin=2)[:, [1, 3, 4]],
                                  [[0, 9, 0], [1, 10, 0], [0, 38, 1], [1, 40, 2]])
