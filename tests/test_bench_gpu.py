"""bench.py's N > 1 code path on a one-GPU box: BENCH_FORCE_DIST=1 takes RCCL init, the per-fragment observation
all-gather, the MAX over ranks and the teardown with a world of one rank -- the 8-GPU run itself is the driver's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(extra_env, *args):
    env = dict(os.environ, **extra_env)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args), env=env, capture_output=True,
                         text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, "bench.py must print exactly one line on stdout: %r" % lines[:3]
    return json.loads(lines[0])


def test_forced_distributed_path_with_one_rank():
    out = run_bench({"BENCH_FORCE_DIST": "1", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "29611"},
                    "--gpus", "1", "--steps", "3000", "--warmup", "1500", "--full", "--no-extras")
    assert out["n_gpus"] == 1 and out["steps"] == 3000 and out["warmup"] == 1500
    assert out["metric"] == "env-steps/sec" and out["scaling"] == "weak" and out["higher_is_better"] is True
    assert out["gather_check"] == {"gathered_rows": 4096, "rank_blocks_equal_local": True}
    assert out["roofline"]["frac"] > 0.05 and out["parity"]["within_1e-4"] is True
    assert out["value"] > 1e9 and abs(out["value"] - 4096 * 3000 / (out["ms_per_step"] * 3000 * 1e-3)) < 1e-3 * out["value"]
    assert out["cpu_baseline"] is None and "rollout_1500" not in out          # --full --no-extras
    assert out["fragment_latency"]["steps"] == 1500


def test_single_gpu_line_has_no_gather_and_strong_scaling_is_the_same_workload_at_one_gpu():
    out = run_bench({}, "--gpus", "1", "--steps", "1500", "--warmup", "1500", "--no-extras", "--scaling", "strong")
    assert out["gather_check"] is None and out["scaling"] == "strong" and out["n_gpus"] == 1
    assert out["config"]["replicas_total"] == 4096 and out["config"]["replicas_per_gpu"] == 4096


def test_plain_run_is_the_headline_alone_and_dumps_what_its_last_step_returned(tmp_path):
    """Without --full the line has no roofline / parity legs; --dump-outputs holds the observation, reward and done of
    the last timed step, bit for bit what the C twin of the FS_MIXED rollout computes for that step."""
    from bench import c2_spec
    from oracle import cbuild
    R = 256
    out = run_bench({}, "--gpus", "1", "--steps", "1500", "--warmup", "1500", "--replicas", str(R),
                    "--dump-outputs", str(tmp_path))
    assert out["steps"] == 1500 and out["dtype"] == "mixed" and out["ms_per_step"] > 0
    assert "roofline" not in out and "parity" not in out and "rollout_1500" not in out and out["cpu_baseline"] is None
    dumped = {n: np.load(str(tmp_path / (n + ".npy"))) for n in ("obs", "reward", "done")}
    assert all(a.dtype == np.float32 for a in dumped.values())
    # warm-up and timed region are one 1500-step episode each: the last timed step is step 1500 from the initial state
    o, r, d = cbuild.CRingIDMMixed(c2_spec(R, seed=1000)).rollout(1500)
    np.testing.assert_array_equal(dumped["obs"], o[0])
    np.testing.assert_array_equal(dumped["reward"], r[0])
    np.testing.assert_array_equal(dumped["done"], d[0].astype(np.float32))
    assert dumped["done"].all()
