"""The reference's figure-eight benchmarks on the command line (examples/train.py figureeight1 / figureeight2 --fuse_policy
--device_adam): ONE policy for all RL vehicles rolled out on the fused kernel (fs_last_kernel "k_loop_policy<AccelVec>"),
the update on the device with the policy sharing the learner's buffer; a run restored from its own middle checkpoint
(--checkpoint_env_state) prints the iteration line the uninterrupted run prints."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SCRIPT = os.path.join(ROOT, "examples", "train.py")
KERNEL = "k_loop_policy<AccelVec>"

pytestmark = pytest.mark.gpu


def train(name, *extra, steps=2):
    res = subprocess.run([sys.executable, SCRIPT, name, "--fuse_policy", "--device_adam", "--replicas", "64", "--num_steps",
                          str(steps), "--rollout_size", "20"] + list(extra), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    return res.stdout


def iteration_lines(out):
    return [ln for ln in out.splitlines() if ln.startswith("iteration")]


def untimed(line):
    """An iteration line without its wall-clock figures."""
    return re.sub(r"rollout \S+ ms \(\S+ M env-steps/s", "rollout (", line)


@pytest.fixture(scope="module")
def figureeight1_run(tmp_path_factory):
    ckpt = str(tmp_path_factory.mktemp("figureeight1"))
    return ckpt, train("figureeight1", "--checkpoint_dir", ckpt, "--checkpoint_freq", "1", "--checkpoint_env_state")


def test_figureeight1_trains_on_the_fused_kernel(figureeight1_run):
    _, out = figureeight1_run
    assert "rollout: fused policy + step kernel (%s)" % KERNEL in out, out
    assert "update: on the device, Adam included" in out, out
    lines = iteration_lines(out)
    assert len(lines) == 2 and all(np.isfinite(float(ln.split()[5])) for ln in lines), out
    assert any(float(ln.split()[5]) > 0 for ln in lines), out


def test_figureeight2_trains_on_the_fused_kernel_with_statistics_and_evaluation():
    out = train("figureeight2", "--episode_stats", "--evaluation_interval", "1", "--evaluation_steps", "10")
    assert "rollout: fused policy + step kernel (%s)" % KERNEL in out, out
    lines = iteration_lines(out)
    assert len(lines) == 2 and all(np.isfinite(float(ln.split()[5])) for ln in lines), out
    assert all("evaluation/" in ln for ln in lines), out


def test_a_restored_run_prints_the_uninterrupted_runs_iteration_line(figureeight1_run):
    """figureeight1 ships SumoParams(seed=None): the handle draws its Philox key per process and the checkpoint carries it,
    so the run is compared with a restore of its OWN checkpoint after iteration 0 (iterations count from 0: the run is
    stopped after its first iteration and continued with its second)."""
    ckpt, whole = figureeight1_run
    again = train("figureeight1", "--checkpoint_env_state", "--restore", os.path.join(ckpt, "checkpoint_0"), steps=1)
    assert "continue from the checkpoint's state" in again, again
    assert KERNEL in again
    want, got = iteration_lines(whole), iteration_lines(again)
    assert len(got) == 1 and got[0].split()[1] == "1", again
    assert untimed(got[0]) == untimed(want[1]), (got[0], want[1])


def test_evaluate_replays_the_checkpoint_on_the_fused_kernel(figureeight1_run):
    """examples/evaluate.py on the run's last checkpoint: one episode of the experiment's horizon per replica with the mean
    action, on the trainer's rollout path."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import evaluate
    ckpt, _ = figureeight1_run
    res = evaluate.evaluate_checkpoint(os.path.join(ckpt, "checkpoint_1"), num_rollouts=32, fragment=100, log=lambda *a: None)
    print(res)
    assert res["kernel"] == KERNEL and res["path"] == "fused" and res["greedy"] is True and res["iteration"] == 1
    assert res["episodes"] >= 32 and res["episode_len_mean"] <= 1500.0
    for key in ("episode_reward_mean", "episode_reward_min", "episode_reward_max"):
        assert np.isfinite(res[key]), key
