"""Snapshots (include/flowsim.h fs_snapshot_info; flow_amd/envs/vec.py VecSnapshot), what can be checked without a GPU:

* fs_snapshot_info and the four entry points are declared, exported and bound together, fs_snapshot_info has the C layout, and
  the ABI version stays;
* what must never launch is refused by name from the arguments alone: a NULL buffer, wrong bytes, a NULL handle;
* ``VecSnapshot.state_dict()`` of a hand-made snapshot survives ``torch.save`` -> ``torch.load(weights_only=True)`` with the
  generator's state intact: ``np.random.default_rng`` continues the original's sequence after the round trip;
* a checkpoint written without ``env`` is the file it was and loads as before; one with ``env`` loads with
  ``weights_only=True``; the flags are off by default in both parsers."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))

NEW_NAMES = ("fs_snapshot_info", "fs_snapshot_dev", "fs_restore_dev", "fs_snapshot", "fs_restore")


@pytest.fixture(scope="module")
def lib():
    from flow_amd import _lib, build
    build.build()
    return _lib.load()


def test_header_binding_and_library_agree_on_the_new_names(lib):
    from flow_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flowsim.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fs_[a-z_0-9]+)\s*\(", text))
    for name in NEW_NAMES:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert hasattr(lib, name), name
    assert re.search(r"struct fs_snapshot_info \{[^}]*\};", text)
    assert lib.fs_abi_version() == 8 and _lib.FS_ABI_VERSION == 8               # additive: the ABI version stays
    from flow_amd.sim import FlowSim
    for name in ("snapshot_info", "snapshot_dev", "restore_dev", "snapshot", "restore"):
        assert callable(getattr(FlowSim, name)), name


def test_fs_snapshot_info_has_the_c_layout(tmp_path):
    from flow_amd import _lib
    M = _lib.fs_snapshot_info
    fields = [n for n, _ in M._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "flowsim.h"\n'
                   'int main(void){printf("%zu' + " %zu" * len(fields) + '\\n", sizeof(struct fs_snapshot_info)'
                   + "".join(", offsetof(struct fs_snapshot_info, %s)" % f for f in fields) + "); return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert out == [ctypes.sizeof(M)] + [getattr(M, f).offset for f in fields]
    assert fields[:4] == ["bytes", "host_bytes", "layout", "nonce"] and out[0] == 40


def test_what_must_never_launch_is_refused_by_name_from_the_arguments_alone(lib):
    """No handle and pointers that are never followed."""
    from flow_amd import _lib

    def err():
        return lib.fs_last_error().decode()
    calls = {
        "fs_snapshot_dev": lambda buf, n: lib.fs_snapshot_dev(None, buf, n, None),
        "fs_restore_dev": lambda buf, n: lib.fs_restore_dev(None, buf, n, 1, 1, None),
        "fs_snapshot": lambda buf, n: lib.fs_snapshot(None, buf, n),
        "fs_restore": lambda buf, n: lib.fs_restore(None, buf, n, 1),
    }
    buffers = {"fs_snapshot_dev": "dst_dev", "fs_restore_dev": "src_dev", "fs_snapshot": "host_dst", "fs_restore": "host_src"}
    for name, call in calls.items():
        assert call(None, 4096) == _lib.FS_ERR_INVALID and name in err() and buffers[name] in err() and "NULL" in err(), err()
        assert call(64, 0) == _lib.FS_ERR_INVALID and name in err() and "bytes" in err(), err()
        assert call(64, 4096) == _lib.FS_ERR_INVALID and name in err() and "NULL handle" in err(), err()
    info = _lib.fs_snapshot_info()
    assert lib.fs_snapshot_info(None, ctypes.byref(info)) == _lib.FS_ERR_INVALID and "NULL handle" in err()
    assert lib.fs_snapshot_info(None, None) == _lib.FS_ERR_INVALID and "out is NULL" in err()


def hand_made_snapshot(rng):
    from flow_amd.envs.vec import VecSnapshot, rng_state_to_plain
    g = torch.Generator().manual_seed(4)
    host = {"rng": rng_state_to_plain(rng.bit_generator.state), "warned": {"_warned_generic": 1, "_warned_pending_inflow": 0,
                                                                            "_warned_pending_length": 0}}
    ep = (torch.randn(5, generator=g, dtype=torch.float64), torch.arange(5, dtype=torch.int32), torch.zeros(8, dtype=torch.float64))
    return VecSnapshot(None, None, torch.randn(5, 3, generator=g), torch.tensor([0, 1, 0, 2, 0], dtype=torch.uint8), ep, host,
                       host_blob=torch.randint(0, 256, (64 + 160,), generator=g, dtype=torch.uint8),
                       layout=0xF123456789ABCDEF, shape="hand made")


def test_a_state_dict_survives_a_weights_only_round_trip_with_the_generator_intact(tmp_path):
    from flow_amd.envs.vec import rng_state_from_plain
    rng = np.random.default_rng(3)
    rng.integers(0, 50, 7), rng.uniform(0, 1, 3)               # (somewhere inside its sequence: has_uint32 may be set)
    rng.integers(0, 2 ** 31, 1, dtype=np.uint32)
    state = hand_made_snapshot(rng).state_dict()
    want = (rng.integers(220, 271, 16), rng.uniform(1000, 2000, 4))
    path = tmp_path / "snap.pt"
    torch.save(state, str(path))
    back = torch.load(str(path), map_location="cpu", weights_only=True)
    assert back["layout"] == 0xF123456789ABCDEF and back["shape"] == "hand made" and back["version"] == 1
    for key in ("blob", "obs", "done"):
        assert torch.equal(back[key], state[key]) and back[key].dtype == state[key].dtype, key
    for key in ("ret", "len", "stats"):
        assert torch.equal(back["ep"][key], state["ep"][key]), key
    assert back["host"] == state["host"] and back["host"]["warned"]["_warned_generic"] == 1
    assert all(isinstance(back["host"]["rng"][k], str) for k in ("bit_generator", "state", "inc"))
    again = np.random.default_rng(0)
    again.bit_generator.state = rng_state_from_plain(back["host"]["rng"])
    got = (again.integers(220, 271, 16), again.uniform(1000, 2000, 4))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_a_checkpoint_without_env_is_the_file_it_was_and_one_with_env_loads(tmp_path):
    import train_vec
    torch.manual_seed(0)
    pi = train_vec.GaussianPolicy(3, 1)
    opt = torch.optim.Adam(pi.parameters(), lr=1e-3)
    fp = train_vec.ring_flow_params(50)
    policies = dict(av=train_vec.policy_state(pi, opt, None))
    plain = train_vec.save_checkpoint(str(tmp_path / "a"), 4, fp, policies, seed=2)
    same = train_vec.save_checkpoint(str(tmp_path / "b"), 4, fp, policies, seed=2, env=None)
    assert open(os.path.join(plain, "state.pt"), "rb").read() == open(os.path.join(same, "state.pt"), "rb").read()
    ck = train_vec.load_checkpoint(plain)
    assert "env" not in ck and ck["iteration"] == 4 and ck["seed"] == 2 and sorted(ck["policies"]) == ["av"]
    rng = np.random.default_rng(9)
    env = dict(snapshot=hand_made_snapshot(rng).state_dict(), world=1, carry=torch.zeros(5, 3), handle_seed=2 ** 63 + 5)
    with_env = train_vec.save_checkpoint(str(tmp_path / "c"), 4, fp, policies, seed=2, env=env)
    ck = train_vec.load_checkpoint(with_env)                    # (weights_only=True)
    assert ck["env"]["snapshot"]["layout"] == 0xF123456789ABCDEF and torch.equal(ck["env"]["carry"], env["carry"])
    assert ck["env"]["snapshot"]["host"]["rng"] == env["snapshot"]["host"]["rng"]
    # the handle's Philox key travels with the state: the restored environments are created with it
    assert train_vec.checkpoint_handle_seed(ck) == 2 ** 63 + 5
    assert train_vec.checkpoint_handle_seed(train_vec.load_checkpoint(plain)) is None and train_vec.checkpoint_handle_seed(None) is None
    lines = []
    assert train_vec.restore_env_state(None, None, log=lines.append) is False and "no environment state" in lines[0]


def test_the_flags_are_off_by_default_in_both_parsers():
    import train
    import train_vec
    seen = {}

    def fake(flow_params, **kw):
        seen.clear()
        seen.update(kw)
        return []
    real, train_vec.train_on_device = train_vec.train_on_device, fake
    try:
        train_vec.main(["--iterations", "1"])
        assert seen["checkpoint_env_state"] is False and seen["evaluation_interval"] is None and seen["evaluation_steps"] is None
        train_vec.main(["--iterations", "1", "--checkpoint_env_state", "--evaluation_interval", "2", "--evaluation_steps", "50"])
        assert seen["checkpoint_env_state"] is True and seen["evaluation_interval"] == 2 and seen["evaluation_steps"] == 50
    finally:
        train_vec.train_on_device = real
    a = train.parse_args(["singleagent_ring"])
    assert train.env_state_settings(a) == dict(checkpoint_env_state=False, evaluation_interval=None, evaluation_steps=None)
    b = train.parse_args(["singleagent_ring", "--checkpoint_env_state", "--evaluation_interval", "5"])
    assert train.env_state_settings(b) == dict(checkpoint_env_state=True, evaluation_interval=5, evaluation_steps=None)
