"""Policy populations and evolution strategies, the parts no GPU is needed for: the C ABI's new names and the layout of
fs_population, the numpy restatements of the direction weights on hand-computed cases, and the command line (what is
refused from the arguments alone, and the flags --help lists)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))

NEW_NAMES = ("fs_population_granule", "fs_population_act_dev", "fs_population_rollout_dev", "fs_es_perturb_dev",
             "fs_es_fitness_dev", "fs_es_weights_dev", "fs_es_workspace", "fs_es_grad_dev")


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
    assert re.search(r"typedef struct fs_population \{[^}]*\} fs_population;", text)
    assert ctypes.sizeof(_lib.fs_policy) == 48                                  # fs_policy is what it was
    from flow_amd.envs import VecFlowEnv
    from flow_amd.sim import FlowSim
    from flow_amd.utils.device_es import DeviceES
    from flow_amd.utils.device_policy import DevicePolicy
    for cls, names in ((FlowSim, ("population_granule", "population_act_dev", "population_rollout_dev")),
                       (VecFlowEnv, ("population_act", "population_rollout")), (DevicePolicy, ("population", "unpack")),
                       (DeviceES, ("generation", "state_dict", "load_state_dict"))):
        for name in names:
            assert callable(getattr(cls, name)), name
    # the workspace of k_es_grad: ceil(pairs / 32) partial vectors; nothing for shapes the kernels refuse
    assert lib.fs_es_workspace(2306, 3) == 2306 and lib.fs_es_workspace(2306, 257) == 9 * 2306
    assert lib.fs_es_workspace(2306, 2049) == 0 and lib.fs_es_workspace(0, 3) == 0


def test_fs_population_has_the_c_layout(tmp_path):
    from flow_amd import _lib
    M = _lib.fs_population
    fields = [n for n, _ in M._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "flowsim.h"\n'
                   'int main(void){printf("%zu' + " %zu" * len(fields) + '\\n", sizeof(struct fs_population)'
                   + "".join(", offsetof(struct fs_population, %s)" % f for f in fields) + "); return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert out == [ctypes.sizeof(M)] + [getattr(M, f).offset for f in fields]
    assert fields == ["struct_size", "members", "group", "reserved", "stride"] and out == [24, 0, 4, 8, 12, 16]


def test_null_arguments_are_refused_by_name(lib):
    from flow_amd import _lib

    def err():
        return lib.fs_last_error().decode()
    assert lib.fs_population_granule(None, None) < 0 and "fs_population_granule" in err()
    assert lib.fs_population_act_dev(None, None, None, None, None, None) == _lib.FS_ERR_INVALID and "fs_population_act_dev" in err()
    assert lib.fs_population_rollout_dev(None, None, None, 1, 0, None, None, None, None, None) == _lib.FS_ERR_INVALID
    assert "fs_population_rollout_dev" in err()
    assert lib.fs_es_perturb_dev(None, 7, 3, 2, 8, None, 0.02, 1, 0, None) == _lib.FS_ERR_INVALID and "fs_es_perturb_dev" in err()
    assert lib.fs_es_fitness_dev(None, 5, 4, 16, None, None, 0, None, None, None) == _lib.FS_ERR_INVALID and "fs_es_fitness_dev" in err()
    assert lib.fs_es_weights_dev(None, 0, 3, 2, 0, None, None, None) == _lib.FS_ERR_INVALID and "fs_es_weights_dev" in err()
    assert lib.fs_es_grad_dev(None, 0, 7, 3, None, 1, 0, 0.005, None, None, None, 0) == _lib.FS_ERR_INVALID and "fs_es_grad_dev" in err()


def test_centered_ranks_by_hand():
    from flow_amd.utils.device_es import centered_ranks_ref
    # N = 2 with a tie: returns (F0+, F0-, F1+, F1-) = (3, 1, 3, 2): ascending (value, index): 1 (i=1), 2 (i=3), 3 (i=0), 3 (i=2)
    # ranks by index: [2, 0, 3, 1]; c = rank / 3 - 1/2 = [1/6, -1/2, 1/2, -1/6]; u = (c+ - c-) / 2 = [1/3, 1/3]
    f32 = np.float32
    c = [f32(2 / 3 - 0.5), f32(0 / 3 - 0.5), f32(3 / 3 - 0.5), f32(1 / 3 - 0.5)]
    want = np.array([f32(c[0] - c[1]) / f32(2), f32(c[2] - c[3]) / f32(2)], f32)
    got = centered_ranks_ref(np.array([3.0, 1.0, 3.0, 2.0]))
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, want)
    np.testing.assert_allclose(got, [1 / 3, 1 / 3], rtol=0, atol=1e-7)
    # swapping the tied values' places changes nothing but their ranks: the earlier index ranks lower
    np.testing.assert_allclose(centered_ranks_ref(np.array([1.0, 3.0, 2.0, 3.0])), [-1 / 3, -1 / 3], rtol=0, atol=1e-7)
    # one pair: ranks 0 and 1 -> c = -+1/2, u = +-1
    np.testing.assert_array_equal(centered_ranks_ref(np.array([5.0, 7.0])), np.array([-1.0], f32))


def test_ars_weights_by_hand():
    from flow_amd.utils.device_es import ars_weights_ref
    # directions (F+, F-): (1, 5), (4, 2), (0, 3): keys max = 5, 4, 3.  top = 1 keeps direction 0: returns {1, 5}, mean 3,
    # population std 2; u = [(1 - 5) / (1 * 2), 0, 0]
    fit = np.array([1.0, 5.0, 4.0, 2.0, 0.0, 3.0])
    np.testing.assert_array_equal(ars_weights_ref(fit, 1), np.array([-2.0, 0.0, 0.0], np.float32))
    # top = 2 keeps directions 0 and 1: {1, 5, 4, 2}: mean 3, variance (4 + 4 + 1 + 1) / 4 = 2.5; u = diff / (2 sqrt(2.5))
    s = np.sqrt(2.5)
    np.testing.assert_array_equal(ars_weights_ref(fit, 2), np.array([-4.0 / (2 * s), 2.0 / (2 * s), 0.0], np.float32))
    # all directions (top 0 or beyond N), and a tie of the keys at the cut: the smaller p is kept
    assert (ars_weights_ref(fit, 0) != 0).all() and np.array_equal(ars_weights_ref(fit, 0), ars_weights_ref(fit, 7))
    tie = np.array([1.0, 5.0, 5.0, 2.0, 0.0, 3.0])
    assert ars_weights_ref(tie, 1)[0] != 0 and ars_weights_ref(tie, 1)[1] == 0
    # equal returns: s == 0, every weight is zero
    np.testing.assert_array_equal(ars_weights_ref(np.full(6, 2.5), 2), np.zeros(3, np.float32))


def test_command_line_refuses_by_name_and_lists_its_flags(capsys):
    import train
    with pytest.raises(NotImplementedError, match=r"--gpus 2 is not built: data-parallel ES"):
        train.main(["singleagent_ring", "--rl_trainer", "es", "--gpus", "2"])
    with pytest.raises(NotImplementedError, match=r"fs_population: not built for FS_ENV_MERGE_PO"):
        train.main(["singleagent_merge", "--rl_trainer", "es"])
    with pytest.raises(NotImplementedError, match=r"fs_population: not built for FS_ENV_MERGE_PO"):
        train.main(["singleagent_merge", "--rl_trainer", "ars"])
    with pytest.raises(NotImplementedError, match=r"no population form of fs_policy_pair"):
        train.main(["adversarial_figure_eight", "--rl_trainer", "es"])
    with pytest.raises(SystemExit):
        train.main(["singleagent_ring", "--help"])
    text = capsys.readouterr().out
    for flag in ("--rl_trainer", "--es_sigma", "--es_stepsize", "--es_l2", "--es_top", "--es_eval_members", "--gpus"):
        assert flag in text, flag
    import train_vec
    assert train_vec.ES_DEFAULTS["es"] == dict(sigma=0.02, stepsize=0.02, l2=0.005)      # es_runner.py; RLlib's l2_coeff
    assert train_vec.ES_DEFAULTS["ars"]["sigma"] == 0.2 and train_vec.ES_DEFAULTS["ars"]["stepsize"] == 0.2
