"""Code generation of the row-per-replica action-vector head (flow_amd/csrc/flowsim_policy.h k_loop_policy_vec,
k_policy_act_row): every instantiation the launcher can pick exists in the float32 row-of-16 part, its register counts are
numbers (all of loop_policy_body and policy_row_vec_act inlined), none uses scratch memory or calls out of line, and none
has grown past tests/golden/loop_vec_kernel_resources.json.  Resource figures only (the .set lines, the kernel metadata
and the kernels' text).  tests/test_codegen.py is the guard that the other instantiations of loop_policy_body did not move."""
import json
import os
import re

import pytest

from flow_amd import build
from test_merge_po_policy_codegen import kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "loop_vec_kernel_resources.json")


@pytest.fixture(scope="module")
def seg16_asm(tmp_path_factory):
    try:
        build.find_hipcc()
    except RuntimeError:
        pytest.skip("hipcc not available")
    files = build.device_asm(str(tmp_path_factory.mktemp("asm")), names=["seg16_f32"])
    with open(files["seg16_f32"]) as f:
        return f.read()


def resources(asm, name):
    """The kernel's .set values as TEXT (an out-of-line call leaves an expression, not a number) and its instructions."""
    get = lambda key: re.search(r"\.set %s\.%s, ([^\n]*)" % (re.escape(name), key), asm).group(1).strip()
    body = re.search(r"^%s:[^\n]*\n(.*?)^\s*\.set %s\.num_vgpr" % (re.escape(name), re.escape(name)), asm, re.S | re.M).group(1)
    return {k: get(k) for k in ("num_vgpr", "num_agpr", "private_seg_size")}, body


def check(asm, name, golden):
    res, body = resources(asm, name)
    assert all(v.isdigit() for v in res.values()), (name, res)
    assert "s_swappc_b64" not in body, name
    assert int(res["private_seg_size"]) == 0, (name, res)
    total = int(res["num_vgpr"]) + int(res["num_agpr"])
    assert total <= 512, (name, res)
    assert name in golden, "not recorded in %s: %s %s" % (os.path.basename(GOLDEN), name, res)
    ref = golden[name]
    assert ref["private_seg_size"] == 0
    assert total <= ref["num_vgpr"] + ref["num_agpr"], "registers: %s, recorded %s" % (res, ref)
    return res


def test_fused_vec_kernel_exists_in_every_form_without_scratch_or_calls(seg16_asm):
    with open(GOLDEN) as f:
        golden = json.load(f)
    table = kernels(seg16_asm, "k_loop_policy_vec")
    names = set(re.findall(r"^(_ZN2fs\d+k_loop_policy_vec\w+):", seg16_asm, re.M))
    assert names and names == set(n for n in golden if "k_loop_policy_vec" in n), sorted(names)
    forms = {}
    for name in names:
        m = re.match(r"_ZN2fs17k_loop_policy_vecILb([01])ELb([01])EEEv", name)
        assert m, name
        forms[(int(m.group(1)), int(m.group(2)))] = name
    # <DELTA4, FASTC>: Sim::launch_policy_loop16's three choices, k_loop_policy's
    assert sorted(forms) == [(0, 0), (1, 0), (1, 1)], sorted(names)
    for form, name in sorted(forms.items()):
        res = check(seg16_asm, name, golden)
        print("k_loop_policy_vec<DELTA4=%d, FASTC=%d>: %s, LDS %s" % (form + (res, table.get(name, {}).get("lds_bytes"))))
        # PolicyLds (13 KB), the output rows (PolicyRowVecLds: 4 KB of weights, 1 KB of log-probabilities) and the tables
        assert 13000 + 5 * 1024 <= table[name]["lds_bytes"] < 64 * 1024, table[name]


def test_eager_row_kernel_exists_without_scratch_or_calls(seg16_asm):
    with open(GOLDEN) as f:
        golden = json.load(f)
    names = set(re.findall(r"^(_ZN2fs\d+k_policy_act_row\w+):", seg16_asm, re.M))
    assert len(names) == 1, sorted(names)
    res = check(seg16_asm, next(iter(names)), golden)
    print("k_policy_act_row: %s" % res)
