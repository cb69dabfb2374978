"""Code generation of the two-policy kernels (flow_amd/csrc/flowsim_policy.h k_loop_policy_pair, k_policy_pair_act): every
instantiation the launcher can pick exists in the float32 row-of-16 part, none uses scratch memory, each fits the LDS of
a workgroup and the register file.  Resource figures only (the .set lines and the kernel metadata)."""
import re

import pytest

from flow_amd import build
from test_merge_po_policy_codegen import kernels


@pytest.fixture(scope="module")
def seg16_asm(tmp_path_factory):
    try:
        build.find_hipcc()
    except RuntimeError:
        pytest.skip("hipcc not available")
    files = build.device_asm(str(tmp_path_factory.mktemp("asm")), names=["seg16_f32"])
    with open(files["seg16_f32"]) as f:
        return f.read()


def check(res):
    assert res["private_seg_size"] == 0, res
    assert 0 < res["lds_bytes"] < 64 * 1024, res
    assert res["num_vgpr"] + res["num_agpr"] <= 512, res


def test_fused_pair_kernel_exists_in_every_form_without_scratch(seg16_asm):
    table = kernels(seg16_asm, "k_loop_policy_pair")
    forms = {}
    for name, res in table.items():
        m = re.match(r"_ZN2fs18k_loop_policy_pairILb([01])ELb([01])EEEv", name)
        assert m, name
        forms[(int(m.group(1)), int(m.group(2)))] = res
    # <DELTA4, FASTC>: Sim::launch_policy_pair16's three choices, k_loop_policy's
    assert sorted(forms) == [(0, 0), (1, 0), (1, 1)], sorted(table)
    for form, res in sorted(forms.items()):
        print("k_loop_policy_pair<DELTA4=%d, FASTC=%d>: %s" % (form + (res,)))
        check(res)
        assert res["lds_bytes"] >= 2 * 13000, res          # two PolicyLds: the adversary's copy is there


def test_eager_pair_kernel_exists_without_scratch(seg16_asm):
    table = kernels(seg16_asm, "k_policy_pair_act")
    assert len(table) == 1, sorted(table)
    res = next(iter(table.values()))
    print("k_policy_pair_act: %s" % res)
    check(res)
