"""MergePOEnv's fused policy kernel for 7 .. 32 places, k_merge_wide_policy (flow_amd/csrc/flowsim_queue.h; fs_last_kernel
"k_merge_policy<PO,WIDE>"), without a GPU: code generation (hipcc -S).  The kernel exists with and without noise, keeps
nothing in scratch memory, stays within a workgroup's 64 KB of LDS and within the register file of one wave per SIMD.
tests/test_queue_codegen.py and tests/test_merge_po_policy_codegen.py hold k_merge_queue's and k_merge_policy's forms to what
they were: the wide head is a kernel of its own, under a name of its own."""
import re

import pytest

from flow_amd import build
from test_merge_po_policy_codegen import kernels


@pytest.fixture(scope="module")
def queue_asm(tmp_path_factory):
    try:
        build.find_hipcc()
    except RuntimeError:
        pytest.skip("hipcc not available")
    files = build.device_asm(str(tmp_path_factory.mktemp("asm")), names=["queue_f32"])
    with open(files["queue_f32"]) as f:
        return f.read()


def test_wide_fused_kernel_exists_in_both_noise_forms_without_scratch(queue_asm):
    table = kernels(queue_asm, "k_merge_wide_policy")
    forms = {}
    for name, res in table.items():
        m = re.match(r"_ZN2fs19k_merge_wide_policyILb([01])EEEv", name)
        assert m, name
        forms[int(m.group(1))] = res
    assert sorted(forms) == [0, 1], sorted(table)
    for noise, res in forms.items():
        print("k_merge_wide_policy<NOISE=%d>: %s" % (noise, res))
        assert res["private_seg_size"] == 0, (noise, res)
        assert 0 < res["lds_bytes"] <= 64 * 1024, (noise, res)
        assert res["num_vgpr"] + res["num_agpr"] <= 512, (noise, res)
