"""Code generation of the MultiWaveAttenuationPOEnv head (HEAD 4) of k_ring_pair (flow_amd/csrc/flowsim_ringrl.h) and
k_ring_policy (flowsim_policy.h): every instantiation the launchers can pick exists in the float32 parts, none uses scratch
memory (the other heads of k_ring_pair keep 12 bytes there for the action columns their lambdas capture; this head has one
column by construction and takes the single-column path at compile time), none uses AGPRs, the fused kernel fits the LDS of
a workgroup.  Resource figures only (the .set lines and the kernel metadata)."""
import re

import pytest

from flow_amd import build
from test_merge_po_policy_codegen import kernels

PARTS = {"seg8_f32": 8, "seg16_f32": 8, "seg32_f32": 16, "seg64_f32": 32}        # part -> ROW of its k_ring_pair


@pytest.fixture(scope="module")
def ring_asm(tmp_path_factory):
    try:
        build.find_hipcc()
    except RuntimeError:
        pytest.skip("hipcc not available")
    files = build.device_asm(str(tmp_path_factory.mktemp("asm")), names=list(PARTS) + ["seg32_f64"])
    return {name: open(path).read() for name, path in files.items()}


@pytest.mark.parametrize("part", sorted(PARTS))
def test_ring_pair_head_4_exists_in_every_form_without_scratch(ring_asm, part):
    row = PARTS[part]
    forms = {}
    for name, res in kernels(ring_asm[part], "k_ring_pair").items():
        m = re.match(r"_ZN2fs11k_ring_pairIfLi(\d+)ELi4ELb([01])ELb([01])ELb([01])EEEv", name)
        if m:
            assert int(m.group(1)) == row, name
            forms[tuple(int(g) for g in m.groups()[1:])] = res
    # <NOISE, FAST, MC = false>: Sim::launch_ring's four choices for this head (one action column: never MC)
    assert sorted(forms) == [(0, 0, 0), (0, 1, 0), (1, 0, 0), (1, 1, 0)], sorted(forms)
    for form, res in sorted(forms.items()):
        print("k_ring_pair<float, %d, 4, NOISE=%d, FAST=%d, MC=%d>: %s" % ((row,) + form + (res,)))
        assert res["private_seg_size"] == 0, (form, res)
        assert res["num_agpr"] == 0 and res["num_vgpr"] <= 256 and res["lds_bytes"] == 0, (form, res)


def test_ring_policy_head_4_exists_in_every_form_without_scratch(ring_asm):
    forms = {}
    for name, res in kernels(ring_asm["seg32_f32"], "k_ring_policy").items():
        m = re.match(r"_ZN2fs13k_ring_policyIfLi4ELb([01])ELb([01])EEEv", name)
        if m:
            forms[(int(m.group(1)), int(m.group(2)))] = res
    assert sorted(forms) == [(0, 0), (0, 1), (1, 0), (1, 1)], sorted(forms)          # <NOISE, FAST>: launch_policy_row16's
    for form, res in sorted(forms.items()):
        print("k_ring_policy<float, 4, NOISE=%d, FAST=%d>: %s" % (form + (res,)))
        assert res["private_seg_size"] == 0, (form, res)
        assert 0 < res["lds_bytes"] < 64 * 1024 and res["num_vgpr"] + res["num_agpr"] <= 512, (form, res)


def test_the_head_is_float32_only(ring_asm):
    assert not re.search(r"_ZN2fs11k_ring_pairIdLi\d+ELi4E|_ZN2fs13k_ring_policyIdLi4E", ring_asm["seg32_f64"])
    for part in PARTS:
        if part != "seg32_f32":                                  # (the fused kernel: rows of 16 lanes only)
            assert "_ZN2fs13k_ring_policyIfLi4E" not in ring_asm[part], part
