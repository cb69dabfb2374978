"""Code-generation guard of k_merge_queue (flow_amd/csrc/flowsim_queue.h): the MergePOEnv head is a template parameter,
so (a) no step form -- either head -- spills (no AGPRs, no scratch), and (b) the multi-agent forms are the code they
were before the head existed: registers and LDS held to the figures of tests/golden/queue_resources_before_po.json
(compiled from the commit before it) within one allocation granule."""
import json
import os
import re

import pytest

from flow_amd import build

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "queue_resources_before_po.json")
GRANULE = 8                      # registers are allocated in blocks of 8 on gfx950 (512 VGPRs + AGPRs per lane)


@pytest.fixture(scope="module")
def queue_asm(tmp_path_factory):
    try:
        build.find_hipcc()
    except RuntimeError:
        pytest.skip("hipcc not available")
    files = build.device_asm(str(tmp_path_factory.mktemp("asm")), names=["queue_f32"])
    with open(files["queue_f32"]) as f:
        return f.read()


def queue_kernels(asm):
    """{(NOISE, ACT, POLICY, PO): {num_vgpr, num_agpr, private_seg_size, lds_bytes}} of the k_merge_queue instantiations."""
    out = {}
    for name, key, val in re.findall(r"\.set (_ZN2fs13k_merge_queue\w+)\.(num_vgpr|num_agpr|private_seg_size), (\d+)", asm):
        out.setdefault(name, {})[key] = int(val)
    lds = None
    for line in asm.splitlines():                       # the metadata lists a kernel's LDS size before its name
        m = re.match(r"\s*\.group_segment_fixed_size:\s*(\d+)", line)
        if m:
            lds = int(m.group(1))
            continue
        m = re.match(r"\s*\.name:\s+(_ZN2fs13k_merge_queue\w+)\s*$", line)
        if m and m.group(1) in out:
            out[m.group(1)]["lds_bytes"] = lds
    table = {}
    for name, res in out.items():
        flags = re.match(r"_ZN2fs13k_merge_queueI((?:Lb[01]E)+)E", name).group(1)
        key = tuple(int(b) for b in re.findall(r"Lb([01])E", flags))
        table[key + (0,) * (4 - len(key))] = res
    return table


def test_step_forms_of_both_heads_use_no_agprs_and_no_scratch(queue_asm):
    table = queue_kernels(queue_asm)
    steps = {k: r for k, r in table.items() if k[2] == 0}
    # NOISE x ACT for the multi-agent head and for MergePOEnv's
    assert sorted(steps) == [(n, a, 0, po) for n in (0, 1) for a in (0, 1) for po in (0, 1)]
    bad = {k: r for k, r in steps.items() if r["num_agpr"] != 0 or r["private_seg_size"] != 0}
    assert not bad, bad
    assert not [k for k in table if k[2] == 1 and k[3] == 1]          # the fused policy is multi-agent only
    assert all(r["private_seg_size"] == 0 for r in table.values())


def test_multi_agent_forms_have_not_grown_with_the_single_agent_head(queue_asm):
    table = queue_kernels(queue_asm)
    with open(GOLDEN) as f:
        golden = json.load(f)["kernels"]
    assert len(golden) == 6
    bad = {}
    for key, ref in golden.items():
        n, a, p = (int(x) for x in re.match(r"NOISE=(\d),ACT=(\d),POLICY=(\d)", key).groups())
        got = table[(n, a, p, 0)]
        if got["num_vgpr"] + got["num_agpr"] > ref["num_vgpr"] + ref["num_agpr"] + GRANULE:
            bad[key] = ("registers", got, ref)
        elif got["lds_bytes"] > ref["lds_bytes"] or got["private_seg_size"] > ref["private_seg_size"]:
            bad[key] = ("LDS / scratch", got, ref)
    assert not bad, bad
