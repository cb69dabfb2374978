"""Shape of the observation path of k_rollout_pair_n<T, 11> in the device assembly (no GPU needed: hipcc cross-compiles
gfx950 here).

The entry exists for what its steps do NOT issue (flowsim_pair.h, RING): a wave that is alone on its SIMD pays issue time
for every LDS and vector-memory instruction, so a step writes its row with ONE ds_write2_b64 (the speeds and the positions
are 11 qwords apart: an immediate only because the vehicle count is a template argument) and the 16 steps of a block leave
as 11 full-wave pieces -- 11 ds_read_b128 and 11 buffer_store_dwordx4 in the unrolled body, not 16.  A compiler that split
the write, formed the write address again in every step, or moved the drain into every step would give the gain back
without failing any parity test.  Instructions are classified by position, as in tests/test_pair_fastpath_codegen.py."""
import re

import pytest

from test_pair_fastpath_codegen import asm_blocks, instructions, is_branch, kernel_body

NEW_MIXED = r"_ZN2fs16k_rollout_pair_nIdLi11ELb0ELb0EE"
NEW_F32 = r"_ZN2fs16k_rollout_pair_nIfLi11ELb0ELb0EE"
OLD_MIXED = r"_ZN2fs14k_rollout_pairIdLi16ELb1ELb1ELb0ELb0ELb0EE"
OLD_F32 = r"_ZN2fs14k_rollout_pairIfLi16ELb1ELb1ELb0ELb0ELb0EE"
PIECES = 11                       # 16 steps x 704 bytes of a wave's rows = 11 x 1024
LDS_BYTES = 4 * 16 * 704          # four waves' 16-step images
STEP_INSTRUCTIONS = 89            # a mid-block step of k_rollout_pair<double, 16, true, true, false> before this entry


@pytest.fixture(scope="module")
def pair_asm(tmp_path_factory):
    """Device assembly of the two objects that hold the 16-lane-row pair kernels."""
    from flow_amd import build
    try:
        build.find_hipcc()
    except RuntimeError:
        pytest.skip("hipcc not found")
    files = build.device_asm(str(tmp_path_factory.mktemp("asm")), names=["seg32_f64", "seg32_f32"])
    return "\n".join(open(f).read() for f in files.values())


def steps_of(body):
    """Text of the 16 steps' part A / part B block pairs' starts: (mid-block steps 1..14, the whole 16-step body)"""
    b = asm_blocks(body)
    assert len(b) >= 34
    return [body[b[2 * k][0]:b[2 * k + 2][0]] for k in range(1, 15)], body[b[0][0]:b[31][1]], b


def count(ins, prefix):
    return sum(1 for t in ins if t.startswith(prefix))


@pytest.mark.parametrize("new,old,branches", [(NEW_MIXED, OLD_MIXED, 1), (NEW_F32, OLD_F32, 0)])
def test_a_step_is_one_lds_write_and_the_block_leaves_in_eleven_pieces(pair_asm, new, old, branches):
    mid, whole, _ = steps_of(kernel_body(pair_asm, new))
    longest_before = max(len(instructions(t)) for t in steps_of(kernel_body(pair_asm, old))[0])
    limit = min(longest_before, STEP_INSTRUCTIONS) if new == NEW_MIXED else longest_before
    for text in mid:
        ins = instructions(text)
        assert text.count(";;#ASMSTART") == 2, "a third asm block stands in the common path"
        br = [t for t in ins if is_branch(t)]
        assert len(br) == branches and all(t.startswith("s_cbranch") for t in br), br
        assert count(ins, "ds_write2_b64") == 1 and count(ins, "ds_write_b64") == 0, [t for t in ins if t.startswith("ds_")]
        assert count(ins, "ds_read_b128") <= 1 and count(ins, "buffer_store_dwordx4") <= 1
        assert count(ins, "ds_read") == count(ins, "ds_read_b128") and count(ins, "buffer_store") == count(ins, "buffer_store_dwordx4")
        assert len(ins) <= limit, (len(ins), limit)
    ins = instructions(whole)
    assert count(ins, "ds_read_b128") == PIECES and count(ins, "buffer_store_dwordx4") == PIECES
    assert count(ins, "ds_write2_b64") == 15 and count(ins, "ds_write_b64") == 0       # (the 16th follows the last block)


def test_slow_block_is_out_of_line_and_rejoins_the_step(pair_asm):
    body = kernel_body(pair_asm, NEW_MIXED)
    mid, whole, _ = steps_of(body)
    loop_end = body.index(mid[-1]) + len(mid[-1])
    for text in mid:
        (target,) = re.findall(r"^\s*s_cbranch_\w+ (\S+)", text, re.M)
        at = body.index("\n" + target + ":")
        assert at > loop_end, "the slow block stands inside the common path"
        block = body[at + 1:]
        block = block[:re.search(r"^\.LBB\S+:", block[len(target) + 1:], re.M).start() + len(target) + 1]
        ins = instructions(block)
        assert block.count(";;#ASMSTART") == 1 and len(ins) >= 30, block
        assert not [t for t in ins if t.startswith(("ds_", "buffer_"))], "the slow block touches the observation path"
        back = re.match(r"s_branch (\S+)", ins[-1])
        assert back, ins[-1]
        rejoin = re.search(r"s_cbranch_\w+ %s\s*\n(\.LBB\S+):" % re.escape(target), text)
        assert rejoin and rejoin.group(1) == back.group(1), (ins[-1], rejoin and rejoin.group(1))


def test_resources_of_every_instantiation(pair_asm):
    names = sorted(set(re.findall(r"^(_ZN2fs16k_rollout_pair_nI\w+):", pair_asm, re.M)))
    # T in {float, double} x speed mode, noise for float only
    assert len(names) == 6 and sum("pair_nId" in n for n in names) == 2, names
    for n in names:
        res = dict(re.findall(r"\.set %s\.(num_vgpr|num_agpr|private_seg_size), (\d+)" % re.escape(n), pair_asm))
        assert int(res["num_vgpr"]) <= 192 and int(res["num_agpr"]) == 0 and int(res["private_seg_size"]) == 0, (n, res)
        desc = pair_asm[pair_asm.index(".amdhsa_kernel " + n):]
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", desc).group(1))
        assert lds == LDS_BYTES, (n, lds)
