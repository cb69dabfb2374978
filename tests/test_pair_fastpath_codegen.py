"""Shape of the hand-written FS_MIXED pair step in the device assembly (no GPU needed: hipcc cross-compiles gfx950 here).

The step's common form falls through; the full form of its tail (flowsim_pair.h: mixed_step_asm_slow) is a block out of
line that a wave enters through ONE conditional branch and leaves by a branch back into the step.  A wave that is alone
on its SIMD pays a fetch bubble for every taken branch, so the layout is part of the design: a compiler that inlined the
slow block, or that turned the common path into the taken side, would give the gain back without failing any parity test.

Works on the disassembly of the hot instantiation k_rollout_pair<double, 16, true, true, false> and classifies
instructions by position only: a mid-block step is what stands between the first instruction block of one step's part A
and the next step's (the unrolled loop body alternates part A, part B; blocks without instructions are skipped)."""
import re

import pytest

from test_codegen import device_asm  # noqa: F401  (the module-scoped fixture: the device assembly of every object)

HOT = r"_ZN2fs14k_rollout_pairIdLi16ELb1ELb1ELb0ELb0ELb0EE"

# instructions of a mid-block step of the parent, counted by fall_through_steps() below on the assembly of commit
# 8898992 ("Train by ES / ARS on the device: one perturbed policy per workgroup"): 97 VALU + s_waitcnt, the
# buffer store, two ds_write_b64 and the ds_read_b128
PARENT_STEP_INSTRUCTIONS = 102


def kernel_body(asm, name_re=HOT):
    name = re.search(r"^(%s\S*?):" % name_re, asm, re.M).group(1)
    body = asm[asm.index("\n" + name + ":"):]
    return body[:body.index(".set " + name)]


def instructions(text):
    out = []
    for line in text.split("\n"):
        t = line.strip()
        if not t or t.startswith(";") or t.startswith(".") or t.endswith(":"):
            continue
        out.append(t)
    return out


def asm_blocks(body):
    """(start, end) of the inline-asm blocks that hold instructions, in text order"""
    return [(m.start(), m.end()) for m in re.finditer(r";;#ASMSTART(.*?);;#ASMEND", body, re.S) if instructions(m.group(1))]


def fall_through_steps(body):
    """Text of the 14 mid-block steps of the 16-step loop body (the first 32 blocks of the kernel are its part A / part B
    blocks: the main loop precedes the remainder loop, and whatever is out of line follows both)."""
    b = asm_blocks(body)
    assert len(b) >= 34
    return [body[b[2 * k][0]:b[2 * k + 2][0]] for k in range(1, 15)]


def is_branch(t):
    return t.startswith(("s_branch", "s_cbranch", "s_setpc", "s_swappc"))


def test_common_path_falls_through_and_is_shorter_than_the_parents(device_asm):  # noqa: F811
    body = kernel_body(device_asm)
    steps = fall_through_steps(body)
    for text in steps:
        ins = instructions(text)
        branches = [t for t in ins if is_branch(t)]
        assert not [t for t in branches if not t.startswith("s_cbranch")], branches      # no unconditional branch
        assert len(branches) <= 1, branches
        assert len(ins) <= PARENT_STEP_INSTRUCTIONS - 10, (len(ins), PARENT_STEP_INSTRUCTIONS)
        assert text.count(";;#ASMSTART") == 2, "a third asm block stands in the common path"


def test_slow_block_is_out_of_line_and_rejoins_the_step(device_asm):  # noqa: F811
    body = kernel_body(device_asm)
    steps = fall_through_steps(body)
    loop_end = body.index(steps[-1]) + len(steps[-1])
    for text in steps:
        (target,) = re.findall(r"^\s*s_cbranch_\w+ (\S+)", text, re.M)
        # the block the branch enters: from its label to the next label, after the loop body's fall-through text
        at = body.index("\n" + target + ":")
        assert at > loop_end, "the slow block stands inside the common path"
        block = body[at + 1:]
        block = block[:re.search(r"^\.LBB\S+:", block[len(target) + 1:], re.M).start() + len(target) + 1]
        ins = instructions(block)
        assert block.count(";;#ASMSTART") == 1 and len(ins) >= 30, block
        # it ends by branching back to the label that follows the conditional branch in the step
        back = re.match(r"s_branch (\S+)", ins[-1])
        assert back, ins[-1]
        rejoin = re.search(r"s_cbranch_\w+ %s\s*\n(\.LBB\S+):" % re.escape(target), text)
        assert rejoin and rejoin.group(1) == back.group(1), (ins[-1], rejoin and rejoin.group(1))
