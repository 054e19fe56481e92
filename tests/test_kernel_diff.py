"""CPU: scripts/kernel_diff.py, the comparison that holds a refactor to "device code identical to the parent, kernel by
kernel" -- on three miniature listings: the same kernel with other label names, one instruction changed, a kernel missing."""
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_diff  # noqa: E402


def _listing(kernels):
    """A listing in the shape hipcc -S writes: per kernel an entry label, the body, an end label and its .amdhsa_kernel block."""
    out = ["\t.text", "\t.amdgcn_target \"amdgcn-amd-amdhsa--gfx950\""]
    for i, (name, body, vgpr) in enumerate(kernels):
        out += [f"\t.globl\t{name}", f"\t.type\t{name},@function", f"{name}:                        ; @{name}", "; %bb.0:"]
        out += body
        out += [f".Lfunc_end{i}:", f"\t.size\t{name}, .Lfunc_end{i}-{name}", "\t.section\t.rodata,\"a\",@progbits",
                f"\t.amdhsa_kernel {name}", f"\t\t.amdhsa_next_free_vgpr {vgpr}", "\t\t.amdhsa_next_free_sgpr 8",
                "\t\t.amdhsa_group_segment_fixed_size 0", "\t\t.amdhsa_private_segment_fixed_size 0", "\t.end_amdhsa_kernel", "\t.text"]
    return "\n".join(out) + "\n"


def _body(label, shift):
    return [f"\t.loc\t1 {shift + 3} 9                      ; a debug directive",
            "\tv_and_b32_e32 v1, 63, v0",
            f"{label}:                                ; =>This Inner Loop Header",
            f"\tv_lshlrev_b32_e32 v2, {shift}, v1         ; a comment",
            "\tv_add_u32_e32 v1, v2, v1",
            "\tv_cmp_gt_u32_e32 vcc, 64, v1",
            f"\ts_cbranch_vccnz {label}",
            "\ts_endpgm"]


A = "_Z6kernelA", "_Z6kernelB"
PARENT = _listing([(A[0], _body(".LBB0_1", 2), 3), (A[1], _body(".LBB1_1", 4), 3)])


def _run(parent, child):
    out = io.StringIO()
    n, bad = kernel_diff.compare([parent], [child], out)
    return n, bad, out.getvalue()


def test_label_names_comments_and_debug_lines_do_not_count():
    # the child holds the same two kernels in the other order: every label number, comment and .loc line differs
    child = _listing([(A[1], _body(".LBB0_7", 4), 3), (A[0], _body(".Ltmp5", 2), 3)])
    child = child.replace("a comment", "another comment").replace(".loc\t1", ".loc\t2")
    n, bad, text = _run(PARENT, child)
    assert (n, bad) == (2, 0), text
    assert text.count(": identical") == 2


def test_string_constants_count_by_what_they_hold_not_by_their_number():
    # a kernel that moved to a smaller unit: its string constant has another number there; another string is a difference
    def with_string(sym, text):
        body = _body(".LBB0_1", 2)[:-1] + [f"\ts_add_u32 s0, s0, {sym}@rel32@lo+4", "\ts_endpgm"]
        rodata = f"\t.type\t{sym},@object\n{sym}:\n\t.asciz\t\"{text}\"\n\t.size\t{sym}, {len(text) + 1}\n"
        return _listing([(A[0], body, 3)]) + ".str:\n\t.asciz\t\"other\"\n" * (sym != ".str") + rodata
    n, bad, text = _run(with_string(".str.9", "\\tNM:i:"), with_string(".str", "\\tNM:i:"))
    assert (n, bad) == (1, 0), text
    n, bad, text = _run(with_string(".str.9", "\\tNM:i:"), with_string(".str", "\\tMD:Z:"))
    assert (n, bad) == (1, 1) and "-1 / +1 lines" in text, text


def test_one_changed_instruction_is_reported_for_its_kernel_alone():
    child = _listing([(A[0], _body(".LBB0_1", 2), 3), (A[1], _body(".LBB1_1", 5), 4)])
    n, bad, text = _run(PARENT, child)
    assert (n, bad) == (2, 1), text
    line = [l for l in text.split("\n") if "kernelB" in l][0]
    assert "instructions 6->6" in line and "VGPR 3->4" in line and "SGPR 8," in line and "-1 / +1 lines" in line, line
    assert [l for l in text.split("\n") if "kernelA" in l][0].endswith(": identical")


def test_a_missing_kernel_fails_on_either_side(tmp_path):
    one = _listing([(A[0], _body(".LBB0_1", 2), 3)])
    for parent, child, where in ((PARENT, one, "child"), (one, PARENT, "parent")):
        n, bad, text = _run(parent, child)
        assert (n, bad) == (2, 1), text
        assert f"kernelB: missing in the {where}" in text or f"{A[1]}: missing in the {where}" in text, text
    # the command line: exit status 1 with a kernel missing, 0 for the same listing under two names
    p, c, c2 = tmp_path / "p.s", tmp_path / "c.s", tmp_path / "c2.s"
    p.write_text(PARENT)
    c.write_text(one)
    c2.write_text(PARENT)
    assert kernel_diff.main(["kernel_diff.py", str(p), str(c)]) == 1
    assert kernel_diff.main(["kernel_diff.py", str(p), str(c2)]) == 0
