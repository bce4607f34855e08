"""tools/isa_same.py on small synthetic assembly listings (no compiler, no GPU): kernels pair by
symbol across files, label renumbering is not a difference, and a changed instruction, a changed
descriptor field and a kernel missing on one side are each reported with the symbol's name."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "isa_same.py")


def kernel(sym, idx, add="v_add_f64 v[0:1], v[0:1], v[2:3]", vgpr=8, tmp=0):
    """One kernel as the compiler lays it out; idx is the function's index in its file."""
    return f"""\t.text
\t.protected\t{sym} ; -- Begin function {sym}
\t.globl\t{sym}
\t.p2align\t8
\t.type\t{sym},@function
{sym}: ; @{sym}
; %bb.0:
\ts_load_dwordx2 s[2:3], s[0:1], 0x0
.Ltmp{tmp}:
\ts_cbranch_scc1 .LBB{idx}_2
; %bb.1: ; some comment {idx}
\t{add} ; a comment that differs {idx}
.LBB{idx}_2: ; =>This Inner Loop Header: Depth=1
\ts_cbranch_vccnz .LBB{idx}_2
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.p2align\t6, 0x0
\t.amdhsa_kernel {sym}
\t\t.amdhsa_group_segment_fixed_size 0
\t\t.amdhsa_private_segment_fixed_size 0
\t\t.amdhsa_next_free_vgpr {vgpr}
\t\t.amdhsa_next_free_sgpr 12
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{idx}:
\t.size\t{sym}, .Lfunc_end{idx}-{sym}
; NumVgprs: {vgpr}
"""


CUID = """\t.type\t__hip_cuid_abc123,@object
\t.globl\t__hip_cuid_abc123
__hip_cuid_abc123:
\t.byte\t0
"""


def run(tmp_path, parent, after):
    for side, files in (("parent", parent), ("after", after)):
        os.makedirs(tmp_path / side)
        for name, text in files.items():
            (tmp_path / side / name).write_text(text)
    p = subprocess.run([sys.executable, TOOL, str(tmp_path / "parent"), str(tmp_path / "after")],
                       capture_output=True, text=True)
    return p.returncode, p.stdout


def test_same_code_under_other_labels_and_in_another_file(tmp_path):
    # parent: both kernels in one file; after: _Zb alone in a new file, so its index and .Ltmp change
    parent = {"align.s": kernel("_Za", 0, tmp=0) + kernel("_Zb", 1, tmp=1) + CUID}
    after = {"dtw.s": kernel("_Za", 0, tmp=0) + CUID.replace("abc123", "ffff00"), "pair.s": kernel("_Zb", 0, tmp=0)}
    rc, out = run(tmp_path, parent, after)
    assert rc == 0, out
    assert "2 kernels at the parent, 2 after, 2 in both; 0 report lines" in out


def test_changed_instruction_is_reported_with_its_symbol(tmp_path):
    parent = {"a.s": kernel("_Za", 0) + kernel("_Zb", 1)}
    after = {"a.s": kernel("_Za", 0) + kernel("_Zb", 1, add="v_fma_f64 v[0:1], v[0:1], v[2:3], v[4:5]")}
    rc, out = run(tmp_path, parent, after)
    assert rc != 0
    lines = [ln for ln in out.splitlines() if ln.startswith("DIFFERS")]
    assert len(lines) == 1 and "_Zb" in lines[0] and "code" in lines[0]
    assert "v_add_f64 v[0:1], v[0:1], v[2:3]" in lines[0] and "v_fma_f64" in lines[0]
    assert "_Za" not in out


def test_changed_descriptor_is_reported(tmp_path):
    rc, out = run(tmp_path, {"a.s": kernel("_Za", 0, vgpr=8)}, {"a.s": kernel("_Za", 0, vgpr=9)})
    assert rc != 0
    lines = [ln for ln in out.splitlines() if ln.startswith("DIFFERS")]
    assert len(lines) == 1 and "_Za" in lines[0] and "descriptor" in lines[0]
    assert ".amdhsa_next_free_vgpr 8" in lines[0] and ".amdhsa_next_free_vgpr 9" in lines[0]


def test_kernel_on_one_side_only_is_reported(tmp_path):
    both = kernel("_Za", 0)
    rc, out = run(tmp_path, {"a.s": both + kernel("_Zgone", 1)}, {"a.s": both, "b.s": kernel("_Znew", 0)})
    assert rc != 0
    assert any(ln.startswith("ONLY IN PARENT _Zgone") for ln in out.splitlines())
    assert any(ln.startswith("ONLY AFTER _Znew") for ln in out.splitlines())
    assert "DIFFERS" not in out
