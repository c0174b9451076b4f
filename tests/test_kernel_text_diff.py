"""tools/kernel_text_diff.py on short synthetic listings: two kernels that differ only in the function number of their local
labels and in comments are the same; one changed instruction, one changed resource line and one missing kernel are each found."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "kernel_text_diff.py")


def _kernel(name, fn, op="v_add_f32_e32 v0, v0, v1", vgpr=8, note=""):
    return f"""\t.text
\t.globl\t{name}
\t.type\t{name},@function
{name}:                                 ; @{name} {note}
; %bb.0:
\ts_load_dword s3, s[0:1], 0x64
\ts_cbranch_execz .LBB{fn}_2

.LBB{fn}_1:                                ; =>This Inner Loop Header: Depth=1 {note}
\t{op}
\ts_cbranch_scc1 .LBB{fn}_1
.LBB{fn}_2:
\ts_endpgm
.Lfunc_end{fn}:
\t.size\t{name}, .Lfunc_end{fn}-{name}
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel {name}
\t\t.amdhsa_group_segment_fixed_size 0
\t\t.amdhsa_next_free_vgpr {vgpr}
\t\t.amdhsa_next_free_sgpr 16
\t.end_amdhsa_kernel
"""


def _run(tmp_path, a, b):
    pa, pb = tmp_path / "a.s", tmp_path / "b.s"
    pa.write_text(a)
    pb.write_text(b)
    r = subprocess.run([sys.executable, TOOL, str(pa), str(pb)], capture_output=True, text=True)
    return r.returncode, r.stdout


def test_equal_apart_from_label_numbers_and_comments(tmp_path):
    a = _kernel("k_one", 0) + _kernel("k_two", 1)
    b = _kernel("k_two", 0, note="moved") + _kernel("k_one", 7, note="moved")
    rc, out = _run(tmp_path, a, b)
    assert rc == 0, out
    assert "same instructions and resources: 2" in out and "different: 0" in out and "RESULT: identical" in out


def test_one_instruction_changed(tmp_path):
    a = _kernel("k_one", 0) + _kernel("k_two", 1)
    b = _kernel("k_one", 0) + _kernel("k_two", 1, op="v_sub_f32_e32 v0, v0, v1")
    rc, out = _run(tmp_path, a, b)
    assert rc == 1, out
    assert "different: 1" in out and "  k_two: instructions" in out and "same instructions and resources: 1" in out


def test_one_resource_line_changed(tmp_path):
    rc, out = _run(tmp_path, _kernel("k_one", 0), _kernel("k_one", 0, vgpr=9))
    assert rc == 1, out
    assert "  k_one: resources" in out and ".amdhsa_next_free_vgpr 8 | B .amdhsa_next_free_vgpr 9" in out
    # a resource line that only one side has is shown too
    extra = _kernel("k_one", 0).replace("\t.end_amdhsa_kernel", "\t\t.amdhsa_uses_dynamic_stack 0\n\t.end_amdhsa_kernel")
    rc, out = _run(tmp_path, _kernel("k_one", 0), extra)
    assert rc == 1, out
    assert "  k_one: resources" in out and "A (no line) | B .amdhsa_uses_dynamic_stack 0" in out


def test_one_kernel_missing_or_defined_twice(tmp_path):
    both = _kernel("k_one", 0) + _kernel("k_two", 1)
    rc, out = _run(tmp_path, both, _kernel("k_one", 0))
    assert rc == 1, out
    assert "only in A: 1\n  k_two" in out and "only in B: 0" in out
    rc, out = _run(tmp_path, _kernel("k_one", 0), both)
    assert rc == 1 and "only in B: 1\n  k_two" in out
    rc, out = _run(tmp_path, both + _kernel("k_two", 2), both)
    assert rc == 1 and "defined more than once: 1\n  k_two" in out
