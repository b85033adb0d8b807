"""tools/kernel_asm_diff.py on three tiny hand-written assembly files: no GPU, no compiler."""
import importlib.util
import io
import os

_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "kernel_asm_diff.py")
_spec = importlib.util.spec_from_file_location("kernel_asm_diff", _PATH)
kad = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kad)


def _kernel(name, label, op="v_add_u32_e32 v1, v0, v0", vgprs=2):
    return """\t.globl\t{n}
\t.type\t{n},@function
{n}:                                  ; @{n}
; %bb.0:
\ts_load_dwordx2 s[0:1], s[0:1], 0x0
\ts_cbranch_execz .LBB{l}_2
; %bb.1:
\t{op}
.LBB{l}_2:                               ; some comment
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel {n}
\t\t.amdhsa_next_free_vgpr {v}
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{l}:
\t.size\t{n}, .Lfunc_end{l}-{n}
\t.section\t.AMDGPU.csdata,"",@progbits
; Kernel info:
; codeLenInByte = 24
; TotalNumSgprs: 8
; NumVgprs: {v}
; NumAgprs: 0
; ScratchSize: 0
; LDSByteSize: 0 bytes/workgroup (compile time only)
; Occupancy: 8
\t.text
""".format(n=name, l=label, op=op, v=vgprs)


def _meta(names):
    rows = "".join("  - .agpr_count:     0\n    .args:\n      - .offset:         0\n        .size:           8\n    .name:           %s\n"
                   "    .sgpr_spill_count: 0\n    .vgpr_spill_count: 0\n" % n for n in names)
    return "\t.amdgpu_metadata\n---\namdhsa.kernels:\n" + rows + "...\n\t.end_amdgpu_metadata\n"


def _file(kernels):
    return "".join(_kernel(*k) for k in kernels) + _meta([k[0] for k in kernels])


BASE = _file([("k_one", 0), ("k_two", 1)])


def _run(old, new):
    out = io.StringIO()
    rc = kad.report(kad.parse(old), kad.parse(new), out)
    return rc, out.getvalue(), kad.compare(kad.parse(old), kad.parse(new))


def test_label_numbers_alone_are_identical():
    rc, text, (same, differ, fresh, gone) = _run(BASE, _file([("k_one", 3), ("k_two", 7)]))
    assert (sorted(same), differ, fresh, gone) == (["k_one", "k_two"], [], [], [])
    assert rc == 0 and "2 identical, 0 differing, 0 new, 0 vanished" in text


def test_one_changed_instruction_differs():
    rc, text, (same, differ, fresh, gone) = _run(BASE, _file([("k_one", 0), ("k_two", 1, "v_sub_u32_e32 v1, v0, v0", 3)]))
    assert (same, differ, fresh, gone) == (["k_one"], ["k_two"], [], [])
    assert rc == 1 and "1 identical, 1 differing, 0 new, 0 vanished" in text
    assert "differs: k_two" in text and "instructions" in text
    row = [l.split() for l in text.splitlines() if l.strip().startswith("VGPRs")][0]
    assert row[1:3] == ["2", "3"]  # both sides' kernel info, side by side
    spills = [l.split() for l in text.splitlines() if l.strip().startswith("SGPR spills")][0]
    assert spills[2:4] == ["0", "0"]  # (read from the metadata)


def test_one_more_kernel_is_new():
    rc, text, (same, differ, fresh, gone) = _run(BASE, _file([("k_zero", 0), ("k_one", 1), ("k_two", 2)]))
    assert (sorted(same), differ, fresh, gone) == (["k_one", "k_two"], [], ["k_zero"], [])
    assert rc == 0 and "2 identical, 0 differing, 1 new, 0 vanished" in text and "new: k_zero" in text


def test_a_vanished_kernel_fails():
    rc, text, (same, differ, fresh, gone) = _run(BASE, _file([("k_one", 0)]))
    assert gone == ["k_two"] and rc == 1 and "vanished: k_two" in text
