"""scripts/code_object_diff.py: the comparison of two code objects is a pure function of their texts (symbol table +
disassembly + metadata notes).  Three small hand-written pairs, no GPU and no build."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("code_object_diff", os.path.join(ROOT, "scripts", "code_object_diff.py"))
cod = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cod)

# what `llvm-objdump -t -d` and `llvm-readelf --notes` print for a unit with one kernel, cut down to the lines that matter
TEXT = """
{file}:\tfile format elf64-amdgpu

SYMBOL TABLE:
0000000000000010 l       *ABS*\t0000000000000000 _Z6kernelPf.num_vgpr
0000000000001000 g     F .text\t0000000000000020 .protected _Z6kernelPf
0000000000000800 g     O .rodata\t0000000000000040 .protected _Z6kernelPf.kd
0000000000002000 g     O .bss\t0000000000000001 .protected __hip_cuid_{cuid}

Disassembly of section .text:

0000000000001000 <_Z6kernelPf>:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0                         // 000000001000: C0060002 00000000
\tv_cvt_f32_f16_e32 {a}, v0                                    // 000000001008: 7E021700
\t{op} {c}, {a}, {b}                                       // 00000000100C: 0A040501
\tglobal_store_dword v3, {c}, s[0:1]                          // 000000001010: DC708000 00000203
\ts_endpgm                                                   // 000000001018: BF810000

Displaying notes found in: .note
amdhsa.kernels:
  - .agpr_count:     0
    .args:
      - .name:           out
        .size:           8
    .group_segment_fixed_size: {lds}
    .name:           _Z6kernelPf
    .private_segment_fixed_size: 0
    .sgpr_count:     14
    .sgpr_spill_count: 0
    .symbol:         _Z6kernelPf.kd
    .vgpr_count:     {vgprs}
    .vgpr_spill_count: 0
"""
BASE = dict(file="a.co", cuid="0123abcd", a="v1", b="v2", c="v4", op="v_mul_f32_e32", lds=0, vgprs=5)


def text(**kw):
    return TEXT.format(**{**BASE, **kw})


def test_equal_texts_are_identical():
    # the file-name header and the __hip_cuid_* object (a hash of the source) always differ between two builds
    r = cod.compare(text(), text(file="b.co", cuid="fedc9876"))
    assert r["verdict"] == "identical" and r["differing"] == 0 and r["why"] == ""
    assert r["symbols"] == 2   # the kernel and its descriptor; not the cuid object, not the *ABS* figures


def test_register_rename_is_renamed():
    # other register numbers and the two sources of a commutative multiply swapped: same mnemonics, same figures, same symbols
    r = cod.compare(text(), text(a="v2", b="v1", c="v3"))
    assert r["verdict"] == "renamed" and r["differing"] == 3 and r["why"] == ""
    # ... but not when a figure moved with it
    assert cod.compare(text(), text(a="v2", b="v1", vgprs=6))["verdict"] == "different"
    assert cod.compare(text(), text(a="v2", b="v1", lds=64))["verdict"] == "different"


def test_changed_opcode_is_different():
    r = cod.compare(text(), text(op="v_add_f32_e32"))
    assert r["verdict"] == "different" and r["differing"] == 1
    assert "_Z6kernelPf" in r["why"] and "instruction 2" in r["why"]
    # a symbol more is different too, whatever the instructions
    more = text() + "\n0000000000001100 g     F .text\t0000000000000004 .protected _Z5otherv\n"
    assert cod.compare(text(), more)["verdict"] == "different"
