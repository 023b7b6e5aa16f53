"""tools/isa_digest.py on hand-written assembly in hipcc's layout (the .amdhsa_kernel block sits between s_endpgm and
.Lfunc_end*): what is normalised away, what is reported."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import isa_digest  # noqa: E402

ASM = """\t.text
\t.p2align\t8
\t.type\tk_one,@function
k_one:                                  ; @k_one
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\tv_cmp_gt_i32_e32 vcc, s2, v0           ; a comment
\ts_cbranch_vccz .LBB{idx}_2
.LBB{idx}_1:
\t{insn}
.LBB{idx}_2:
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.p2align\t6, 0x0
\t.amdhsa_kernel k_one
\t\t.amdhsa_group_segment_fixed_size 0
\t\t.amdhsa_next_free_vgpr {vgpr}
\t\t.amdhsa_next_free_sgpr 16
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{idx}:
\t.size\tk_one, .Lfunc_end{idx}-k_one
\t.type\tk_two,@function
k_two:
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel k_two
\t\t.amdhsa_next_free_vgpr 8
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{idx2}:
"""


def table(tmp_path, name, **kw):
    args = dict(idx=3, idx2=4, insn="v_add_f32_e32 v1, v1, v2", vgpr=64)
    args.update(kw)
    path = tmp_path / f"{name}-hip-amdgcn-amd-amdhsa-gfx950.s"
    path.write_text(ASM.format(**args))
    out = {}
    isa_digest.digest_file(str(path), out)
    return out


def test_descriptor_is_captured_apart_from_the_body(tmp_path):
    t = table(tmp_path, "a")
    assert sorted(t) == ["k_one", "k_two"]
    assert t["k_one"][2] == [".amdhsa_group_segment_fixed_size 0", ".amdhsa_next_free_vgpr 64", ".amdhsa_next_free_sgpr 16"]
    assert t["k_two"][2] == [".amdhsa_next_free_vgpr 8"]
    assert t["k_one"][1] == 5 and t["k_two"][1] == 1          # instructions: no label, directive or descriptor line


def test_label_index_is_normalised(tmp_path):
    a, b = table(tmp_path, "a"), table(tmp_path, "b", idx=12, idx2=13)
    assert a == b
    report = isa_digest.compare(a, b, "REV")
    assert report == ["REV: 2 device functions, working tree: 2; 2 equal, 0 changed, 0 missing, 0 extra"]


def test_descriptor_line_is_reported(tmp_path):
    a, b = table(tmp_path, "a"), table(tmp_path, "b", idx=12, idx2=13, vgpr=56)
    assert a["k_two"] == b["k_two"] and a["k_one"][0] != b["k_one"][0]
    report = isa_digest.compare(a, b, "REV")
    assert report == ["changed: k_one: 5 -> 5 instructions",
                      "    .amdhsa_next_free_vgpr 64  ->  56",
                      "REV: 2 device functions, working tree: 2; 1 equal, 1 changed, 0 missing, 0 extra"]


def test_instruction_change_and_missing_symbol(tmp_path):
    a = table(tmp_path, "a")
    b = table(tmp_path, "b", insn="v_add_f32_e32 v1, v1, v2\n\tv_mul_f32_e32 v1, v1, v1")
    del b["k_two"]
    report = isa_digest.compare(a, b, "REV")
    assert report == ["only in REV: k_two", "changed: k_one: 5 -> 6 instructions",
                      "REV: 2 device functions, working tree: 1; 0 equal, 1 changed, 1 missing, 0 extra"]
