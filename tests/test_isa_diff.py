"""tools/isa_diff.py on two hand-written assembly texts: a register renaming is reported as such, a
changed opcode with its counts.  Compiles nothing."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import isa_diff  # noqa: E402

ASM = """\t.text
\t.globl\tkern
kern:                                   ; @kern
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\tv_mov_b32_e32 v2, 0
.LBB0_1:                                ; =>This Inner Loop Header: Depth=1
\tv_fma_f64 v[0:1], v[0:1], v[2:3], v[4:5]
\ts_cbranch_scc1 .LBB0_1
\ts_endpgm
\t.amdhsa_kernel kern
\t.end_amdhsa_kernel
.Lfunc_end0:
amdhsa.kernels:
  - .agpr_count:     0
    .args:
      - .offset:         0
    .group_segment_fixed_size: 64
    .name:           kern
    .private_segment_fixed_size: 0
    .sgpr_spill_count: 0
    .vgpr_count:     6
...
"""


def _report(b):
    lines, moved = isa_diff.compare(isa_diff.parse(ASM), isa_diff.parse(b))
    return "\n".join(lines), moved


def test_renamed_registers_are_the_same_code():
    text, moved = _report(ASM.replace("v[2:3]", "v[8:9]").replace("v2,", "v8,").replace("s[0:1]", "s[2:3]")
                          .replace(".LBB0_1", ".LBB7_3"))
    assert "same up to renaming" in text and moved == 0
    assert "vgpr 6 agpr 0 sgpr_spill 0 scratch 0 lds 64" in text
    # one register named like another one of the same stream is not a renaming
    text, moved = _report(ASM.replace("v[2:3]", "v[4:5]"))
    assert "same opcodes, other order" in text and moved == 1
    assert _report(ASM) == (_report(ASM)[0], 0) and "identical" in _report(ASM)[0]


def test_changed_opcode_is_reported_with_its_counts():
    text, moved = _report(ASM.replace("v_fma_f64", "v_mul_f64").replace("vgpr_count:     6", "vgpr_count:     8"))
    assert "opcodes differ (2)" in text and moved == 1
    assert "v_fma_f64" in text and "1 ->      0" in text
    assert "v_mul_f64" in text and "0 ->      1" in text
    assert "resources differ" in text
