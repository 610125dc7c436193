"""tools/step_count.py on a small hand-written assembly text (CPU only, nothing
is compiled): the loops are found by their loads, the internal-node path skips
the triangle test and a leaf's further loads and keeps the bookkeeping, and
instructions are classed by mnemonic prefix."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sc():
    spec = importlib.util.spec_from_file_location("step_count", os.path.join(ROOT, "tools", "step_count.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TRI = "\n".join(f"\tv_mul_f32_e32 v{20 + i}, v1, v2" for i in range(16))

ASM = f"""
\t.text
\t.globl\twalk_kernel
walk_kernel:                            ; @walk_kernel
; %bb.0:
\ts_mov_b32 s0, 4
\ts_load_dwordx4 s[8:11], s[4:5], 0x0
.LBB0_1:                                ; =>This Loop Header: Depth=1
\tv_mov_b32_e32 v0, 0
\tglobal_load_dwordx4 v[4:7], v[40:41], off
.LBB0_2:                                ; the lockstep loop
\ts_waitcnt vmcnt(0)
\tv_sub_f32_e32 v1, v4, v2
\tv_min_f32_e32 v2, v1, v5
\tv_cmp_gt_f32_e32 vcc, v1, v2
\ts_and_b64 s[2:3], vcc, s[4:5]
\tbuffer_load_dwordx4 v[4:7], v3, s[8:11], 0 offen
\tbuffer_load_dwordx4 v[8:11], v3, s[8:11], 0 offen offset:16
\ts_and_saveexec_b64 s[6:7], s[2:3]
\ts_cbranch_execz .LBB0_4
; %bb.3:                                ; the triangle test
{TRI}
\tds_read_b32 v30, v31
.LBB0_4:
\ts_or_b64 exec, exec, s[6:7]
\ts_and_saveexec_b64 s[6:7], vcc
\ts_cbranch_execz .LBB0_6
; %bb.5:                                ; a leaf's further loads
\tbuffer_load_dwordx4 v[12:15], v3, s[8:11], 0 offen offset:32
\tbuffer_load_dwordx4 v[16:19], v3, s[8:11], 0 offen offset:48
.LBB0_6:
\ts_or_b64 exec, exec, s[6:7]
\ts_and_saveexec_b64 s[12:13], vcc
\ts_cbranch_execz .LBB0_8
; %bb.7:                                ; bookkeeping: stays on the path
\ts_bcnt1_i32_b64 s2, exec
\tv_mov_b32_e32 v1, v2
\t;;#ASMSTART
\ts_add_u32 s20, s20, 1
s_add_u32 s20, s20, 1
\t;;#ASMEND
.LBB0_8:
\ts_or_b64 exec, exec, s[12:13]
\ts_andn2_b64 exec, exec, s[14:15]
\ts_nop 0
\ts_cbranch_execnz .LBB0_2
; %bb.9:
\ts_mov_b32 s7, 0
.LBB0_10:                               ; the solo loop
\ts_cbranch_vccnz .LBB0_12
; %bb.11:                               ; a leaf's triangle
\ts_add_i32 s2, s7, 32
\ts_load_dwordx8 s[24:31], s[58:59], s2 offset:0x0
.LBB0_12:
\ts_load_dwordx8 s[36:43], s[58:59], s7 offset:0x0
\ts_waitcnt lgkmcnt(0)
\tv_sub_f32_e32 v27, s38, v39
\tv_cmp_gt_f32_e32 vcc, v34, v27
\ts_bitcmp1_b32 s39, 29
\ts_cselect_b32 s7, s7, s14
\ts_cmp_lt_u32 s7, s6
\ts_cbranch_scc1 .LBB0_10
; %bb.13:
\ts_add_i32 s0, s0, -1
\ts_cmp_lg_u32 s0, 0
\ts_cbranch_scc1 .LBB0_1
; %bb.14:
\tscratch_load_dword v1, off, off
\ts_endpgm
.Lfunc_end0:
\t.size\twalk_kernel, .Lfunc_end0-walk_kernel
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel walk_kernel
\t.end_amdhsa_kernel
\t.text
other_kernel:                           ; @other_kernel
\tv_mov_b32_e32 v0, 0
\ts_endpgm
"""


def test_classes_by_prefix(sc):
    want = {"v_pk_add_f32": "valu", "v_cmp_gt_f32_e32": "valu", "s_and_b64": "salu", "s_bcnt1_i32_b64": "salu",
            "s_setprio": "salu", "s_load_dwordx8": "smem", "s_buffer_load_dword": "smem", "s_branch": "branch",
            "s_cbranch_execz": "branch", "s_waitcnt": "wait", "s_nop": "wait", "buffer_load_dwordx4": "vmem",
            "global_load_dwordx4": "vmem", "scratch_load_dword": "vmem", "flat_load_dword": "vmem",
            "ds_read_b32": "other"}
    for m, c in want.items():
        assert sc.classify(m) == c, m


def test_kernels_are_told_apart(sc):
    ks = sc.kernels(ASM)
    assert set(ks) == {"walk_kernel", "other_kernel"}
    assert set(sc.count_text(ASM, "walk_")) == {"walk_kernel"}
    assert sc.count_text(ASM, "other_") == {"other_kernel": {}}          # no loop with the loads
    assert sc.count_text(ASM) == {}                                       # no production kernel in this text


def test_lockstep_step(sc):
    r = sc.count_text(ASM, "walk_kernel")["walk_kernel"]["lockstep"]
    # .LBB0_2, .LBB0_4, .LBB0_6, %bb.7, .LBB0_8: the triangle test (16 VALU) and the
    # leaf loads are skipped, the bookkeeping block is not
    assert r["path"] == {"valu": 4, "salu": 11, "branch": 4, "wait": 2, "vmem": 2, "smem": 0, "other": 0}
    assert r["path_blocks"][0] == ".LBB0_2" and ".LBB0_8" in r["path_blocks"]
    assert r["loop"] == {"valu": 20, "salu": 11, "branch": 4, "wait": 2, "vmem": 4, "smem": 0, "other": 1}
    assert r["scratch"] == 0                                              # the store after the loops is outside


def test_solo_step(sc):
    r = sc.count_text(ASM, "walk_kernel")["walk_kernel"]["solo"]
    # .LBB0_10 and .LBB0_12: the leaf's second load is skipped
    assert r["path"] == {"valu": 2, "salu": 3, "branch": 2, "wait": 1, "vmem": 0, "smem": 1, "other": 0}
    assert r["loop"]["smem"] == 2 and r["loop"]["salu"] == 4
    assert r["blocks"] == 3


def test_loops_are_the_innermost(sc):
    blocks = sc.kernels(ASM)["walk_kernel"]
    found = sc.loops(blocks)
    labels = {blocks[h].label: len(body) for h, body in found.items()}
    assert set(labels) == {".LBB0_1", ".LBB0_2", ".LBB0_10"}
    assert labels[".LBB0_1"] > labels[".LBB0_2"] > labels[".LBB0_10"]
    h, body = sc.find_loop(blocks, found, "lockstep")
    assert blocks[h].label == ".LBB0_2"
    h, body = sc.find_loop(blocks, found, "solo")
    assert blocks[h].label == ".LBB0_10"


def test_render_and_main(sc, tmp_path, capsys):
    p = tmp_path / "k.s"
    p.write_text(ASM)
    assert sc.main([str(p), "--kernel", "walk_kernel"]) == 0
    out = capsys.readouterr().out
    assert "lockstep" in out and "solo" in out and "(whole)" in out
    assert sc.main([str(p)]) == 1                                         # no production kernel
