"""tools/listing_diff.py on two synthetic listings of three short functions: identical, renumbered registers, one added instruction."""
import subprocess
import sys
from pathlib import Path

TOOL = Path(__file__).resolve().parent.parent / "tools" / "listing_diff.py"

# void keep<true>(float*), void regs<true, float const*, float>(float*, float const*, float), void grow<true>(float*), and a table that is no function
OLD = """\
\t.text
\t.type\t_Z4keepILb1EEvPf,@function
_Z4keepILb1EEvPf:                       ; @_Z4keepILb1EEvPf
; %bb.0:
\ts_load_dwordx2 s[0:1], s[0:1], 0x0
\tv_mov_b32_e32 v1, 0                   ; a comment
.LBB0_1:                                ; =>This Inner Loop Header: Depth=1
\tv_add_u32_e32 v1, 1, v1
\ts_cbranch_vccnz .LBB0_1
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel _Z4keepILb1EEvPf
\t.end_amdhsa_kernel
\t.text
.Lfunc_end0:
\t.size\t_Z4keepILb1EEvPf, .Lfunc_end0-_Z4keepILb1EEvPf
\t.type\t_Z4regsILb1EJPKffEEvPfDpT0_,@function
_Z4regsILb1EJPKffEEvPfDpT0_:
\ts_load_dwordx2 s[2:3], s[0:1], 0x8
\tv_mov_b32_e32 v2, s2
\ts_endpgm
.Lfunc_end1:
\t.type\t_Z4growILb1EEvPf,@function
_Z4growILb1EEvPf:
\tv_mov_b32_e32 v0, 0
\ts_endpgm
.Lfunc_end2:
\t.type\tTABLE,@object
TABLE:
\t.long\t1
\t.size\tTABLE, 4
"""

# the functions in another order (so other block numbers), a second template argument, and the two changes
NEW = """\
\t.text
\t.type\t_Z4growILb1ELb0EEvPfi,@function
_Z4growILb1ELb0EEvPfi:
\tv_mov_b32_e32 v0, 0
\ts_nop 0
\ts_endpgm
.Lfunc_end0:
\t.type\t_Z4regsILb1ELb0EEvPfi,@function
_Z4regsILb1ELb0EEvPfi:
\ts_load_dwordx2 s[4:5], s[0:1], 0x10
\tv_mov_b32_e32 v3, s4
\ts_endpgm
.Lfunc_end1:
\t.type\t_Z4keepILb1ELb0EEvPfi,@function
_Z4keepILb1ELb0EEvPfi:                  ; @_Z4keepILb1ELb0EEvPfi
; %bb.0:
\ts_load_dwordx2 s[0:1], s[0:1], 0x0
\tv_mov_b32_e32 v1, 0
.LBB2_1:
\tv_add_u32_e32 v1, 1, v1
\ts_cbranch_vccnz .LBB2_1
\ts_endpgm
.Lfunc_end2:
\t.type\tTABLE,@object
TABLE:
\t.long\t2
\t.size\tTABLE, 4
"""


def run(tmp_path, *options):
    (tmp_path / "old.s").write_text(OLD)
    (tmp_path / "new.s").write_text(NEW)
    r = subprocess.run([sys.executable, str(TOOL), str(tmp_path / "old.s"), str(tmp_path / "new.s"), *options], capture_output=True, text=True)
    return r.returncode, r.stdout.splitlines()


def test_listing_diff(tmp_path):
    rc, out = run(tmp_path, "--pad-false", "--drop-pack-types")
    assert out == ["different     grow<true, false> : +1 s_nop",
                   "identical     keep<true, false>",
                   "same opcodes  regs<true, false>",
                   "3 functions in old, 3 in new: 1 identical, 1 same opcodes, 1 different, 0 unpaired"]
    assert rc == 1
    assert run(tmp_path, "--pad-false", "--drop-pack-types", "--allow", "^grow<")[0] == 0
    assert "only in old   regs<true, float const*, float>" in run(tmp_path, "--pad-false")[1]
    rc, out = run(tmp_path)                                            # without the padding nothing pairs
    assert rc == 1 and out[-1].endswith("6 unpaired") and "only in old   keep<true>" in out
    assert run(tmp_path, "--allow", "^(keep|regs)<")[0] == 1           # grow<...> is still without a partner
    assert run(tmp_path, "--allow", "<")[0] == 0
