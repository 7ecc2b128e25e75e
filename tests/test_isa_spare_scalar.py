"""Code-generation guard of the SCALAR half of the spare-slot sweep loop (CPU only: hipcc cross-compiles).  A wave issues at most
one instruction per turn, so its single-stream speed follows the loop's total instruction count, and the scalar unit is shared by a
CU's four SIMDs.  The four-row pipeline (score_kernel.h sweep_rows, PARTS == 0) carries one row pointer, advanced once per
iteration, loads every row at an immediate offset from it, does not clamp its look-ahead (the rows' storage has a readable tail:
kSweepLookahead <= kRowsTailRows), fetches two of the four spare rows whole (one s_load_dwordx16) and runs on one counter: hold the
generated loop to that.  The vector side is test_isa_spare.py's and test_isa_spare_lean.py's; its counts are repeated here so that
a scalar saving bought with vector instructions fails in this file."""
import shutil
import subprocess

import pytest

from test_isa_spare import CSRC, _count, _kernel, _sweep_loop

SRC = """#include "dcx_internal.h"
namespace dcx {
template __global__ void score_kernel_sp<12, KF_POLY1, 1, MODE_GRAD_ROW, 1024>(const ScoreArgs);
template __global__ void score_kernel_sp<12, KF_RQ2, 1, MODE_GRAD_ROW, 1024>(const ScoreArgs);
template __global__ void score_kernel<12, KF_POLY1, 1, MODE_GRAD_ROW, 1024, true>(const ScoreArgs);
}
"""
SP = r"^(_ZN3dcx15score_kernel_spILi12ELi%dELi1ELi1ELi1024EEEvNS_9ScoreArgsE):"     # % KF: KF_RQ2 = 0, KF_POLY1 = 1
PLAIN = r"^(_ZN3dcx12score_kernelILi12ELi1ELi1ELi1ELi1024ELb1ELb0EEEvNS_9ScoreArgsE):"
PER_ROW_ADDRESSING = ("s_min_i32", "s_ashr_i32", "s_lshl_b64")   # the look-ahead's clamp; index -> address, row by row


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("isa_spare_scalar")
    src, out = d / "k.hip", d / "k.s"
    src.write_text(SRC)
    subprocess.run(["hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I", CSRC, "-S", "--cuda-device-only",
                    str(src), "-o", str(out)], check=True, stderr=subprocess.DEVNULL)
    return out.read_text()


def _salu(c):
    """test_isa_guard.py's count for pair2: opcodes starting s_ other than loads, s_waitcnt, s_nop"""
    return sum(v for op, v in c.items() if op.startswith("s_") and not op.startswith(("s_load", "s_waitcnt", "s_nop")))


@pytest.mark.parametrize("kf,quarter", [(1, "v_rsq_f32"), (0, "v_rcp_f32")], ids=["poly1", "rq2"])
def test_spare_loop_scalar_side(isa, kf, quarter):
    body, vgpr = _kernel(isa, SP % kf)
    c = _sweep_loop(body)
    print(sorted(c.items()), "VALU", _count(c, "v_"), "loads", _count(c, "s_load_dword"), "SALU", _salu(c), "all", sum(c.values()), "vgpr", vgpr)
    # the vector side, unchanged
    assert c["v_pk_fma_f32"] == 48 and _count(c, quarter) == 4 and _count(c, "v_") <= 68, c
    # two rows arrive whole (x16), two as x8 + x4 + x1 + x2: 10 loads per four rows
    assert _count(c, "s_load_dword") <= 12, c
    assert not any(c[op] for op in PER_ROW_ADDRESSING), c
    # one pointer add pair (2), loop control (<= 3), flush test (3), the two gates (10), two spare
    assert _salu(c) <= 20, (_salu(c), c)
    assert _count(c, "v_readlane") + _count(c, "v_writelane") == 0 and _count(c, "scratch_") == 0, c
    assert vgpr <= 64, vgpr


def test_plain_expanded_loop_has_no_per_row_addressing(isa):
    body, _ = _kernel(isa, PLAIN)
    c = _sweep_loop(body)
    print(sorted(c.items()), "SALU", _salu(c))
    assert not any(c[op] for op in PER_ROW_ADDRESSING), c
