"""Code-generation guard of the lean stage of the spare-slot sweep (CPU only: hipcc cross-compiles).  The near gate stands in
front of the accumulation, so the headline loop carries no v_max, and the two rows of a stage share one packed multiply for their
coefficients: 48 v_pk_fma + 4 v_add + 4 v_rsq + 4 v_cmp + 4 v_fmac + 2 v_pk_mul = 66 VALU per four rows (score_kernel.h
sweep_rows SP, stage_x).  Compiled and searched the way test_isa_spare.py does, which keeps holding its own bounds beside this."""
import shutil
import subprocess

import pytest

from test_isa_spare import CSRC, _count, _kernel, _sweep_loop

SRC = """#include "dcx_internal.h"
namespace dcx {
template __global__ void score_kernel_sp<12, KF_POLY1, 1, MODE_GRAD_ROW, 1024>(const ScoreArgs);
template __global__ void score_kernel_sp<12, KF_RQ2, 1, MODE_GRAD_ROW, 1024>(const ScoreArgs);
}
"""


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("isa_spare_lean")
    src, out = d / "k.hip", d / "k.s"
    src.write_text(SRC)
    subprocess.run(["hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I", CSRC, "-S", "--cuda-device-only",
                    str(src), "-o", str(out)], check=True, stderr=subprocess.DEVNULL)
    return out.read_text()


def test_headline_loop_has_no_clamp_and_one_packed_multiply_per_stage(isa):
    body, vgpr = _kernel(isa, r"^(_ZN3dcx15score_kernel_spILi12ELi1ELi1ELi1ELi1024EEEvNS_9ScoreArgsE):")
    sp = _sweep_loop(body)
    print("poly1:", sorted(sp.items()), "VALU", _count(sp, "v_"), "vgpr", vgpr)
    assert _count(sp, "v_max_f32") == 0, sp            # the clamp lives on the cold side alone
    assert _count(sp, "v_mul_f32") == 0, sp
    assert sp["v_pk_mul_f32"] == 2, sp                 # coef = g w, both rows of a stage
    assert sp["v_pk_fma_f32"] == 48, sp
    assert _count(sp, "v_rsq_f32") == 4, sp            # four rows per iteration
    assert _count(sp, "v_cmp_") == 4, sp               # one near gate per row
    assert _count(sp, "s_nop") <= 4, sp                # the two rows' distance chains interleave
    assert _count(sp, "scratch_") == 0, sp
    assert _count(sp, "v_readlane") + _count(sp, "v_writelane") == 0, sp
    assert vgpr <= 64, vgpr
    assert _count(sp, "v_") <= 68, (_count(sp, "v_"), sp)   # the arithmetic is 66; two register copies are tolerated


def test_rq2_loop_packs_the_kernel_function_of_two_rows(isa):
    body, vgpr = _kernel(isa, r"^(_ZN3dcx15score_kernel_spILi12ELi0ELi1ELi1ELi1024EEEvNS_9ScoreArgsE):")
    rq = _sweep_loop(body)
    print("rq2:", sorted(rq.items()), "VALU", _count(rq, "v_"), "vgpr", vgpr)
    assert rq["v_pk_mul_f32"] >= 6, rq                 # u u, val u and g w of a stage's two rows
    assert _count(rq, "v_mul_f32") == 0, rq
    assert _count(rq, "v_rcp_f32") == 4, rq            # one reciprocal per row
