"""Code-generation guard of the pre-staged spare-slot sweep (CPU only: hipcc cross-compiles).  A block's waves all sweep the same
64 configurations, so score_body centres the features and exchanges the agreed column with the last one ONCE per block, in LDS,
and sweep_rows' PRE entry takes them as they are: the select chain that swapped the columns on the way in is gone from every wave,
the column index no longer rides in a VGPR, and the way back is index arithmetic in the cross-wave fold (score_kernel.h score_body,
fold_mine_sp).  Held here: the sweep loop itself is what it was - the counts test_isa_spare_lean.py pins, for both kernel functions -
and the whole kernel holds fewer v_cndmask_b32 than the commit before, by at least the entry swap's 2 (D - 1).
Compiled and searched the way test_isa_spare.py does."""
import shutil
import subprocess
from collections import Counter

import pytest

from test_isa_spare import CSRC, _count, _kernel, _sweep_loop

SRC = """#include "dcx_internal.h"
namespace dcx {
template __global__ void score_kernel_sp<12, KF_POLY1, 1, MODE_GRAD_ROW, 1024>(const ScoreArgs);
template __global__ void score_kernel_sp<12, KF_RQ2, 1, MODE_GRAD_ROW, 1024>(const ScoreArgs);
}
"""
D = 12
POLY1 = r"^(_ZN3dcx15score_kernel_spILi12ELi1ELi1ELi1ELi1024EEEvNS_9ScoreArgsE):"
RQ2 = r"^(_ZN3dcx15score_kernel_spILi12ELi0ELi1ELi1ELi1024EEEvNS_9ScoreArgsE):"
# static v_cndmask_b32 of the whole kernel: the commit before this form / this one, both compiled here (profiles/r21_spare_prestage.txt)
CNDMASK_PARENT = {"poly1": 244, "rq2": 216}
CNDMASK_NEW = {"poly1": 201, "rq2": 173}


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("isa_spare_prestage")
    src, out = d / "k.hip", d / "k.s"
    src.write_text(SRC)
    subprocess.run(["hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I", CSRC, "-S", "--cuda-device-only",
                    str(src), "-o", str(out)], check=True, stderr=subprocess.DEVNULL)
    return out.read_text()


def _whole(body):
    return Counter(x.split()[0] for x in (y.strip() for y in body) if x and not x.startswith((".", ";")) and not x.endswith(":"))


def test_headline_loop_is_what_it_was(isa):
    body, vgpr = _kernel(isa, POLY1)
    sp = _sweep_loop(body)
    print("poly1:", sorted(sp.items()), "VALU", _count(sp, "v_"), "vgpr", vgpr)
    assert sp["v_pk_fma_f32"] == 48, sp
    assert sp["v_pk_mul_f32"] == 2, sp
    assert _count(sp, "v_rsq_f32") == 4, sp
    assert _count(sp, "v_cmp_") == 4, sp
    assert _count(sp, "v_max_f32") == 0, sp
    assert _count(sp, "v_cndmask") == 0, sp
    assert _count(sp, "v_") <= 68, (_count(sp, "v_"), sp)
    assert _count(sp, "s_nop") <= 4, sp
    assert _count(sp, "scratch_") == 0, sp
    assert vgpr <= 64, vgpr


def test_rq2_loop_is_what_it_was(isa):
    """the RQ2 twin has no near gate and no clamp: four reciprocals, no compare, its own packed multiplies (u u, val u, g w)"""
    body, vgpr = _kernel(isa, RQ2)
    rq = _sweep_loop(body)
    print("rq2:", sorted(rq.items()), "VALU", _count(rq, "v_"), "vgpr", vgpr)
    assert rq["v_pk_fma_f32"] == 48, rq
    assert rq["v_pk_mul_f32"] == 6, rq
    assert _count(rq, "v_rcp_f32") == 4, rq
    assert _count(rq, "v_max_f32") == 0, rq
    assert _count(rq, "v_cndmask") == 0, rq
    assert _count(rq, "v_") <= 68, (_count(rq, "v_"), rq)
    assert _count(rq, "scratch_") == 0, rq
    assert vgpr <= 64, vgpr


@pytest.mark.parametrize("kname,pattern", [("poly1", POLY1), ("rq2", RQ2)])
def test_the_entry_swap_is_gone_from_the_kernel(isa, kname, pattern):
    body, _ = _kernel(isa, pattern)
    n = _count(_whole(body), "v_cndmask_b32")
    print(f"{kname}: v_cndmask_b32 {n} (recorded {CNDMASK_NEW[kname]}, the commit before {CNDMASK_PARENT[kname]})")
    assert n <= CNDMASK_PARENT[kname] - 2 * (D - 1), (kname, n)
