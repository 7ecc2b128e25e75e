"""Code-generation guard of the spare-slot form of the expanded sweep (CPU only: hipcc cross-compiles).  The form exists to
take two v_add per pair out of the headline loop - the seed |x|^2 + |s|^2 and the run's sum of coefficients ride in the packed
fmas' slots of a feature column on which all supports agree (score_kernel.h spare_applies) - so hold the generated loop to
exactly that, beside the plain expanded loop compiled in the same translation unit."""
import os
import re
import shutil
import subprocess
from collections import Counter

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "diffco_amd", "csrc")

SRC = """#include "dcx_internal.h"
namespace dcx {
template __global__ void score_kernel_sp<12, KF_POLY1, 1, MODE_GRAD_ROW, 1024>(const ScoreArgs);
template __global__ void score_kernel<12, KF_POLY1, 1, MODE_GRAD_ROW, 1024, true>(const ScoreArgs);
}
"""


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("isa_spare")
    src, out = d / "k.hip", d / "k.s"
    src.write_text(SRC)
    subprocess.run(["hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I", CSRC, "-S", "--cuda-device-only",
                    str(src), "-o", str(out)], check=True, stderr=subprocess.DEVNULL)
    return out.read_text()


def _kernel(txt, pattern):
    m = re.search(pattern, txt, re.M)
    assert m, pattern
    body = txt[m.end():txt.index(".Lfunc_end", m.end())].split("\n")
    meta = txt[txt.index(".name:           " + m.group(1)):]
    return body, int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1))


def _sweep_loop(body):
    """the smallest backward-branch range that loads support rows through the scalar cache and holds at least two quarter-rate
    ops (test_isa_guard.py's rule)"""
    labels = {m.group(1): n for n, l in enumerate(body) if (m := re.match(r"^(\.LBB\d+_\d+):", l))}
    best = None
    for n, l in enumerate(body):
        m = re.search(r"s_c?branch\w* (\.LBB\d+_\d+)", l)
        if m and m.group(1) in labels and labels[m.group(1)] < n:
            seg = body[labels[m.group(1)]:n + 1]
            quarter = sum(("v_rsq_f32" in x) or ("v_rcp_f32" in x) for x in seg)
            if quarter >= 2 and sum("s_load_dword" in x for x in seg) >= 2 and (best is None or len(seg) < len(best)):
                best = seg
    assert best is not None, "sweep loop not found"
    return Counter(x.split()[0] for x in (y.strip() for y in best) if x and not x.startswith((".", ";")))


def _count(c, prefix):
    return sum(v for op, v in c.items() if op.startswith(prefix))


def test_spare_loop_drops_the_two_adds_per_pair(isa):
    sp_body, sp_vgpr = _kernel(isa, r"^(_ZN3dcx15score_kernel_spILi12ELi1ELi1ELi1ELi1024EEEvNS_9ScoreArgsE):")
    pl_body, _ = _kernel(isa, r"^(_ZN3dcx12score_kernelILi12ELi1ELi1ELi1ELi1024ELb1ELb0EEEvNS_9ScoreArgsE):")
    sp, pl = _sweep_loop(sp_body), _sweep_loop(pl_body)
    print("spare:", sorted(sp.items()), "VALU", _count(sp, "v_"), "vgpr", sp_vgpr)
    print("plain:", sorted(pl.items()), "VALU", _count(pl, "v_"))
    assert _count(pl, "v_add_f32") == 12 and _count(pl, "v_") == 78, pl       # what the spare form is measured against
    assert _count(sp, "v_rsq_f32") == 4, sp                                     # four rows per iteration
    assert sp["v_pk_fma_f32"] == 48, sp
    assert _count(sp, "v_add_f32") <= 4, sp                                     # the add of the two halves alone
    assert _count(sp, "v_") <= 74, (_count(sp, "v_"), sp)
    assert _count(sp, "v_readlane") + _count(sp, "v_writelane") == 0, sp        # no SGPR parked in VGPR lanes
    assert _count(sp, "scratch_") == 0, sp
    assert sp_vgpr <= 64, sp_vgpr
