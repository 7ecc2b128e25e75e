"""Records tests/golden/motion_parent_bits.npz: every output of tests/motion_parent_bits_cases.py run_all() from the library
DCX_LIB names - the build of the commit BEFORE the motion kernels were moved onto motion_tile.h (tools/build_variant.sh parent ""
"2 4 12 24" in a checkout of that commit; the cases use the widths 4, 12 and 24 and one and five classes).  Run once, on the GPU:

    DCX_LIB=/path/to/libdcx_parent.so python tools/record_motion_parent_bits.py

Never run it on the library under test: tests/test_gpu_motion_parent_bits.py compares the shipped library with this file."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    if not os.environ.get("DCX_LIB"):
        sys.exit("set DCX_LIB to the parent commit's library")
    import motion_parent_bits_cases as cases
    from diffco_amd import _lib, _ops
    lib = _lib.require_gpu()
    knob = lambda name, v: _lib.check(lib.dcx_debug_set(name.encode(), int(v)))
    out = cases.run_all(_ops, knob, lambda v: knob("motion_early_exit", v))
    n = out["cfg2_baxter_poly1|step|check_n_samples_ee1"][0]
    assert cases.layout_ok(n), "the work list lost the layout the cases exist for"
    path = os.path.join(ROOT, "tests", "golden", "motion_parent_bits.npz")
    np.savez_compressed(path, **out)
    print(f"{len(out)} arrays, {os.path.getsize(path)} bytes -> {path}")


if __name__ == "__main__":
    main()
