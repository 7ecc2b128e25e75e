"""Records tests/golden/sweep_lookahead_parent_bits.npz: score and gradient of every launch of tests/sweep_lookahead_cases.py
run_all() from the library DCX_LIB names - the build of the commit BEFORE the four-row pipeline of the sweep took its rows through
one advancing pointer with an unclamped look-ahead (tools/build_variant.sh parent "" "12" in a checkout of that commit; the cases
use the width 12 and one class).  Run once, on the GPU:

    DCX_LIB=/path/to/libdcx_parent.so python tools/record_sweep_lookahead_parent_bits.py [output.npz]

Never run it on the library under test: tests/test_gpu_sweep_lookahead.py compares the shipped library with this file."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    if not os.environ.get("DCX_LIB"):
        sys.exit("set DCX_LIB to the parent commit's library")
    import sweep_lookahead_cases as cases
    from diffco_amd import _lib
    lib = _lib.require_gpu()
    out, plain, _ = cases.run_all(lambda name, v: _lib.check(lib.dcx_debug_set(name.encode(), int(v))))
    assert sorted(out) == sorted(cases.keys())
    same = [k for k in out if np.array_equal(out[k][0], plain[k][0]) and np.array_equal(out[k][1], plain[k][1])]
    assert not same, f"the spare form did not run: {same}"
    arrays = {}
    for k, (s, g) in out.items():
        assert np.isfinite(s).all() and np.isfinite(g).all(), k
        arrays[k + "_s"], arrays[k + "_g"] = s, g
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "sweep_lookahead_parent_bits.npz")
    np.savez_compressed(path, **arrays)
    print(f"{len(arrays)} arrays, {os.path.getsize(path)} bytes -> {path}")


if __name__ == "__main__":
    main()
