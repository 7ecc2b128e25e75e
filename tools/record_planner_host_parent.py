"""Records what the host side of the planner calls and every workspace layout answered BEFORE they were moved onto one prelude
(PlannerCheck) and one carver (work_layout.h), from the library DCX_LIB names - the build of the parent commit
(tools/build_variant.sh parent "" "4 12" in a checkout of that commit; the models use the widths 4 and 12, one and five classes):

    DCX_LIB=/path/to/libdcx_parent.so python tools/record_planner_host_parent.py cpu    # anywhere: no device is touched
    DCX_LIB=/path/to/libdcx_parent.so python tools/record_planner_host_parent.py gpu    # on the GPU: three models are created

cpu -> tests/golden/planner_boundary_parent.json: (rc, message) of every case of tests/planner_boundary_cases.py and the planners'
       size queries on the stand-in model;  gpu -> tests/golden/planner_work_bytes_parent.json: every size query on real models.
Never run it on the library under test: tests/test_planner_boundary_recorded.py and tests/test_gpu_work_bytes_recorded.py compare
the shipped library with these files."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    if not os.environ.get("DCX_LIB"):
        sys.exit("set DCX_LIB to the parent commit's library")
    if sys.argv[1:] not in (["cpu"], ["gpu"]):
        sys.exit("usage: record_planner_host_parent.py cpu|gpu")
    import planner_boundary_cases as cases
    from diffco_amd import _lib
    if sys.argv[1] == "cpu":
        boundary, sizes = cases.run_boundary(_lib.load())
        assert all(rc != 0 for c in boundary.values() for rc, _ in c.values()), "a case was not refused"
        name, out = cases.GOLDEN_BOUNDARY, {"boundary": boundary, "work_bytes": sizes}
    else:
        from diffco_amd import _ops
        lib = _lib.require_gpu()
        name, out = cases.GOLDEN_WORK_BYTES, cases.run_work_bytes(lib, cases.build_models(_ops))
    path = os.path.join(ROOT, "tests", "golden", name)
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print(f"{os.path.getsize(path)} bytes -> {path}")


if __name__ == "__main__":
    main()
