"""GPU: the shape fuzz of the worst-sample motion queries.  Every entry of helpers.MOTION_CASES - every compiled width, padded
widths, 1 to 8 classes, every kernel family and FK kind, runs of empty edges - with the sizes and launch legs of
tests/test_gpu_fuzz.py's test_motion_checks_shapes (rule "open" runs as "closed": the call has no open_end) and edges of this
fuzz's own (motion_worst_helpers.fuzz_case: samples far enough apart that at least 70 % of every case's edges lie outside the
tie band - tests/test_motion_worst_referee.py holds every case to that on the CPU), judged by the fp64 referee as
tests/test_gpu_motion_worst.py judges its fixtures: the value on every edge within 1e-5 max|s|; index and class outside the
tie band, and there - on every third case - the endpoint gradients."""
import numpy as np
import pytest

from helpers import MOTION_CASES
from motion_worst_helpers import FUZZ_MIN_KEEP, check_against_oracle, fuzz_case
from test_gpu_fuzz import _margin_arg, _motion_id, _motion_legs, _n, _t

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("ci", range(len(MOTION_CASES)), ids=[_motion_id(c) for c in MOTION_CASES])
def test_motion_worst_shapes(ci, knob):
    from diffco_amd import _ops
    case = MOTION_CASES[ci]
    grads = ci % 3 == 0
    x = fuzz_case(case)
    m = _ops.ScoreModel(x["desc"], *x["kern"], _t(x["sup"]), _t(x["W"]))
    over, counts, kw, ref = x["over"], x["counts"], x["kw"], x["ref"]
    norm = ~over
    keep = norm & ~ref["tie"]
    assert keep.sum() >= FUZZ_MIN_KEEP * norm.sum(), (case, int(keep.sum()), int(norm.sum()))
    assert (ref["worst"][keep] > 0).any() and (ref["worst"][keep] < 0).any(), case
    fields = ("worst", "idx", "cls", "tie") + (("ga", "gb") if grads else ())
    for name, knobs, sl in _motion_legs(case, x):
        for k, v in knobs.items():
            knob(k, v)
        ms = None if (x["derived_bound"] and name == "default") else x["ms"]
        runs = []
        for _ in range(2 if name == "split" else 1):
            got = m.motion_worst_raw(_t(x["qa"][sl]), _t(x["qb"][sl]), res=kw.get("res"), max_step=kw.get("max_step"),
                                     margin=_margin_arg(x), max_samples=ms if kw.get("res") is None else None, grad=grads)
            runs.append([_n(v) for v in got])
        for k in knobs:
            knob(k, -1)
        what = (case, name, len(runs[0][0]))
        if name == "split":   # the same bits on a second call
            for a, b in zip(runs[0], runs[1]):
                assert np.array_equal(a, b, equal_nan=True), what
        worst, idx, cls, n = runs[0][:4]
        assert n.tolist() == counts[sl].tolist(), what
        o, nm = over[sl], norm[sl]
        assert np.isnan(worst[o]).all() and (idx[o] == -2).all() and (cls[o] == -1).all(), what
        assert (idx[nm] >= 0).all() and (idx[nm] < n[nm]).all() and (cls[nm] >= 0).all() and (cls[nm] < x["W"].shape[1]).all(), what
        sub = dict(ref, **{k: ref[k][sl][nm] for k in fields})
        got = [worst[nm], idx[nm], cls[nm]]
        if grads:
            ga, gb = runs[0][4:6]
            assert np.isnan(ga[o]).all() and np.isnan(gb[o]).all(), what
            got += [ga[nm], gb[nm]]
        check_against_oracle(got, sub, what, grads=grads)
        if name == "default":
            # worst > 0 exactly where check_motions finds a hit: the two calls score a sample to the same bits
            first, _ = m.check_motions(_t(x["qa"]), _t(x["qb"]), res=kw.get("res"), max_step=kw.get("max_step"),
                                       margin=_margin_arg(x), max_samples=ms if kw.get("res") is None else None)
            first = _n(first)
            assert ((worst > 0)[nm] == (first >= 0)[nm]).all(), what
            hit = nm & (first >= 0)
            assert (first[hit] <= idx[hit]).all(), what
