"""The fp64 referee of the worst-sample motion queries (dcx_motion_worst) on helpers.motion_samples / helpers.motion_scores,
and the small pieces its GPU tests share.  Plain numpy: importable without a GPU."""
import numpy as np

from helpers import motion_samples, motion_scores

TIE_BAND = 1e-4   # of max |s|: the project's tie band (tests/test_gpu_motion_cost.py, helpers.motion_oracle)


def worst_oracle(desc, kern, sup, W, samples, margin, scores=None, grad=True):
    """the fp64 referee on the given samples (helpers.motion_samples' tuples), a dict: per edge 'worst' (max over its samples k
    and classes c of s_c(x_k) - margin_c), 'idx' (the smallest k that attains it), 'cls' (the smallest c that attains it at that
    k), 'tie' (the runner-up - another sample or another class - lies within TIE_BAND * max|s| of the peak, so fp32 may pick
    it), 'n'; with grad=True 'ga', 'gb' [E, dof]: the gradient of the peak through the worst sample alone, chained to the
    endpoints as helpers.motion_chain chains one sample; 's' [N, C] and 's_max' = max|s| (the scale of the tolerances).
    An edge without samples answers NaN / -2 / -1 and is flagged as a tie (nothing to compare)."""
    from oracle import oracle
    s = motion_scores(desc, kern, sup, W, samples) if scores is None else scores
    C = s.shape[1]
    dof = desc.dof
    mg = np.broadcast_to(np.asarray(margin, np.float64).reshape(-1), (C,))
    s_max = float(np.abs(s).max(initial=0))
    band = TIE_BAND * s_max
    E = len(samples)
    worst, idx, cls, tie = np.full(E, np.nan), np.full(E, -2, int), np.full(E, -1, int), np.ones(E, bool)
    ends = np.cumsum([0] + [len(p) for p, *_ in samples])
    for e in range(E):
        v = s[ends[e]:ends[e + 1]] - mg
        if len(v) == 0:
            continue
        flat = int(np.argmax(v))             # the first maximum in (k, c) order: the smallest k, then the smallest c
        idx[e], cls[e] = divmod(flat, C)
        worst[e] = v.reshape(-1)[flat]
        rest = np.delete(v.reshape(-1), flat)
        tie[e] = bool(len(rest) and worst[e] - rest.max() <= band)
    out = dict(worst=worst, idx=idx, cls=cls, tie=tie, n=np.diff(ends), s=s, s_max=s_max)
    if grad:
        has = idx >= 0
        x = np.stack([samples[e][0][idx[e]] if has[e] else np.zeros(dof) for e in range(E)]) if E else np.zeros((0, dof))
        up = np.zeros((E, C))
        up[np.nonzero(has)[0], cls[has]] = 1.0
        g = oracle.score_grad(desc, kern[0], kern[1], kern[2], sup, W, x, upstream=up, dtype=np.float64)[1] if E else np.zeros((0, dof))
        ga, gb = np.full((E, dof), np.nan), np.full((E, dof), np.nan)
        for e in np.nonzero(has)[0]:
            _, t, u, tgt = samples[e]
            k = idx[e]
            if u is None:                    # res rule
                gb[e], ga[e] = t[k] * g[e], (1 - t[k]) * g[e]
            elif tgt[k]:                     # the closed rule's target carries identity to grad_b
                gb[e], ga[e] = g[e], np.zeros(dof)
            else:
                gb[e] = t[k] * (g[e] - u * (u @ g[e]))
                ga[e] = g[e] - gb[e]
        out.update(ga=ga, gb=gb, g=g)
    return out


def check_against_oracle(got, ref, what, min_keep=None, grads=True):
    """got: (worst, idx, cls[, ga, gb]) numpy; ref: worst_oracle's dict.  Values on every edge within 1e-5 max|s| (a max is
    1-Lipschitz in the scores: no tie exclusion); index and class equal and gradients within 1e-4 of their scale on the edges
    outside the tie band, of which there must be at least min_keep."""
    worst, idx, cls = (np.asarray(x) for x in got[:3])
    keep = ~ref["tie"]
    if min_keep is not None:
        assert keep.sum() >= min_keep, (what, int(keep.sum()))
    err = np.abs(worst.astype(np.float64) - ref["worst"])
    print(f"{what}: value err {err.max(initial=0):.3e} (bound {1e-5 * ref['s_max']:.3e}), kept {int(keep.sum())} / {len(keep)}")
    assert err.max(initial=0) <= 1e-5 * ref["s_max"], (what, err.max(), ref["s_max"])
    assert (idx[keep] == ref["idx"][keep]).all(), (what, np.nonzero(idx[keep] != ref["idx"][keep]))
    assert (cls[keep] == ref["cls"][keep]).all(), (what, np.nonzero(cls[keep] != ref["cls"][keep]))
    if grads and len(got) > 3:
        ga, gb = (np.asarray(x, np.float64) for x in got[3:5])
        gs = max(np.abs(ref["ga"][keep]).max(initial=0), np.abs(ref["gb"][keep]).max(initial=0), 1e-30)
        ea = np.abs(ga[keep] - ref["ga"][keep]).max(initial=0)
        eb = np.abs(gb[keep] - ref["gb"][keep]).max(initial=0)
        print(f"{what}: gradient err {ea:.3e} / {eb:.3e} (bound {1e-4 * gs:.3e})")
        assert ea <= 1e-4 * gs, (what, ea, gs)
        assert eb <= 1e-4 * gs, (what, eb, gs)


def class_margins(scores64, pct):
    """per-class margins at a percentile of a fixture's fp64 scores"""
    return np.percentile(scores64, pct, axis=0).astype(np.float32).tolist()


def samples32(qa, qb, res=None, max_step=None):
    """the fp32 samples of the closed sample set (check_motions')"""
    return motion_samples(qa, qb, res, max_step, False)


# ---- the fixtures of the GPU oracle test (tests/test_gpu_motion_worst.py), shared with the CPU guard of its tie condition ----
ORACLE_FIXTURES = ["cfg1_planar2_rq", "cfg2_baxter_poly1", "cfg2_panda_rq", "cfg4_se3_nofk_rq", "cfg3_baxter_rq_c5"]
ORACLE_EDGES, ORACLE_MIN_KEEP = 300, 200
_cache = {}


def fixture_model(name):
    """(fixture, FK description, kernel triple, fp32 supports [S, D], fp32 weights [S, C]) of a golden case"""
    from helpers import CASE_ROBOT, case_kernel, desc_for, load
    d = load(name)
    desc = desc_for(CASE_ROBOT[name], dof=d["q"].shape[1])
    sup = d["sup_x32"].reshape(len(d["sup_x32"]), -1) if "sup_x32" in d.files and CASE_ROBOT[name] else d["sup_q"]
    sup = np.asarray(sup, dtype=np.float32).reshape(len(sup), -1)
    return d, desc, case_kernel(d), sup, np.asarray(d["weights"], np.float32)


def fixture_edges(q, E, seed, scale=1.0):
    """tests/test_gpu_motions.py's _edges"""
    g = np.random.default_rng(seed)
    i, j = g.integers(0, len(q), E), g.integers(0, len(q), E)
    qa = q[i].astype(np.float32)
    qb = (qa + scale * (q[j] - qa)).astype(np.float32)
    return qa, qb


def oracle_case(name, rule, margin_kind):
    """the GPU oracle test's inputs and its fp64 reference, computed once per (fixture, rule, margins): a dict with qa, qb, the
    call's keywords, the margins ("zero": 0; "pct": per-class percentiles of the fixture's scores) and worst_oracle's result"""
    key = (name, rule, margin_kind)
    if key not in _cache:
        d, desc, kern, sup, W = fixture_model(name)
        qa, qb = fixture_edges(d["q"], ORACLE_EDGES, 1)
        if rule == "res":
            kw = dict(res=13)
        else:
            span = float(np.median(np.linalg.norm(qb - qa, axis=1)))
            kw = dict(max_step=max(span / 20, 1e-3))
        C = W.reshape(len(W), -1).shape[1]
        margin = [0.0] * C if margin_kind == "zero" else class_margins(d["score64"], 70 if C == 1 else 95)
        smp = samples32(qa, qb, kw.get("res"), kw.get("max_step"))
        skey = (name, rule)
        if skey not in _cache:   # the scores do not depend on the margins
            _cache[skey] = motion_scores(desc, kern, sup, W, smp)
        ref = worst_oracle(desc, kern, sup, W, smp, margin, scores=_cache[skey])
        _cache[key] = dict(qa=qa, qb=qb, kw=kw, margin=margin, ref=ref, smp=smp, model=(desc, kern, sup, W))
    return _cache[key]


# ---- the cases of the shape fuzz (tests/test_gpu_motion_worst_fuzz.py), built without a GPU so that the CPU guard in
# tests/test_motion_worst_referee.py can hold every case to the fuzz's keep condition before anything runs on a device ----
FUZZ_MIN_KEEP = 0.7      # of the judged edges, outside the tie band: the sibling fuzzes' share (tests/test_gpu_fuzz.py)
FUZZ_RUN = 70            # edges in a run of empty ones: more than the 64 samples of one tile end there
FUZZ_STEP_DIV = 8        # max_step = the median edge length / this
FUZZ_SCALE = (0.15, 3.0)  # an edge is this share of the way to a random configuration (log-uniform)


def fuzz_case(case):
    """model inputs, edges, the fp32 samples and the fp64 referee of one entry of helpers.MOTION_CASES, with the sizes of
    tests/test_gpu_fuzz.py's _motion_setup (S from {37, 150, 333, 1000}, 150 - 300 edges, res in 7 .. 13, runs of 70 empty
    edges) and the dict keys its _motion_legs reads.  What is this fuzz's own: the supports' features come from the fp64 oracle
    (no device), and under max_step the samples lie further apart - step = median length / 8 and edges of 0.15 - 3 times the way
    to a random configuration instead of / 30 and 0.001 - 4 - because the peak's runner-up is usually its neighbour sample: a
    thirtieth of an edge away, or on an edge a thousandth of the space long, it lies inside the tie band and the edge could not be
    judged on index, class and gradient.  Rule "open" runs as "closed"."""
    import zlib
    from helpers import KERNELS, fuzz_desc
    from oracle import oracle
    if case in _cache:
        return _cache[case]
    F = np.float32
    kind, D, C, ki, rule, empty = case
    rng = np.random.default_rng(zlib.crc32(repr(("motion worst", case)).encode()))
    desc, dof, lim = fuzz_desc(kind, D, rng)
    kern = KERNELS[ki]
    S = int(rng.choice([37, 150, 333, 1000]))
    cfg = lambda n: rng.uniform(lim[:, 0], lim[:, 1], (n, dof)).astype(F)  # noqa: E731
    sup = oracle.fkine(desc, cfg(S).astype(np.float64), dtype=np.float64).reshape(S, -1).astype(F)
    assert sup.shape[1] == D
    W = rng.standard_normal((S, C)).astype(F)
    W[rng.random((S, C)) < 0.2] = 0.0
    E = int(rng.integers(150, 301))
    qa, far = cfg(E), cfg(E)
    if rule == "res":
        kw = dict(res=int(rng.integers(7, 14)))
        qb = far
    else:
        step = float(np.median(np.linalg.norm(far - qa, axis=1))) / FUZZ_STEP_DIV
        scale = np.exp(rng.uniform(np.log(FUZZ_SCALE[0]), np.log(1.5 if empty else FUZZ_SCALE[1]), E))
        scale[rng.random(E) < 0.03] = 0.0   # zero length: one sample (qb)
        qb = (qa + scale[:, None] * (far - qa)).astype(F)
        kw = dict(max_step=step)
    smp = samples32(qa, qb, kw.get("res"), kw.get("max_step"))
    ms = max(len(p) for p, *_ in smp)
    over = np.zeros(E, bool)
    if empty:   # after 20 edges: a run of zero-length edges, then a run of edges over max_samples, then the rest
        dirn = rng.standard_normal((FUZZ_RUN, dof))
        dirn /= np.linalg.norm(dirn, axis=1, keepdims=True)
        a0 = cfg(2 * FUZZ_RUN)
        b0 = np.concatenate([a0[:FUZZ_RUN], a0[FUZZ_RUN:] + dirn * kw["max_step"] * (ms + 20)]).astype(F)
        qa, qb = np.concatenate([qa[:20], a0, qa[20:]]), np.concatenate([qb[:20], b0, qb[20:]])
        smp = samples32(qa, qb, kw.get("res"), kw.get("max_step"))
        over = np.array([len(p) > ms for p, *_ in smp])
        assert over.sum() == FUZZ_RUN
    counts = np.array([len(p) for p, *_ in smp])
    judged = [(p[:0], t[:0], u, g[:0]) if o else (p, t, u, g) for (p, t, u, g), o in zip(smp, over)]
    s = motion_scores(desc, kern, sup, W, judged)
    # per-class margins: a quantile of the edges' largest scores, so that about half of the edges rise above some class's
    ends = np.cumsum([0] + [len(p) for p, *_ in judged])
    emax = np.stack([s[ends[e]:ends[e + 1]].max(0) for e in range(len(judged)) if ends[e + 1] > ends[e]])
    margin = np.quantile(emax, 1 - 0.5 / C, axis=0).astype(F)
    ref = worst_oracle(desc, kern, sup, W, judged, margin.astype(np.float64), scores=s)
    _cache[case] = dict(desc=desc, kern=kern, sup=sup, W=W, qa=qa, qb=qb, kw=kw, ms=ms, over=over, counts=counts, margin=margin,
                        ref=ref, device_margin=bool(rng.random() < 0.5), nw=int(rng.choice([1, 2, 4, 8])),
                        ys=int(rng.choice([2, 4])), derived_bound=bool(rng.random() < 0.5) and not empty, S=S, dof=dof)
    return _cache[case]
