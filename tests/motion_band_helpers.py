"""The fp64 referee of the hybrid motion checks (dcx_motion_band) on helpers.motion_samples / helpers.motion_scores, and the
cases its GPU oracle test shares with the CPU guard of that test's condition.  Plain numpy: importable without a GPU."""
import numpy as np

from motion_worst_helpers import ORACLE_EDGES, ORACLE_FIXTURES, TIE_BAND, class_margins, oracle_case

BAND_RULES = ("res", "max_step")
BAND_MIN_JUDGED, BAND_MIN_EACH = 270, 15      # of the 300 edges of a case: judged edges, and edges of each verdict among them
_cache = {}


def band_codes(s, lo, hi):
    """per-sample codes from class scores s [N, C]: 1 some class above hi, else 0 every class at or below lo, else 2 (a NaN
    score is neither a hit nor clear)"""
    s = np.asarray(s)
    C = s.shape[1]
    lo = np.broadcast_to(np.asarray(lo, s.dtype).reshape(-1), (C,))
    hi = np.broadcast_to(np.asarray(hi, s.dtype).reshape(-1), (C,))
    hit = (s - hi[None] > 0).any(axis=1)
    clear = (s - lo[None] <= 0).all(axis=1)
    return np.where(hit, 1, np.where(clear, 0, 2)).astype(np.int32)


def band_fold(codes, counts, over=None):
    """the per-edge results and the list from per-sample codes in flat (edge, sample) order and the edges' sample counts: a dict
    with 'verdict', 'first', 'n_unc' [E], 'unc_edge', 'unc_sample' (the code-2 samples of the verdict-2 edges, ordered) and
    'total'.  `over` [E] bool: edges over max_samples (no samples among the codes): -2 / -2 / 0, nothing listed."""
    counts = np.asarray(counts, np.int64)
    E = len(counts)
    ends = np.concatenate([[0], np.cumsum(counts)])
    verdict, first, n_unc = np.zeros(E, np.int32), np.full(E, -1, np.int32), np.zeros(E, np.int32)
    ue, us = [], []
    for e in range(E):
        if over is not None and over[e]:
            verdict[e], first[e] = -2, -2
            continue
        c = codes[ends[e]:ends[e + 1]]
        hits = np.nonzero(c == 1)[0]
        unc = np.nonzero(c == 2)[0]
        if len(hits):
            verdict[e], first[e] = 1, hits[0]
        elif len(unc):
            verdict[e], n_unc[e] = 2, len(unc)
            ue += [e] * len(unc)
            us += unc.tolist()
    return dict(verdict=verdict, first=first, n_unc=n_unc, unc_edge=np.array(ue, np.int32), unc_sample=np.array(us, np.int32),
                total=len(ue))


def band_oracle(samples, s, lo, hi):
    """the fp64 referee on the given samples (helpers.motion_samples' tuples) and their fp64 class scores s [N, C]: band_fold's
    dict plus 'codes', 'n' (the sample counts), 'judged' [E] - no sample of the edge has a class score within TIE_BAND * max|s|
    of that class's lo or hi, so fp32 cannot code one of its samples differently - and 's_max'"""
    s = np.asarray(s, np.float64)
    C = s.shape[1]
    counts = np.array([len(p) for p, *_ in samples], np.int64)
    lo = np.broadcast_to(np.asarray(lo, np.float64).reshape(-1), (C,))
    hi = np.broadcast_to(np.asarray(hi, np.float64).reshape(-1), (C,))
    codes = band_codes(s, lo, hi)
    out = band_fold(codes, counts)
    s_max = float(np.abs(s).max(initial=0))
    near = ((np.abs(s - lo[None]) <= TIE_BAND * s_max) | (np.abs(s - hi[None]) <= TIE_BAND * s_max)).any(axis=1)
    ends = np.concatenate([[0], np.cumsum(counts)])
    judged = np.array([not near[ends[e]:ends[e + 1]].any() for e in range(len(counts))], bool)
    out.update(codes=codes, n=counts, judged=judged, s_max=s_max)
    return out


def band_case(name, rule):
    """one of the ten cases of the GPU oracle test: the fixture's 300 edges of motion_worst_helpers.oracle_case (fixture_edges(q,
    300, 1); res = 13, or the closed rule at max_step = the median length / 20), lo / hi at the per-class 90th / 97th percentile
    of the fixture's fp64 scores, and band_oracle's result on the fp64 scores of the fp32 samples"""
    key = (name, rule)
    if key not in _cache:
        from helpers import load
        c = oracle_case(name, rule, "zero")          # (the edges, the samples and their fp64 scores are computed once and shared)
        assert len(c["qa"]) == ORACLE_EDGES == 300
        s64 = load(name)["score64"]
        lo, hi = class_margins(s64, 90), class_margins(s64, 97)
        _cache[key] = dict(qa=c["qa"], qb=c["qb"], kw=c["kw"], lo=lo, hi=hi, smp=c["smp"], model=c["model"],
                           ref=band_oracle(c["smp"], c["ref"]["s"], lo, hi))
    return _cache[key]


def judged_list(ref, judged=None):
    """the (edge, sample) pairs of the list on the judged edges, as a list of tuples"""
    judged = ref["judged"] if judged is None else judged
    return [(int(e), int(k)) for e, k in zip(ref["unc_edge"], ref["unc_sample"]) if judged[e]]


# ---- the listed configurations, bit for bit ------------------------------------------------------------------------------------
def _round32(x):
    """the float32 nearest to the exact rational x, ties to even (a float64 in between would round twice)"""
    from fractions import Fraction
    f = np.float32(float(x))
    best = None
    for c in (np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))):
        if not np.isfinite(c):
            continue
        err = abs(Fraction(float(c)) - x)
        even = (int(np.float32(c).view(np.uint32)) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even and not best[2]):
            best = (err, c, even)
    return np.float32(best[1])


def _fma32(a, b, c):
    """float32 fused multiply-add: a * b + c rounded once"""
    from fractions import Fraction
    return _round32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def listed_points32(qa, qb, mask, edges, samples, res=None, max_step=None):
    """the configurations of the samples (edges[i], samples[i]) as the device forms them (motion_tile.h motion_coord), fp32:
    masked coordinates operation by operation (motion_wrap_helpers.motion_samples_wrapped, the wrap tests' restatement);
    unmasked coordinates with the last product and sum of helpers.motion_samples' expression fused, as the compiler contracts
    them: qa + d (k / res) -> fma(d, k / res, qa), qa + k (d frac) -> fma(k, d frac, qa); the closed rule's target is qb."""
    from motion_wrap_helpers import mask_bits, motion_samples_wrapped
    F = np.float32
    qa, qb = np.asarray(qa, F), np.asarray(qb, F)
    on = mask_bits(mask, qa.shape[1])
    out = np.zeros((len(edges), qa.shape[1]), F)
    memo = {}
    for i, (e, k) in enumerate(zip(edges, samples)):
        e, k = int(e), int(k)
        if e not in memo:
            memo[e] = motion_samples_wrapped(qa[e:e + 1], qb[e:e + 1], mask, res, max_step)[0]
        p, _, _, tgt = memo[e]
        out[i] = p[k]
        if tgt[k]:
            continue
        a, b = qa[e], qb[e]
        d = (b - a).astype(F)
        if res is None:
            l2 = F(0)
            dw = np.where(on, _wrapped(a, b), d).astype(F)   # (the length takes the wrapped delta of the masked coordinates)
            for v in dw:
                l2 = F(l2 + F(v * v))
            L = F(np.sqrt(l2))
            frac = F(F(F(1) / L) * F(max_step))
        for j in np.nonzero(~on)[0]:
            out[i, j] = _fma32(d[j], F(F(k) / F(res)), a[j]) if res is not None else _fma32(F(k), F(d[j] * frac), a[j])
    return out


def _wrapped(a, b):
    from motion_wrap_helpers import wrap2pi32
    return wrap2pi32((np.asarray(b, np.float32) - np.asarray(a, np.float32)).astype(np.float32))


__all__ = ["BAND_RULES", "BAND_MIN_JUDGED", "BAND_MIN_EACH", "ORACLE_FIXTURES", "band_codes", "band_fold", "band_oracle",
           "band_case", "judged_list", "listed_points32"]
