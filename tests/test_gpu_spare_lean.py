"""GPU tests of the lean stage of the spare-slot sweep (score_kernel.h sweep_rows SP, stage_x / single_x): the near gate stands in
front of the accumulation - raw distances of a stage's two rows, one ballot of !(d2 > thr), and only a stage with a near or NaN lane
runs the clamped sequence plus the near-pair block - and the two rows' coefficient multiplies ride in one packed multiply.  Neither
may move a bit: the skipped clamp was an identity wherever it is skipped, the packed multiply is the same IEEE multiply, and a
lane's result never depends on its wave-mates.  Held here: every position a coincident pair can take in the pipeline (first / second
row of a stage, the tail rows, odd slice starts) against the fp64 oracle at test_gpu_parity.py's TOL; wave-mates of a near lane and
of a NaN lane bit for bit; and the bits of the commit before the lean stage, recorded with that commit's library from the same
inputs (tests/golden/spare_lean_parent_bits.npz: keys <case>_<kernel>_s / _g; the seeds are below)."""
import numpy as np
import pytest
import torch

from helpers import load, make_robot, relerr

pytestmark = pytest.mark.gpu

TOL = 1e-5                      # test_gpu_parity.py: max|a - ref| / max|ref| against the fp64 referee
B = 70                          # one full tile + six lanes
SIZES = (200, 201, 202, 203)    # four waves' slices of ~50 rows: tails of 0 - 3 rows, odd slice starts
N_ON_TOP = 64                   # queries 0 .. 63 = support configurations 0 .. 63
KERNELS = {"poly1": (1, 1.0, 1.0), "rq2": (0, 10.0, 2.0)}
MATE = 17                       # the row of the wave-mates test that is replaced
MATE_SUPPORT = 101              # ... by this support configuration (second slice of S = 203, an odd row)


def _inputs(S):
    """(robot, support configurations [S, dof], weights [S], stage-position queries [B, dof], random queries [B, dof]); CPU tensors"""
    rob = make_robot("baxter_left")
    g = torch.Generator().manual_seed(1700 + S)
    lim = rob.limits
    rnd = lambda n: torch.rand((n, rob.dof), generator=g) * (lim[:, 1] - lim[:, 0]) + lim[:, 0]
    sup_q = rnd(S)
    w = 0.05 * torch.randn(S, generator=g)
    q_top = torch.cat([sup_q[:N_ON_TOP], rnd(B - N_ON_TOP)]).contiguous()
    return rob, sup_q, w, q_top, rnd(B)


def mates_queries(sup_q, q_rand):
    """the three batches of the wave-mates test: random, one query on top of a support, one query NaN"""
    near, nan = q_rand.clone(), q_rand.clone()
    near[MATE] = sup_q[MATE_SUPPORT]
    nan[MATE] = float("nan")
    return {"mates_random": q_rand, "mates_near": near, "mates_nan": nan}


def run_all(set_knob):
    """every launch of this file: {"<case>_<kernel>": (score, gradient)} as CUDA tensors, plus what the oracle needs.  The spare
    form is shown to have run (knob spare = 0 moves the last bits) where the case is random."""
    from diffco_amd import _lib, _ops
    _lib.require_gpu()
    set_knob("nw", 4)
    set_knob("ys", 1)
    set_knob("spare", -1)
    out, ctx = {}, {}
    for S in SIZES:
        rob, sup_q, w, q_top, q_rand = _inputs(S)
        desc = rob.fk_desc()
        sup = _ops.fkine(desc, sup_q.cuda()).reshape(S, -1).contiguous()
        assert float(sup[:, 2].max() - sup[:, 2].min()) == 0.0      # the column the form lives on
        ctx[S] = dict(desc=desc, sup_q=sup_q, sup=sup, w=w.cuda(), q_top=q_top.cuda())
        for kname, kern in KERNELS.items():
            m = _ops.ScoreModel(desc, *kern, sup, w.cuda())
            out[f"stage{S}_{kname}"] = m.score_grad_raw(q_top.cuda())
            if S == SIZES[-1]:
                for tag, q in mates_queries(sup_q, q_rand).items():
                    out[f"{tag}_{kname}"] = m.score_grad_raw(q.cuda())
                set_knob("spare", 0)
                plain = m.score_grad_raw(q_rand.cuda())
                set_knob("spare", -1)
                rule = out[f"mates_random_{kname}"]
                assert not (torch.equal(rule[0], plain[0]) and torch.equal(rule[1], plain[1])), "the spare form did not run"
    return out, ctx


@pytest.fixture(scope="module")
def runs():
    from diffco_amd import _lib
    lib = _lib.require_gpu()
    set_knob = lambda name, v: _lib.check(lib.dcx_debug_set(name.encode(), int(v)))
    try:
        yield run_all(set_knob)
    finally:
        for k in ("nw", "ys", "spare"):
            lib.dcx_debug_set(k.encode(), -1)


@pytest.mark.parametrize("kname", sorted(KERNELS))
@pytest.mark.parametrize("S", SIZES)
def test_coincident_pairs_at_every_stage_position(runs, S, kname):
    """queries 0 .. 63 sit on supports 0 .. 63: with slices of ~50 rows the one coincident pair of a lane lands on the first and
    on the second row of stages and in the tails of 0 - 3 rows; score and gradient against float64"""
    from oracle import oracle
    out, ctx = runs
    c = ctx[S]
    s, g = out[f"stage{S}_{kname}"]
    # (the referee walks the arm in float64: it gets ITS OWN features of the support configurations, so that the coincident
    # pairs coincide there as well - test_gpu_spare_slot.py test_queries_on_top_of_supports)
    sup64 = oracle.fkine(c["desc"], c["sup_q"].numpy().astype(np.float64), dtype=np.float64).reshape(S, -1)
    so, go, _ = oracle.score_grad(c["desc"], *KERNELS[kname], sup64, c["w"].cpu().numpy().astype(np.float64),
                                  c["q_top"].cpu().numpy().astype(np.float64), dtype=np.float64)
    es, eg = relerr(s.cpu().numpy(), so.reshape(s.shape)), relerr(g.cpu().numpy(), go)
    print(f"S={S} {kname}: score {es:.2e} grad {eg:.2e}")
    assert torch.isfinite(s).all() and torch.isfinite(g).all()
    assert es < TOL and eg < TOL, (S, kname, es, eg)


@pytest.mark.parametrize("kname", sorted(KERNELS))
def test_wave_mates_do_not_see_a_near_or_nan_lane(runs, kname):
    """one query of a random batch replaced by a support configuration (its stage takes the cold side), then by NaN (the negated
    compare sends it there too): every other row keeps its bits"""
    out, _ = runs
    s0, g0 = out[f"mates_random_{kname}"]
    keep = torch.arange(B, device=s0.device) != MATE
    for tag in ("mates_near", "mates_nan"):
        s, g = out[f"{tag}_{kname}"]
        assert torch.equal(s[keep], s0[keep]) and torch.equal(g[keep], g0[keep]), (tag, kname)
    s, g = out[f"mates_near_{kname}"]
    assert torch.isfinite(s[MATE]).all() and torch.isfinite(g[MATE]).all()


@pytest.mark.parametrize("kname", sorted(KERNELS))
def test_nan_query_gives_nan_score_and_gradient(runs, kname):
    """the NaN row of the wave-mates runs is NaN in score and gradient.  (Polyharmonic(1): every pair of a NaN configuration is a
    near pair - fmaxf(NaN, thr) = thr - and the near-pair block hands the NaN distance on to the score; before the lean stage
    kernel_eval's clamp turned it into 1e-15 per support there: score 6.876e-16 beside a NaN gradient)"""
    out, _ = runs
    s, g = out[f"mates_nan_{kname}"]
    print(f"{kname}: NaN row score {s[MATE].flatten().tolist()} grad {g[MATE].flatten().tolist()}")
    assert torch.isnan(s[MATE]).all() and torch.isnan(g[MATE]).all(), (kname, s[MATE], g[MATE])


def test_bits_of_the_commit_before_the_lean_stage(runs):
    """every output of the tests above, both kernels, equals what the parent commit's library gave for the same inputs - but for
    ONE number: the Polyharmonic(1) score of the NaN row, 6.876e-16 in the recording, which the test above requires to be NaN
    (the operation that differs is the near-pair block's NaN select, score_kernel.h fix_near; it cannot be restored beside that
    requirement).  That row is held there; every other row of that array keeps the parent's bits like every other array."""
    out, _ = runs
    gold = load("spare_lean_parent_bits")
    assert sorted(gold.files) == sorted(f"{k}_{part}" for k in out for part in "sg")
    assert np.isfinite(gold["mates_nan_poly1_s"][MATE]).all()       # the recorded value that cannot stay
    bad = []
    for k, (s, g) in out.items():
        for part, t in (("s", s), ("g", g)):
            a, ref = t.cpu().numpy(), gold[f"{k}_{part}"]
            if f"{k}_{part}" == "mates_nan_poly1_s":
                keep = np.arange(B) != MATE
                a, ref = a[keep], ref[keep]
            if not np.array_equal(a, ref, equal_nan=True):
                bad.append(f"{k}_{part}")
    assert not bad, bad
