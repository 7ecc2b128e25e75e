"""GPU parity: the HIP path (through the C ABI of libdcx.so) against the CPU oracle, the golden
vectors generated from the reference, and size-independent properties at BASELINE.json's sizes.

Tolerance (BASELINE.json north_star: "within 1e-5 relative fp32"): the metric is
max|a - ref| / max|ref|.  HIP vs the fp64 referee must be <= 1e-5; HIP vs the reference's own fp32
output must be <= 1e-5 plus the reference's own distance from the referee (its torch.cdist GEMM
form is up to ~1e-4 off for large coordinates); HIP vs the fp32 oracle <= 1e-5.
"""

import numpy as np
import pytest
import torch

from helpers import CASE_ROBOT, FK_NAMES, KIND, case_kernel, desc_for, load, make_robot, relerr

pytestmark = pytest.mark.gpu

TOL = 1e-5
TOL_ORACLE = 1e-5  # the fp32 oracle sums S terms sequentially; it is itself ~5e-6 from the referee at S=10k


def _t(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float32, device="cuda")


def _n(t):
    return t.detach().cpu().numpy()


@pytest.fixture(autouse=True, params=["expanded", "direct"])
def fold_pipe(request, knob):
    """every test of this file runs twice: the sweep in its expanded form (score_kernel.h XF, the default; shapes
    without one — every kernel but Polyharmonic(1), rows wider than 37 floats — take the direct form) and in its direct form
    (differences)"""
    knob("xf", 0 if request.param == "direct" else 1)
    yield request.param


@pytest.fixture(scope="module")
def ops():
    from diffco_amd import _lib, _ops
    _lib.require_gpu()  # fails loudly if libdcx.so or the GPU is missing
    return _ops


# ----------------------------------------------------------------------------------- FK
@pytest.mark.parametrize("name", FK_NAMES)
def test_fkine_and_vjp(ops, name):
    from oracle import oracle
    d = load("fk_" + name)
    desc = desc_for(name)
    q = _t(d["q"]).requires_grad_(True)
    X = ops.fkine(desc, q)
    assert X.shape == d["x64"].shape
    assert relerr(_n(X), d["x64"]) < 2e-6
    assert relerr(_n(X), oracle.fkine(desc, d["q"])) < 1e-6
    (gq,) = torch.autograd.grad((X * _t(d["gx"])).sum(), q)
    assert relerr(_n(gq), d["gq64"]) < 5e-6
    # ragged tail and a single configuration
    for n in (1, 63, 65):
        Xs = ops.fkine(desc, _t(d["q"][:n] if n <= 64 else np.concatenate([d["q"], d["q"][:1]])))
        ref = d["x64"][:n] if n <= 64 else np.concatenate([d["x64"], d["x64"][:1]])
        assert relerr(_n(Xs), ref) < 2e-6


def test_robot_classes_known_answers():
    from diffco_amd import model
    z = torch.zeros(1, 7, device="cuda")
    b = model.BaxterLeftArmFK().fkine(z)[0].cpu().numpy()
    np.testing.assert_allclose(b, [[0.069, 0, 0.27035], [0.43335, 0, 0.20135], [0.80764, 0, 0.19135],
                                   [1.19499, 0, 0.19135]], atol=2e-6)
    p = model.PandaFK().fkine(z)[0].cpu().numpy()
    np.testing.assert_allclose(p[4:], [[.088, 0, .819], [.088, -.107, .819], [.088, .107, .819]], atol=2e-6)
    pl = model.RevolutePlanarRobot(1.0, 0.1, dof=2).fkine(torch.tensor([[.5, -1.]]))  # CPU tensor in -> CPU out
    assert pl.device.type == "cpu"
    np.testing.assert_allclose(pl[0].numpy(), [[0.87758255, 0.47942555], [1.7551651, 0.0]], atol=1e-6)


# ----------------------------------------------------------------------------------- kernels
def test_kernel_matrix(ops):
    from oracle import oracle
    d = load("kernels")
    for D in (4, 12, 21, 6):
        x, s = d[f"x_D{D}"], d[f"s_D{D}"]
        for i, (kind, p) in enumerate(zip(d["kernel_kinds"], d["kernel_params"])):
            K = _n(ops.kernel_matrix(KIND[str(kind)], p[0], p[1], _t(x), _t(s)))
            assert relerr(K, d[f"k64_D{D}_{i}"]) < 3e-6, (D, i)
            assert relerr(K, oracle.kernel_matrix(KIND[str(kind)], p[0], p[1], x, s)) < 2e-6, (D, i)
    from diffco_amd import kernel
    a, b = torch.zeros(1, 1), torch.tensor([[1.0], [2.0]])
    np.testing.assert_allclose(kernel.RQKernel(10)(a, b).numpy(), [0.02777778, 0.00226757], rtol=3e-6)
    assert kernel.RQKernel(10)(a, b).shape == (2,)  # one query row is squeezed (kernel.py:26-27)
    np.testing.assert_allclose(kernel.Polyharmonic(1, 1)(a, b).numpy(), [[1, 2]], rtol=1e-6)
    np.testing.assert_allclose(kernel.Polyharmonic(3, 2)(a, b).numpy(), [[0.5, 4]], rtol=1e-6)
    np.testing.assert_allclose(kernel.Polyharmonic(2, 1)(a, b).numpy(), [[0, 2.7725887]], rtol=2e-6, atol=1e-12)


# ----------------------------------------------------------------------------------- fused score + grad
def _model(ops, name, d, sup=None):
    kind, p0, p1 = case_kernel(d)
    desc = desc_for(CASE_ROBOT[name], dof=d["q"].shape[1])
    if sup is None:
        sup = ops.fkine(desc, _t(d["sup_q"])) if name.startswith("edge_r0") else _t(d["sup_x32"])
    return ops.ScoreModel(desc, kind, p0, p1, sup.reshape(len(sup), -1), _t(d["weights"])), desc, (kind, p0, p1)


@pytest.mark.parametrize("name", sorted(CASE_ROBOT))
def test_score_grad_vs_oracle_and_reference(ops, name):
    from oracle import oracle
    d = load(name)
    m, desc, (kind, p0, p1) = _model(ops, name, d)
    q = _t(d["q"])
    B, C = len(q), m.C
    s, g = m.score_grad_raw(q)
    s, g = _n(s), _n(g)
    s64, g64 = d["score64"].reshape(B, C), d["grad64"]
    s32, g32 = d["score32"].reshape(B, C), d["grad32"]
    assert relerr(s, s64) < TOL and relerr(g, g64) < TOL
    assert relerr(s, s32) < TOL + relerr(s32, s64) and relerr(g, g32) < TOL + relerr(g32, g64)
    sup_o = oracle.fkine(desc, d["sup_q"]) if name.startswith("edge_r0") else d["sup_x32"]
    so, go, jo = oracle.score_grad(desc, kind, p0, p1, sup_o, d["weights"], d["q"], want_jac=True)
    assert relerr(s, so) < TOL_ORACLE and relerr(g, go) < TOL_ORACLE
    # score-only entry point == score of the fused pass
    assert relerr(_n(m.score_raw(q)), s) < 3e-6  # a different instantiation may associate the sums differently
    # Jacobian entry point
    sj, jac = m.score_jac_raw(q)
    assert relerr(_n(sj), s) < 3e-6 and relerr(_n(jac), jo) < TOL_ORACLE
    if "upstream" in d.files:
        _, gv = m.score_grad_raw(q, _t(d["upstream"]))
        assert relerr(_n(gv), d["vjp64"]) < TOL
        assert relerr(_n(gv), d["vjp32"]) < TOL + relerr(d["vjp32"], d["vjp64"])
        nj = d["jac32"].shape[0]
        assert relerr(_n(jac)[:nj], d["jac32"]) < TOL + relerr(g32, g64)
    elif C == 1:
        up = torch.linspace(-2, 3, B, device="cuda").reshape(B, 1)
        _, gv = m.score_grad_raw(q, up)
        assert relerr(_n(gv), g * _n(up)) < 1e-6


@pytest.mark.parametrize("name", ["cfg2_baxter_poly1", "cfg3_baxter_rq_c5", "misc_dualpanda_rq"])
def test_support_slicing_is_invariant(ops, name, knob):
    """every launch geometry — waves per block (support slices meeting in LDS) x support super-chunks across
    blocks (split launch + finish kernel) — gives the same answer"""
    d = load(name)
    m, _, _ = _model(ops, name, d)
    q = _t(d["q"][:200])
    up = _t(d["upstream"][:200]) if "upstream" in d.files else None
    outs = []
    for ys in (1, 2, 4, 8):
        for nw in (1, 2, 4, 8, 16):
            knob("nw", nw)
            knob("ys", ys)
            s, g = m.score_grad_raw(q, up)
            s0 = m.score_raw(q)
            _, jac = m.score_jac_raw(q)
            outs.append((_n(s), _n(g), _n(s0), _n(jac)))
    knob("nw", -1)
    knob("ys", -1)
    for o in outs[1:]:
        for a, b in zip(o, outs[0]):
            assert relerr(a, b) < 3e-6


@pytest.mark.parametrize("name", ["cfg2_baxter_poly1", "cfg3_baxter_rq_c5", "cfg2_panda_poly1"])
def test_owner_polls_handover_equals_the_counter_protocol_bitwise(ops, name, knob):
    """round 4: the split launch's hand-over with block y = 0 owning its tile and polling its peers' (value, tag) words
    (score_kernel.h, knob owner_poll = 1) against the arrival-counter protocol (knob 0): the same sums in the same order ->
    bit-identical score, gradient and Jacobian, launch after launch (the owner puts the zeros back), ragged batches"""
    d = load(name)
    kind, p0, p1 = case_kernel(d)
    m = ops.ScoreModel(desc_for(CASE_ROBOT[name]), kind, p0, p1, _t(d["sup_x32"].reshape(len(d["sup_x32"]), -1)), _t(d["weights"]))
    for n in (150, 64, 333):
        q = _t(d["q"][:n])
        up = _t(d["upstream"][:n]) if m.C > 1 and "upstream" in d.files else None
        knob("owner_poll", 0)
        s0, g0 = m.score_grad_raw(q, up)
        j0 = m.score_jac_raw(q)[1]
        knob("owner_poll", 1)
        for _ in range(3):
            s1, g1 = m.score_grad_raw(q, up)
            assert torch.equal(s0, s1) and torch.equal(g0, g1), n
        assert torch.equal(j0, m.score_jac_raw(q)[1])
    knob("owner_poll", -1)


def test_a_launch_that_gave_up_is_reported_by_the_next_one(ops, knob):
    """round 5: an owner block whose peers never publish gives up after seconds, turns its tile into NaN and sets a
    host-visible flag on the model; the model's NEXT launch must fail loudly instead of computing on (knob giveup_inject sets the
    flag the way the kernel would).  Other models are not affected."""
    from diffco_amd._lib import DcxError
    d = load("cfg2_baxter_poly1")
    kind, p0, p1 = case_kernel(d)
    sup, w = _t(d["sup_x32"].reshape(len(d["sup_x32"]), -1)), _t(d["weights"])
    m1 = ops.ScoreModel(desc_for("baxter_left"), kind, p0, p1, sup, w)
    m2 = ops.ScoreModel(desc_for("baxter_left"), kind, p0, p1, sup, w)
    q = _t(d["q"][:300])
    s0, _ = m1.score_grad_raw(q)
    knob("giveup_inject", 1)
    with pytest.raises(DcxError, match="gave up waiting"):
        m1.score_grad_raw(q)
    with pytest.raises(DcxError, match="gave up waiting"):      # sticky: this model's results can no longer be trusted
        m1.score_raw(q)
    s2, _ = m2.score_grad_raw(q)                                  # another model of the same shape is fine
    assert torch.equal(s2, s0)


def test_owner_polls_on_one_stream_counters_on_the_others(ops, knob):
    """round 5: owners of concurrent launches on several streams could together fill every workgroup slot before
    any publisher is dispatched, so the rule gives the owner-polls hand-over to ONE stream per device (the first that asked)
    and the arrival counters to every other; both produce the same bits, launches interleaved over three streams, and the
    words of a launch carry that launch's own tag (a second model on the same streams: its own scratch, its own tags)"""
    d = load("cfg2_baxter_poly1")
    kind, p0, p1 = case_kernel(d)
    sup, w = _t(d["sup_x32"].reshape(len(d["sup_x32"]), -1)), _t(d["weights"])
    m1 = ops.ScoreModel(desc_for("baxter_left"), kind, p0, p1, sup, w)
    m2 = ops.ScoreModel(desc_for("baxter_left"), kind, p0, p1, sup, 2.0 * w)
    q = _t(d["q"][:700])
    knob("qt", 0)   # the split launch, not the 16-configuration tile
    s0, g0 = m1.score_grad_raw(q)
    s0, g0 = s0.clone(), g0.clone()
    streams = [torch.cuda.current_stream(), torch.cuda.Stream(), torch.cuda.Stream()]
    outs = []
    for it in range(60):
        with torch.cuda.stream(streams[it % 3]):
            outs.append((1.0, m1.score_grad_raw(q)))
            outs.append((2.0, m2.score_grad_raw(q)))
    torch.cuda.synchronize()
    for f, (s, g) in outs:
        assert torch.equal(s, f * s0) and torch.equal(g, f * g0)


@pytest.mark.parametrize("name", ["cfg2_baxter_poly1", "cfg3_baxter_rq_c5"])
def test_split_launch_finish_modes_agree_bitwise(ops, name, knob):
    """small batches split the supports across blocks; the rows are added either by the last block to arrive
    (in-launch, arrival counters) or by a second launch — same fixed order, so the results are bit-identical, and the
    counters are back at zero after every launch (three launches in a row)"""
    d = load(name)
    kind, p0, p1 = case_kernel(d)
    m = ops.ScoreModel(desc_for(CASE_ROBOT[name]), kind, p0, p1, _t(d["sup_x32"].reshape(len(d["sup_x32"]), -1)), _t(d["weights"]))
    q = _t(d["q"][:150])
    up = _t(d["upstream"][:150]) if m.C > 1 and "upstream" in d.files else None
    knob("split_finish_kernel", -1)
    runs = [m.score_grad_raw(q, up) for _ in range(3)]
    knob("split_finish_kernel", 1)
    s2, g2 = m.score_grad_raw(q, up)
    for s1, g1 in runs:
        assert torch.equal(s1, s2) and torch.equal(g1, g2)
    knob("split_finish_kernel", -1)
    knob("ys", 1)  # and the unsplit launch agrees to rounding
    s3, g3 = m.score_grad_raw(q, up)
    assert relerr(_n(s3), _n(s2)) < 3e-6 and relerr(_n(g3), _n(g2)) < 3e-6


@pytest.mark.parametrize("D,C", [(12, 1), (12, 3), (7, 1), (21, 1), (6, 2)])
def test_expanded_form_around_the_near_threshold(ops, knob, D, C):
    """the expanded sweep's near-pair machinery under load: every query sits at a chosen relative distance
    r / |x| in [1e-7, 1] from one support (the threshold is r / |x| = 0.1), many per wave, on both sides of it, plus exact
    coincidences — score and gradient against the float64 oracle at the 1e-5 bar, in the expanded AND the direct form, and
    a configuration's result must not depend on its wave-mates (shuffled batch, bit for bit)."""
    from diffco_amd import _fkdesc
    from oracle import oracle
    g = torch.Generator().manual_seed(100 * D + C)
    S, B = 300, 4096
    sup = (torch.rand((S, D), generator=g) * 2 - 1) * 1.5
    W = torch.randn((S, C), generator=g)
    j = torch.randint(0, S, (B,), generator=g)
    u = torch.randn((B, D), generator=g)
    u = u / u.norm(dim=1, keepdim=True)
    rel = 10.0 ** (torch.rand((B, 1), generator=g) * 7 - 7)            # 1e-7 .. 1
    rel[::97] = 0.0                                                     # exact coincidences
    rel[1::53] = 0.1 * (1 + (torch.rand((len(rel[1::53]), 1), generator=g) - 0.5) * 1e-3)   # on the threshold
    q = sup[j] + rel * sup[j].norm(dim=1, keepdim=True) * u
    desc = _fkdesc.none_desc(D)
    m = ops.ScoreModel(desc, 1, 1.0, 1.0, sup.cuda(), W.cuda())
    up = torch.randn((B, C), generator=g).cuda() if C > 1 else None
    so, go, _ = oracle.score_grad(desc, 1, 1.0, 1.0, sup.numpy().astype(np.float64), W.numpy().astype(np.float64),
                                  q.numpy().astype(np.float64), upstream=None if up is None else _n(up).astype(np.float64),
                                  dtype=np.float64)
    res = {}
    for form in (1, 0):
        knob("xf", form)
        s, gr = m.score_grad_raw(q.cuda(), up)
        assert torch.isfinite(s).all() and torch.isfinite(gr).all()
        assert relerr(_n(s), so) < TOL and relerr(_n(gr), go) < TOL, (form, relerr(_n(s), so), relerr(_n(gr), go))
        perm = torch.randperm(B, generator=g).cuda()
        sp, gp = m.score_grad_raw(q.cuda()[perm].contiguous(), None if up is None else up[perm].contiguous())
        assert torch.equal(sp, s[perm]) and torch.equal(gp, gr[perm]), form
        res[form] = (s, gr)
    assert relerr(_n(res[1][0]), _n(res[0][0])) < 6e-6 and relerr(_n(res[1][1]), _n(res[0][1])) < 6e-6


@pytest.mark.parametrize("name", ["cfg3_baxter_rq_c5", "cfg3_baxter_poly1_c5", "misc_baxterR_mq_c2"])
@pytest.mark.parametrize("nw", [16, 4, 1])
def test_one_sweep_jacobian_equals_one_sweep_per_class(ops, name, nw, knob):
    """jac_kernel.h (all classes of a pair in one sweep, C x D accumulators per lane, the C J^T products side by side)
    against the one-hot sweeps of score_kernel in its direct form with the same slicing: same arithmetic per
    (configuration, class), same fold order -> identical bits; ragged last tile, one tile, many tiles"""
    d = load(name)
    m, _, _ = _model(ops, name, d)
    reps = -(-700 // len(d["q"]))
    q = _t(np.tile(d["q"], (reps, 1))[:700])
    q = q + 0.01 * torch.arange(len(q), device="cuda", dtype=torch.float32)[:, None] / len(q)
    knob("nw", nw)
    knob("ys", 1)
    knob("min_rows", 1)
    knob("xf", 0)
    for B in (700, 64, 5):
        knob("jac_one_sweep", 0)
        knob("jac_per_class", 1)
        s1, j1 = m.score_jac_raw(q[:B])
        knob("jac_per_class", -1)
        knob("jac_one_sweep", 1)
        s2, j2 = m.score_jac_raw(q[:B])
        assert j2.shape == (B, m.C, q.shape[1])
        assert torch.equal(s1, s2) and torch.equal(j1, j2), (B, float((j1 - j2).abs().max()))
    # and against the float64 oracle's Jacobian
    from oracle import oracle
    kind, p0, p1 = case_kernel(d)
    desc = desc_for(CASE_ROBOT[name], dof=d["q"].shape[1])
    _, _, jo = oracle.score_grad(desc, kind, p0, p1, d["sup_x32"].reshape(len(d["sup_x32"]), -1).astype(np.float64),
                                 d["weights"].astype(np.float64), _n(q[:64]).astype(np.float64), want_jac=True, dtype=np.float64)
    s2, j2 = m.score_jac_raw(q[:64])
    assert relerr(_n(j2), jo) < TOL


@pytest.mark.parametrize("ys", [1, 4])
def test_jacobian_rows_in_one_launch_equal_one_launch_per_class(ops, ys, knob):
    """C > 1: `dcx_score_jac` sends the C one-hot sweeps of a small batch out as ONE launch (grid z = class); with the
    geometry pinned it is bit-identical to one launch per class, also when the split launch has no arrival counters
    (then the per-class route is taken) and three times in a row (counters of every (tile, class) back at zero)"""
    d = load("cfg3_baxter_rq_c5")
    m, _, _ = _model(ops, "cfg3_baxter_rq_c5", d)
    q = _t(d["q"][:333])
    knob("nw", 8)
    knob("ys", ys)
    knob("min_rows", 1)
    runs = [m.score_jac_raw(q) for _ in range(3)]
    knob("jac_per_class", 1)
    s2, j2 = m.score_jac_raw(q)
    knob("jac_per_class", -1)
    knob("split_finish_kernel", 1)
    s3, j3 = m.score_jac_raw(q)
    for s1, j1 in runs:
        assert torch.equal(s1, s2) and torch.equal(j1, j2)
    assert torch.equal(s3, s2) and torch.equal(j3, j2)
    assert float(j2.abs().max()) > 0


def test_split_launch_protocol_stress(ops, knob):
    """the cross-block hand-over of a split launch (write-through partial rows, release fence, arrival counter, acquire
    fence, re-read) under load: 300 back-to-back launches at batch sizes that exercise every split geometry (ys = 8, 4,
    2 and the thirds split), alternating between two streams on one model, each result bit-identical to the
    second-launch finish of the same inputs — a stale or torn row would show up as a mismatch"""
    g = torch.Generator().manual_seed(11)
    desc = desc_for("baxter_left")
    S = 2000
    sup = torch.randn((S, 12), generator=g).cuda()
    w = torch.randn((S, 1), generator=g).cuda()
    m = ops.ScoreModel(desc, 1, 1.0, 1.0, sup, w)  # Polyharmonic(1, 1)
    sizes = [64, 1000, 2048, 4096, 8192, 9216, 10240]
    qs = {n: ((torch.rand((n, 7), generator=g) - 0.5) * 4).cuda() for n in sizes}
    knob("split_finish_kernel", 1)
    want = {n: m.score_grad_raw(qs[n]) for n in sizes}
    torch.cuda.synchronize()
    knob("split_finish_kernel", -1)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    got = []
    for it in range(300):
        n = sizes[it % len(sizes)]
        with torch.cuda.stream(streams[it % 2]):
            got.append((n, m.score_grad_raw(qs[n])))
    torch.cuda.synchronize()
    for n, (s1, g1) in got:
        assert torch.equal(s1, want[n][0]) and torch.equal(g1, want[n][1]), n


def test_ragged_empty_and_padding(ops, knob):
    knob("nw", 4)  # fixed slicing: results are then bit-identical across batch sizes
    d = load("cfg2_baxter_poly1")
    m, desc, (kind, p0, p1) = _model(ops, "cfg2_baxter_poly1", d)
    q = _t(d["q"])
    s_full, g_full = m.score_grad_raw(q[:300])
    for n in (1, 2, 63, 64, 65, 127, 257):
        s, g = m.score_grad_raw(q[:n].contiguous())
        assert torch.equal(s, s_full[:n]) and torch.equal(g, g_full[:n]), n  # batch-independent, bit-exact
    s0, g0 = m.score_grad_raw(q[:0])
    assert s0.shape == (0, 1) and g0.shape == (0, 7)
    # zero-weight rows (max_num_supports padding, kernel_perceptrons.py:159-196) change nothing ...
    sup = _t(d["sup_x32"]).reshape(1000, -1)
    w = _t(d["weights"])
    mp = ops.ScoreModel(desc, kind, p0, p1, torch.cat([sup, torch.zeros(24, 12, device="cuda")]),
                        torch.cat([w, torch.zeros(24, 1, device="cuda")]))
    sp, gp = mp.score_grad_raw(q[:300])
    assert torch.equal(sp, s_full) and torch.equal(gp, g_full)
    # ... and a model with no active support scores zero
    me = ops.ScoreModel(desc, kind, p0, p1, sup[:5], torch.zeros(5, 1))
    se, ge = me.score_grad_raw(q[:70])
    assert float(se.abs().max()) == 0.0 and float(ge.abs().max()) == 0.0
    # ... with zero second derivatives (this call used to divide by a zero slice size)
    gh, he = me.score_hess_raw(q[:70].contiguous())
    assert he.shape == (70, 7, 7) and float(he.abs().max()) == 0.0 and float(gh.abs().max()) == 0.0


@pytest.mark.parametrize("D", [2, 4, 6, 8])
@pytest.mark.parametrize("kspec", [(0, 10.0, 2.0), (1, 1.0, 1.0)])
def test_two_rows_per_packed_instruction_every_tail(ops, knob, D, kspec):
    """round 5 (score_kernel.h pair2): narrow one-class rows in the direct form take the two rows of a pipeline stage in the two
    halves of every packed register, fetched by one load.  Raw D-dimensional inputs (no transform), both compiled kernel
    functions, support counts and block sizes that leave every tail of a slice (0 .. 3 rows behind the last whole stage, slices
    of a single row, a slice ending on the model's last row): score, gradient with the row weight and with an explicit upstream
    against the float64 oracle, and the score-only launch; 2 D = 3, 5, 7 features run padded to the compiled width"""
    from diffco_amd import _fkdesc
    from oracle import oracle
    knob("xf", 0)      # the direct form whatever the data would allow
    g = torch.Generator().manual_seed(100 * D + kspec[0])
    for Du in ((D,) if D == 2 else (D - 1, D)):
        desc = _fkdesc.none_desc(Du)
        for S in (1, 2, 3, 5, 7, 31, 64, 257, 1001):
            sup = torch.randn((S, Du), generator=g) * 2.0
            W = torch.randn((S, 1), generator=g)
            q = (torch.randn((200, Du), generator=g) * 2.0).cuda()
            q[3] = sup[S // 2].cuda()                      # r = 0 on one pair
            m = ops.ScoreModel(desc, *kspec, sup.cuda(), W.cuda())
            so, go, _ = oracle.score_grad(desc, *kspec, sup.numpy().astype(np.float64), W.numpy().astype(np.float64),
                                          _n(q).astype(np.float64), dtype=np.float64)
            up = torch.randn((200, 1), generator=g).cuda()
            for nw in (1, 4, 16):
                knob("nw", nw)
                s, gr = m.score_grad_raw(q)
                s0 = m.score_raw(q)
                su, gu = m.score_grad_raw(q, up)
                tag = (Du, S, nw)
                assert relerr(_n(s), so) < TOL and relerr(_n(gr), go) < TOL, tag
                assert relerr(_n(s0), so) < TOL and torch.equal(su, s), tag
                assert relerr(_n(gu), go * _n(up).astype(np.float64)) < TOL, tag
    knob("nw", -1)
    knob("xf", -1)


@pytest.mark.parametrize("C", [1, 2, 3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("rob_name,kspec", [("baxter_left", (0, 10.0, 2.0)), ("baxter_left", (1, 1.0, 1.0)), ("planar3", (2, 0.8, 0.0))])
def test_every_class_count(ops, C, rob_name, kspec, knob):
    """C = 1 .. 8 (DCX_MAX_C): the sweeps are compiled for 1, 2, 4, 5 and 8 classes - 3 runs as 4, 6 and 7 as 8 with zero
    weight columns that are neither read from `upstream` nor written to `score` / `jac` (dcx_internal.h compiled_classes).
    Score, vjp with a random upstream, the full Jacobian and the Hessian against the float64 oracle, small (split) and
    larger batches; the output buffers are exactly [B, C] wide (a guard band behind them stays untouched)"""
    from oracle import oracle
    rob, desc, sup, W, g = _rand_setup(ops, rob_name, 500, C, kspec, seed=C)
    m = ops.ScoreModel(desc, *kspec, sup, W)
    for B in (70, 3000):
        q = _rand_q(rob, B, g)
        up = torch.randn((B, C), generator=g).cuda()
        so, go, jo = oracle.score_grad(desc, *kspec, _n(sup).astype(np.float64), _n(W).astype(np.float64), _n(q).astype(np.float64),
                                       upstream=_n(up).astype(np.float64), want_jac=True, dtype=np.float64)
        s, gr = m.score_grad_raw(q, up)
        assert s.shape == (B, C) and relerr(_n(s), so) < TOL and relerr(_n(gr), go) < TOL
        s1, g1 = m.score_grad_raw(q)                         # upstream = ones: the row-sum weight column
        assert relerr(_n(g1), jo.sum(axis=1)) < TOL and torch.equal(s1, s)
        for one_sweep in (0, 1):
            knob("jac_one_sweep", one_sweep)
            sj, jac = m.score_jac_raw(q)
            assert jac.shape == (B, C, rob.dof) and relerr(_n(jac), jo) < TOL and relerr(_n(sj), so) < TOL
        knob("jac_one_sweep", -1)
        assert relerr(_n(m.score_raw(q)), so) < TOL
    # guard band: a [B, C] score buffer carved out of a larger one
    B = 130
    q = _rand_q(rob, B, g)
    big = torch.full((B * C + 64,), 7.0, device="cuda")
    out = big[:B * C].view(B, C)
    grad = torch.empty((B, rob.dof), device="cuda")
    import ctypes as Ct
    from diffco_amd import _lib
    _lib.check(m._lib.dcx_score_grad(m._h, Ct.c_void_p(q.data_ptr()), B, None, Ct.c_void_p(out.data_ptr()), Ct.c_void_p(grad.data_ptr()),
                                     Ct.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert float(big[B * C:].min()) == 7.0 and float(big[B * C:].max()) == 7.0
    assert relerr(_n(out), _n(m.score_raw(q))) < 3e-6       # (the score-only launch may take another form of the sweep)
    if rob_name == "baxter_left" and kspec[0] == 0:
        q40, up40 = q[:40].contiguous(), torch.randn((40, C), generator=g).cuda()
        gh, hs = m.score_hess_raw(q40, up40)                 # the second-derivative kernel reads the same rows and upstream
        _, g40 = m.score_grad_raw(q40, up40)
        assert hs.shape == (40, rob.dof, rob.dof) and torch.isfinite(hs).all() and relerr(_n(gh), _n(g40)) < 1e-5


def test_errors_are_loud(ops):
    from diffco_amd._lib import DcxError
    d = load("cfg2_baxter_poly1")
    desc = desc_for("baxter_left")
    sup, w = _t(d["sup_x32"]).reshape(1000, -1), _t(d["weights"])
    with pytest.raises(DcxError):
        ops.ScoreModel(desc, 7, 1.0, 1.0, sup, w)  # unknown kernel kind
    with pytest.raises(DcxError):
        ops.ScoreModel(desc, 1, 1.5, 1.0, sup, w)  # non-integer polyharmonic order
    with pytest.raises((DcxError, ValueError)):
        ops.ScoreModel(desc, 1, 1.0, 1.0, sup[:, :9], w)  # feature width mismatch
    with pytest.raises(DcxError):
        ops.ScoreModel(desc, 1, 1.0, 1.0, sup, torch.zeros(1000, 9))  # C > DCX_MAX_C


# ----------------------------------------------------------------------------------- BASELINE sizes: properties
def _rand_setup(ops, rob_name, S, C, kind_spec, seed=0):
    g = torch.Generator().manual_seed(seed)
    rob = make_robot(rob_name)
    lim = rob.limits
    sup_q = torch.rand((S, lim.shape[0]), generator=g) * (lim[:, 1] - lim[:, 0]) + lim[:, 0]
    W = torch.randn((S, C), generator=g)
    desc = rob.fk_desc()
    sup = ops.fkine(desc, sup_q.cuda()).reshape(S, -1)
    return rob, desc, sup, W.cuda(), g


def _rand_q(rob, B, g):
    lim = rob.limits
    return (torch.rand((B, lim.shape[0]), generator=g) * (lim[:, 1] - lim[:, 0]) + lim[:, 0]).cuda()


@pytest.mark.parametrize("B,S,C,kspec", [(65536, 2000, 1, (1, 1.0, 1.0)), (65536, 2000, 5, (0, 10.0, 2.0)),
                                          (4096, 1000, 1, (0, 10.0, 2.0))])
def test_full_size_properties(ops, B, S, C, kspec, knob, fold_pipe):
    """headline / config #2 / config #3 sizes: linearity in the weights, additivity over a support
    split, invariance to batch order, and an fp64 spot check of 64 random rows."""
    from oracle import oracle
    # (round 5, VERDICT r4 item 8: everything but the last block runs at the DEFAULT launch geometry - the 16-wave blocks the
    # bench's headline actually runs, the 8-wave blocks of a five-class model, the split launch of the 4096 batch)
    rob, desc, sup, W, g = _rand_setup(ops, "baxter_left", S, C, kspec)
    q = _rand_q(rob, B, g)
    m = ops.ScoreModel(desc, *kspec, sup, W)
    s, gr = m.score_grad_raw(q)
    scale_s, scale_g = float(s.abs().max()), float(gr.abs().max())
    # additivity over a support split
    h = S // 3
    s1, g1 = ops.ScoreModel(desc, *kspec, sup[:h], W[:h]).score_grad_raw(q)
    s2, g2 = ops.ScoreModel(desc, *kspec, sup[h:], W[h:]).score_grad_raw(q)
    # (RQ in the expanded form, round 4: each of the three models is centred on its own supports and carries the form's
    # ~2e-6 against float64 - the last assertion of this test - so the residual of three evaluations is a few of those)
    tol_add = 8e-6 if (kspec[0] == 0 and fold_pipe != "direct") else 3e-6
    assert float((s1 + s2 - s).abs().max()) < tol_add * scale_s
    assert float((g1 + g2 - gr).abs().max()) < tol_add * scale_g
    # linearity in the weights: a power-of-two scale is exact in fp32, so the results are bit-identical
    s3, g3 = ops.ScoreModel(desc, *kspec, sup, -4.0 * W).score_grad_raw(q)
    assert torch.equal(s3, -4.0 * s) and torch.equal(g3, -4.0 * gr)
    s4, g4 = ops.ScoreModel(desc, *kspec, sup, -2.5 * W).score_grad_raw(q)
    assert float((s4 + 2.5 * s).abs().max()) < 2e-5 * scale_s and float((g4 + 2.5 * gr).abs().max()) < 2e-5 * scale_g  # -2.5*w rounds
    # batch order does not matter (each configuration is independent): bit-exact
    perm = torch.randperm(B, generator=g).cuda()
    sp, gp = m.score_grad_raw(q[perm].contiguous())
    assert torch.equal(sp, s[perm]) and torch.equal(gp, gr[perm])
    # fp64 referee on a random subset of rows
    idx = torch.randint(0, B, (64,), generator=g)
    so, go, _ = oracle.score_grad(desc, *kspec, _n(sup).astype(np.float64), _n(W), _n(q[idx.cuda()]), dtype=np.float64)
    assert relerr(_n(s[idx.cuda()]), so) < TOL and relerr(_n(gr[idx.cuda()]), go) < TOL
    # another block size (4 waves: other support slices, another fold tree): the same properties, and the same numbers up to
    # the reassociation of the sums
    knob("nw", 4)
    s4w, g4w = m.score_grad_raw(q)
    assert float((s4w - s).abs().max()) < 3e-6 * scale_s and float((g4w - gr).abs().max()) < 3e-6 * scale_g
    sp, gp = m.score_grad_raw(q[perm].contiguous())
    assert torch.equal(sp, s4w[perm]) and torch.equal(gp, g4w[perm])
    assert relerr(_n(s4w[idx.cuda()]), so) < TOL and relerr(_n(g4w[idx.cuda()]), go) < TOL


def test_config4_se3_streaming(ops):
    """config #4 at BASELINE size: 1 M SE(3) configurations, RQ(10), 10k supports, no FK (D = 6)"""
    from diffco_amd import _fkdesc
    from oracle import oracle
    g = torch.Generator().manual_seed(4)
    lo = torch.tensor([-10.0] * 3 + [-np.pi] * 3)
    S, B = 10000, 1 << 20
    sup = (torch.rand((S, 6), generator=g) * (-2 * lo) + lo).cuda()
    q = (torch.rand((B, 6), generator=g) * (-2 * lo) + lo).cuda()
    W = torch.randn((S, 1), generator=g).cuda()
    desc = _fkdesc.none_desc(6)
    m = ops.ScoreModel(desc, 0, 10.0, 2.0, sup, W)
    s, gr = m.score_grad_raw(q)
    idx = torch.randint(0, B, (64,), generator=g).cuda()
    so, go, _ = oracle.score_grad(desc, 0, 10.0, 2.0, _n(sup).astype(np.float64), _n(W), _n(q[idx]), dtype=np.float64)
    assert relerr(_n(s[idx]), so) < TOL and relerr(_n(gr[idx]), go) < TOL
    half = ops.ScoreModel(desc, 0, 10.0, 2.0, sup[:5000], W[:5000]).score_grad_raw(q)
    rest = ops.ScoreModel(desc, 0, 10.0, 2.0, sup[5000:], W[5000:]).score_grad_raw(q)
    assert float((half[0] + rest[0] - s).abs().max()) < 5e-6 * float(s.abs().max())
    assert float((half[1] + rest[1] - gr).abs().max()) < 5e-6 * float(gr.abs().max())  # max over 1 M rows of a reassociated sum


@pytest.mark.parametrize("B", [200, 5000])
def test_hip_graph_capture_and_replay(ops, B):
    """the launches carry no allocation and no synchronisation, so a caller can capture them into a HIP graph: small
    batch (split launch, finished inside the launch with per-tile arrival counters that must be back at zero after
    every replay) and a larger one (plain launch); replays reproduce the eager result bit for bit"""
    d = load("cfg2_baxter_poly1")
    kind, p0, p1 = case_kernel(d)
    m = ops.ScoreModel(desc_for("baxter_left"), kind, p0, p1, _t(d["sup_x32"].reshape(len(d["sup_x32"]), -1)), _t(d["weights"]))
    rng = np.random.default_rng(3)
    q = _t(np.tile(d["q"], (B // len(d["q"]) + 1, 1))[:B] + rng.normal(0, 0.05, (B, d["q"].shape[1])).astype(np.float32))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        s0, g0 = m.score_grad_raw(q)          # warm-up on the capture stream: its scratch buffer now exists
        torch.cuda.current_stream().synchronize()
        s = torch.empty_like(s0)
        g = torch.empty_like(g0)
        import ctypes as C
        from diffco_amd import _lib
        lib = _lib.load()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=side):
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            _lib.check(lib.dcx_score_grad(m._h, C.c_void_p(q.data_ptr()), B, None, C.c_void_p(s.data_ptr()),
                                          C.c_void_p(g.data_ptr()), st))
    for _ in range(3):
        s.zero_()
        g.zero_()
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(s, s0) and torch.equal(g, g0)


def test_concurrent_streams_share_a_model(ops):
    """a model handle is immutable: launches on different streams may overlap (each stream gets its own scratch for
    split launches); interleaved small and large batches on three streams reproduce the serial results"""
    d = load("cfg2_baxter_poly1")
    kind, p0, p1 = case_kernel(d)
    m = ops.ScoreModel(desc_for("baxter_left"), kind, p0, p1, _t(d["sup_x32"].reshape(len(d["sup_x32"]), -1)), _t(d["weights"]))
    rng = np.random.default_rng(5)
    qs = [_t(rng.uniform(-1.5, 1.5, (n, 7)).astype(np.float32)) for n in (130, 700, 9000)]
    want = [m.score_grad_raw(q) for q in qs]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in qs]
    got = [[] for _ in qs]
    for rep in range(6):
        for i, (st, q) in enumerate(zip(streams, qs)):
            with torch.cuda.stream(st):
                got[i].append(m.score_grad_raw(q))
    torch.cuda.synchronize()
    for i, (s0, g0) in enumerate(want):
        for s, g in got[i]:
            assert torch.equal(s, s0) and torch.equal(g, g0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["baxter_left", "panda", "panda5", "baxter_dual", "dual_panda"])
@pytest.mark.parametrize("B", [1, 200, 4096, 20000])
def test_dh_fk_walks_agree_bitwise(ops, knob, name, B):
    """DH arms have three FK walks: the step table (fk_device.h dh2_*, knob fkk = 2, the default), the FkProg read with
    scalar loads (fk_forward_chain_dh_k / fk_vjp_dh_k, fkk = 1) and the FkProg interpreted from its LDS copy (fkk = 0, what
    every other transform kind uses): the same arithmetic, so score, gradient and the one-sweep Jacobian must agree bit
    for bit — for one and two chains, frames with no / one / three control points (Panda's fingers become identity steps
    of the table), unsplit and split launches"""
    rob = make_robot(name)
    g = torch.Generator().manual_seed(len(name) * 1000 + B)
    lim = rob.limits.float()
    S, C = 300, 5
    rnd = lambda n: torch.rand((n, rob.dof), generator=g) * (lim[:, 1] - lim[:, 0]) + lim[:, 0]
    sup = rob.fkine(rnd(S).cuda()).reshape(S, -1)
    q = rnd(B).cuda()
    out = {}
    for fkk in (2, 1, 0):
        knob("fkk", fkk)
        m1 = ops.ScoreModel(rob.fk_desc(), 1, 1.0, 1.0, sup, torch.randn((S, 1), generator=torch.Generator().manual_seed(3)).cuda())
        mc = ops.ScoreModel(rob.fk_desc(), 0, 10.0, 2.0, sup, torch.randn((S, C), generator=torch.Generator().manual_seed(4)).cuda())
        s1, g1 = m1.score_grad_raw(q)
        up = torch.randn((B, C), generator=torch.Generator().manual_seed(5)).cuda()
        sc, gc = mc.score_grad_raw(q, up)
        sj, jj = mc.score_jac_raw(q)
        out[fkk] = [_n(t).copy() for t in (s1, g1, sc, gc, sj, jj)]
    knob("fkk", -1)
    for other in (2, 1):
        for a, b in zip(out[other], out[0]):
            assert np.isfinite(a).all() and np.array_equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["long14", "long16_pts", "two_chains_12_5", "short3"])
@pytest.mark.parametrize("B", [3, 300, 5000])
def test_dh_step_table_beyond_the_unrolled_walks(ops, knob, shape, B):
    """synthetic DH arms outside the shapes the unrolled multi-wave walks cover (fk_device.h kDhUnroll = 10 steps per chain):
    14 and 16 joints in one chain, up to three control points on a frame (identity steps), a 12 + 5 pair of chains sharing
    no joint, and a 3-joint arm - the step table's single-wave walks take over; all three FK walks must still agree bit for
    bit, and match the float64 oracle"""
    from diffco_amd import _fkdesc
    from oracle import oracle
    rng = np.random.default_rng({"long14": 1, "long16_pts": 2, "two_chains_12_5": 3, "short3": 4}[shape])

    def chain(n, q0, base=None):
        c = dict(a=rng.uniform(-0.3, 0.3, n), d=rng.uniform(-0.3, 0.3, n), alpha=rng.choice([0.0, np.pi / 2, -np.pi / 2, 0.3], n),
                 theta0=rng.uniform(-0.5, 0.5, n), joint_q=list(range(q0, q0 + n)))
        if base is not None:
            c["base"] = base
        return c
    if shape == "long14":
        dof, chains = 14, [chain(14, 0)]
        pts = [(0, f, (0, 0, 0)) for f in (1, 3, 5, 8, 11, 13)]
    elif shape == "long16_pts":
        dof, chains = 16, [chain(16, 0)]
        pts = [(0, 2, (0, 0, 0)), (0, 2, (0.1, 0, 0.05)), (0, 2, (0, -0.1, 0)), (0, 9, (0, 0, 0)), (0, 15, (0.05, 0.05, 0)), (0, 15, (0, 0, 0))]
    elif shape == "two_chains_12_5":
        dof, chains = 17, [chain(12, 0), chain(5, 12, _fkdesc.rotz_base(0.7, (0.2, -0.4, 0.1)))]
        pts = [(0, f, (0, 0, 0)) for f in (2, 6, 11)] + [(1, f, (0, 0, 0)) for f in (1, 4)]
    else:
        dof, chains = 3, [chain(3, 0)]
        pts = [(0, 0, (0, 0, 0)), (0, 2, (0, 0, 0))]
    desc = _fkdesc.dh_desc(dof, chains, pts)
    S, C = 200, 2
    sq = rng.uniform(-2.0, 2.0, (S, dof)).astype(np.float32)
    q = _t(rng.uniform(-2.0, 2.0, (B, dof)).astype(np.float32))
    sup = ops.fkine(desc, _t(sq)).reshape(S, -1)
    W1 = rng.standard_normal((S, 1)).astype(np.float32)
    WC = rng.standard_normal((S, C)).astype(np.float32)
    up = _t(rng.standard_normal((B, C)).astype(np.float32))
    out = {}
    for fkk in (2, 1, 0):
        knob("fkk", fkk)
        m1 = ops.ScoreModel(desc, 1, 1.0, 1.0, sup, _t(W1))
        mc = ops.ScoreModel(desc, 0, 10.0, 2.0, sup, _t(WC))
        s1, g1 = m1.score_grad_raw(q)
        sc, gc = mc.score_grad_raw(q, up)
        out[fkk] = [_n(t).copy() for t in (s1, g1, sc, gc)]
    knob("fkk", -1)
    for other in (2, 1):
        for a, b in zip(out[other], out[0]):
            assert np.isfinite(a).all() and np.array_equal(a, b), (shape, other)
    n64 = min(B, 256)
    so, go, _ = oracle.score_grad(desc, 1, 1.0, 1.0, _n(sup).astype(np.float64), W1.astype(np.float64), _n(q[:n64]).astype(np.float64),
                                  dtype=np.float64)
    assert relerr(out[2][0][:n64], so) < TOL and relerr(out[2][1][:n64], go) < TOL


def _baxter_at(base_xyz):
    """the Baxter arm's description with its base translated (the reference's DualArm bases do the same, model.py:312-363)"""
    from diffco_amd import _fkdesc, model
    rob = model.BaxterLeftArmFK()
    base = list(_fkdesc.IDENTITY_BASE)
    base[3], base[7], base[11] = (float(v) for v in base_xyz)
    desc = _fkdesc.dh_desc(7, [rob.dhparams.chain(range(7), base)], [(0, i, (0, 0, 0)) for i, m in enumerate(rob.fk_mask) if m])
    return rob, desc


@pytest.mark.gpu
@pytest.mark.parametrize("where", [(0.0, 0.0, 0.0), (20.0, 0.0, 0.0), (100.0, 50.0, 0.0)])
def test_expanded_form_far_from_the_origin_baxter(ops, knob, where):
    """the kernels depend on x - s only (kernel.py:73-79), so moving the whole scene must change
    nothing but the last bits.  A Baxter arm based at (20, 0, 0) and at (100, 50, 0) — where the uncentred expanded
    form saw every pair as a "near" pair — against the float64 oracle at the 1e-5 bar, in both sweep forms; the
    expanded and direct forms agree to 6e-6 wherever the arm stands."""
    from oracle import oracle
    rob, desc = _baxter_at(where)
    g = torch.Generator().manual_seed(7)
    lim = rob.limits.float()
    S, B = 1500, 4096
    rnd = lambda n: torch.rand((n, 7), generator=g) * (lim[:, 1] - lim[:, 0]) + lim[:, 0]
    sup_q, q = rnd(S), rnd(B)
    sup = ops.fkine(desc, sup_q.cuda()).reshape(S, -1)
    W = torch.randn((S, 1), generator=g)
    m = ops.ScoreModel(desc, 1, 1.0, 1.0, sup, W.cuda())
    so, go, _ = oracle.score_grad(desc, 1, 1.0, 1.0, _n(sup).astype(np.float64), W.numpy().astype(np.float64),
                                  q.numpy().astype(np.float64), dtype=np.float64)
    res = {}
    for form in (1, 0):
        knob("xf", form)
        s, gr = m.score_grad_raw(q.cuda())
        assert torch.isfinite(s).all() and torch.isfinite(gr).all()
        res[form] = (s, gr, relerr(_n(s), so), relerr(_n(gr), go))
    # fp32 forward kinematics itself carries ~ulp(|x|) per coordinate: at |x| ~ 100 that is 8e-6 of a unit distance, the
    # same for either sweep form (and for the reference's fp32 torch FK); the bar scales with it beyond the origin
    bar = TOL * max(1.0, float(np.linalg.norm(where)) / 25.0)
    for form in (1, 0):
        assert res[form][2] < bar and res[form][3] < bar, (where, form, res[form][2:])
    assert res[1][2] < 1.5 * res[0][2] + 1e-6 and res[1][3] < 1.5 * res[0][3] + 1e-6, (where, res[1][2:], res[0][2:])
    assert relerr(_n(res[1][0]), _n(res[0][0])) < 6e-6 and relerr(_n(res[1][1]), _n(res[0][1])) < 6e-6


@pytest.mark.gpu
@pytest.mark.parametrize("spread", [1.0, 10.0])
def test_expanded_form_se3_bodies_across_the_workspace(ops, knob, spread):
    """SE(3) bodies with 8 keypoints (D = 24) at xyz ~ U(-spread, spread), Polyharmonic(1): both forms against the float64
    oracle (the reference samples rigid bodies in [-10, 10]^3, model.py:146-147)"""
    from diffco_amd import _fkdesc
    from oracle import oracle
    g = torch.Generator().manual_seed(11)
    kp = (torch.rand((8, 3), generator=g) - 0.5) * 0.6
    desc = _fkdesc.keypoint_desc(kp.numpy(), 3)
    S, B = 2000, 2048
    lo = torch.tensor([-spread] * 3 + [-np.pi] * 3)
    rnd = lambda n: torch.rand((n, 6), generator=g) * (-2 * lo) + lo
    sup_q, q = rnd(S), rnd(B)
    sup = ops.fkine(desc, sup_q.cuda()).reshape(S, -1)
    W = torch.randn((S, 1), generator=g)
    m = ops.ScoreModel(desc, 1, 1.0, 1.0, sup, W.cuda())
    so, go, _ = oracle.score_grad(desc, 1, 1.0, 1.0, _n(sup).astype(np.float64), W.numpy().astype(np.float64),
                                  q.numpy().astype(np.float64), dtype=np.float64)
    for form in (1, 0):
        knob("xf", form)
        s, gr = m.score_grad_raw(q.cuda())
        es, eg = relerr(_n(s), so), relerr(_n(gr), go)
        assert es < TOL and eg < TOL, (spread, form, es, eg)


@pytest.mark.parametrize("name", ["cfg2_baxter_poly1", "cfg2_baxter_rq", "headline_baxter_poly1_s2000"])
def test_tile_of_16_configurations_against_the_split_launch_and_the_oracle(ops, name, knob):
    """round 4: small batches of a one-class D = 12 model run as blocks of 16 configurations that sweep
    ALL the rows from an LDS copy (score_kernel.h QT; knob qt = 1 forces it wherever it fits, 0 = the split launch).  Same
    pairs, direct form, another summation order: both sit at the oracle, ragged batches included, score-and-gradient,
    upstream scaling, the hinge gradient and the C = 1 Jacobian."""
    d = load(name)
    kind, p0, p1 = case_kernel(d)
    S = min(len(d["sup_x32"]), 1000)   # (a 2000-row model does not fit the LDS beside 16 waves' partial rows: its first 1000)
    m = ops.ScoreModel(desc_for(CASE_ROBOT[name]), kind, p0, p1, _t(d["sup_x32"][:S].reshape(S, -1)), _t(d["weights"][:S]))
    from oracle import oracle
    for n in (1, 15, 16, 17, 100, 256):
        q = _t(d["q"][:n])
        knob("qt", 0)
        s0, g0 = m.score_grad_raw(q)
        knob("qt", 1)
        s1, g1 = m.score_grad_raw(q)
        assert not torch.equal(g0, g1) or n == 1, "the knob did not change the launch"
        so, go, _ = oracle.score_grad(desc_for(CASE_ROBOT[name]), kind, p0, p1, d["sup_x32"][:S], d["weights"][:S], d["q"][:n], dtype=np.float64)
        assert relerr(_n(s1), so) < TOL and relerr(_n(g1), go) < TOL, (n, relerr(_n(g1), go))
        assert torch.equal(m.score_raw(q), s1)        # the score-only launch takes the tile too: same sums, no gradient
        # (the split launch it is compared with may be the EXPANDED form - RQ: ~2e-6 from the referee itself; the tile is direct)
        assert relerr(_n(s1), _n(s0)) < 8e-6 and relerr(_n(g1), _n(g0)) < 8e-6
        up = torch.linspace(-1.5, 2.0, n, device=q.device)[:, None]
        a, b = m.score_grad_raw(q, up)[1], None
        knob("qt", 0)
        b = m.score_grad_raw(q, up)[1]
        assert relerr(_n(a), _n(b)) < 8e-6
        h0 = m.score_hinge_grad_raw(q, 0.1, 2.0)
        j0 = m.score_jac_raw(q)[1]
        knob("qt", 1)
        if h0 is not None:
            h1 = m.score_hinge_grad_raw(q, 0.1, 2.0)
            clear = (h0[0][:, 0] - 0.1).abs() > 1e-3   # (rows whose score sits on the hinge may switch with the rounding)
            if bool(clear.any()):
                assert relerr(_n(h1[1][clear]), _n(h0[1][clear])) < 8e-6
        assert relerr(_n(m.score_jac_raw(q)[1]), _n(j0)) < 8e-6
    knob("qt", -1)


def test_tile_of_16_configurations_is_bit_stable_across_batch_order(ops, knob):
    """a configuration's result does not depend on where it stands in the batch, on its neighbours in the block, or on the
    launch: the tile's sums have a fixed order (slices of the rows, waves, the four slices of a wave)"""
    d = load("cfg2_baxter_poly1")
    kind, p0, p1 = case_kernel(d)
    m = ops.ScoreModel(desc_for("baxter_left"), kind, p0, p1, _t(d["sup_x32"].reshape(len(d["sup_x32"]), -1)), _t(d["weights"]))
    g = torch.Generator().manual_seed(5)
    q = _t(d["q"][:200])
    knob("qt", 1)
    s0, g0 = m.score_grad_raw(q)
    for _ in range(3):
        perm = torch.randperm(200, generator=g).to(q.device)
        s1, g1 = m.score_grad_raw(q[perm].contiguous())
        assert torch.equal(s1, s0[perm]) and torch.equal(g1, g0[perm])
    s2, g2 = m.score_grad_raw(q[37:38].contiguous())   # alone in its block
    assert torch.equal(s2, s0[37:38]) and torch.equal(g2, g0[37:38])
    knob("qt", -1)


@pytest.mark.parametrize("S", [64, 65, 130, 1023, 1100])
def test_tile_of_16_configurations_row_counts(ops, knob, S):
    """slices of unequal length end in zero-weight rows; the largest model that fits beside 16 waves' partial rows"""
    from oracle import oracle
    g = np.random.default_rng(S)
    desc = desc_for("baxter_left")
    q = g.uniform(-1.5, 1.5, (70, 7)).astype(np.float32)
    sup = oracle.fkine(desc, g.uniform(-1.5, 1.5, (S, 7)).astype(np.float32)).reshape(S, -1)
    w = g.standard_normal((S, 1)).astype(np.float32)
    m = ops.ScoreModel(desc, KIND["poly"], 1, 1.0, _t(sup), _t(w))
    knob("qt", 1)
    s1, g1 = m.score_grad_raw(_t(q))
    so, go, _ = oracle.score_grad(desc, KIND["poly"], 1, 1.0, sup, w, q, dtype=np.float64)
    assert relerr(_n(s1), so) < TOL and relerr(_n(g1), go) < TOL
    knob("qt", -1)


@pytest.mark.parametrize("kspec", [("poly", 1, 1.0), ("rq", 10.0, 2.0)])
def test_tile_of_16_configurations_on_raw_inputs(ops, knob, kspec):
    """no transform (DCX_FK_NONE, D = 12): the tile form is the direct form on the caller's own numbers - exact differences,
    a query sitting ON a support included (r = 0: value 0, sub-gradient 0 for Polyharmonic)"""
    from diffco_amd import _fkdesc
    from oracle import oracle
    kind, p0, p1 = KIND[kspec[0]], kspec[1], kspec[2]
    g = np.random.default_rng(12)
    S, B = 700, 333
    sup = g.uniform(-3, 3, (S, 12)).astype(np.float32)
    w = g.standard_normal((S, 1)).astype(np.float32)
    x = g.uniform(-3, 3, (B, 12)).astype(np.float32)
    x[:40] = sup[:40]                      # r = 0 pairs
    x[40:80] = sup[40:80] + 1e-4           # and near ones
    raw = _fkdesc.none_desc(12)
    m = ops.ScoreModel(raw, kind, p0, p1, _t(sup), _t(w))
    knob("qt", 1)
    s1, g1 = m.score_grad_raw(_t(x))
    knob("qt", 0)
    s0, g0 = m.score_grad_raw(_t(x))
    knob("qt", -1)
    so, go, _ = oracle.score_grad(raw, kind, p0, p1, sup, w, x, dtype=np.float64)
    assert not torch.equal(g0, g1)
    assert relerr(_n(s1), so) < TOL and relerr(_n(g1), go) < TOL
    assert torch.isfinite(g1).all()


@pytest.mark.parametrize("name", ["headline_baxter_poly1_s2000", "cfg3_baxter_rq_c5"])
def test_wave_group_shares_tile_the_rows(ops, name, knob):
    """the unequal slices of a block's wave groups (score_kernel.h wave_slice, knobs skew / skew8): whatever the shares - the rules',
    one group taking everything, shares that overshoot the block's rows, a last group left with nothing - every support is swept
    exactly once: scores, gradients and Jacobians agree with the equal slices to the order of the fp32 sums, in the unsplit and the
    split launch, on 16- and 8-wave blocks"""
    d = load(name)
    m, _, _ = _model(ops, name, d)
    rng = np.random.default_rng(3)
    B = 700
    q = _t(np.repeat(d["q"], -(-B // len(d["q"])), axis=0)[:B] + 0.05 * rng.standard_normal((B, d["q"].shape[1])).astype(np.float32))
    up = _t(rng.standard_normal((B, m.C)).astype(np.float32)) if m.C > 1 else None

    def pack(w0, w1, w2):
        return w0 | (w1 << 10) | (w2 << 20)

    def run():
        s, g = m.score_grad_raw(q, up)
        return _n(s), _n(g), _n(m.score_raw(q)), _n(m.score_jac_raw(q)[1])

    for nw, ys in ((16, 1), (16, 3), (8, 1), (8, 2)):
        knob("nw", nw)
        knob("ys", ys)
        knob("skew", 0)
        knob("skew8", 0)
        ref = run()
        cases = [("skew", v) for v in (-1, pack(480, 320, 150), pack(1000, 0, 0), pack(10, 10, 10), pack(700, 700, 700), pack(333, 333, 334),
                                       pack(0, 0, 1000), pack(1, 998, 1))] if nw == 16 else \
                [("skew8", v) for v in (-1, 600, 1000, 10, 500, 999)]
        for k, v in cases:
            knob(k, v)
            out = run()
            for a, b in zip(out, ref):
                assert a.shape == b.shape and relerr(a, b) < 3e-6, (nw, ys, k, v)
            knob(k, 0)
