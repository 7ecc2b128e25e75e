"""GPU tests of the spare-slot form of the expanded sweep (score_kernel.h spare_applies / sweep_rows SP): a model whose kept
supports agree bit for bit on one feature column (Baxter's first control point has a fixed height) carries |s - c|^2 and the
constant 1 in that column's slots of the packed fmas.  Every case that is meant to run the form first proves that it did
(knob spare: -1 = the rule, 0 = the plain expanded form - the outputs differ in their last bits), then holds it to the fp64
oracle at the tolerance the expanded form has everywhere else (test_gpu_parity.py TOL)."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import make_robot, relerr

pytestmark = pytest.mark.gpu

TOL = 1e-5          # test_gpu_parity.py: max|a - ref| / max|ref| against the fp64 referee
B, S = 70, 1203     # one full tile + six lanes; four waves' slices of 301 / 300 rows: > DCX_XF_FLUSH, not multiples of four
KERNELS = {"poly1": (1, 1.0, 1.0), "rq2": (0, 10.0, 2.0)}


@pytest.fixture
def spare(knob):
    """spare(v): the developer knob of the form (conftest's `knob` restores only the knobs it lists)"""
    knob("spare", -1)
    yield lambda v: knob("spare", v)
    knob("spare", -1)


@pytest.fixture(scope="module")
def data():
    from diffco_amd import _lib, _ops
    _lib.require_gpu()
    rob = make_robot("baxter_left")
    g = torch.Generator().manual_seed(1203)
    lim = rob.limits
    rnd = lambda n: torch.rand((n, rob.dof), generator=g) * (lim[:, 1] - lim[:, 0]) + lim[:, 0]
    sup_q, q = rnd(S), rnd(B)
    desc = rob.fk_desc()
    sup = _ops.fkine(desc, sup_q.cuda()).reshape(S, -1).contiguous()
    assert float(sup[:, 2].max() - sup[:, 2].min()) == 0.0      # the column the form lives on
    w = (0.05 * torch.randn(S, generator=g)).cuda()
    return dict(rob=rob, desc=desc, sup_q=sup_q.cuda(), q=q.cuda(), sup=sup, w=w)


def _oracle(desc, kern, sup, w, q):
    from oracle import oracle
    s, g, _ = oracle.score_grad(desc, *kern, sup.cpu().double().numpy(), w.cpu().numpy().astype(np.float64),
                                q.cpu().numpy().astype(np.float64), dtype=np.float64)
    return s, g


def _run_both(m, q, spare):
    spare(0)
    plain = m.score_grad_raw(q)
    spare(-1)
    rule = m.score_grad_raw(q)
    return rule, plain


def _check(tag, out, ref):
    (s, g), (so, go) = out, ref
    es, eg = relerr(s.cpu().numpy(), so.reshape(s.shape)), relerr(g.cpu().numpy(), go)
    print(f"{tag}: score {es:.2e} grad {eg:.2e}")
    assert torch.isfinite(s).all() and torch.isfinite(g).all(), tag
    assert es < TOL and eg < TOL, (tag, es, eg)


def _ran_spare(rule, plain):
    return not (torch.equal(rule[0], plain[0]) and torch.equal(rule[1], plain[1]))


@pytest.mark.parametrize("geometry", ["four_waves", "sixteen_waves"])
@pytest.mark.parametrize("kname", sorted(KERNELS))
def test_score_and_gradient_against_float64(data, kname, geometry, knob, spare):
    """(a) random queries; (c) the supports moved to another base height: still one agreed column, but the queries' own
    value there differs from it by 0.05 - e = x - v enters |x|^2, the near threshold and the gradient"""
    from diffco_amd import _ops
    # unsplit blocks (a batch this small would take the quarter tile, which has no expanded form): slices of 301 / 300 rows -
    # several flushes and a tail of one row - or of 76 rows: one flush, no tail
    knob("nw", 4 if geometry == "four_waves" else 16)
    knob("ys", 1)
    kern = KERNELS[kname]
    for tag, dz in (("a", 0.0), ("c", 0.05)):
        sup = data["sup"].clone()
        sup[:, 2] += dz
        m = _ops.ScoreModel(data["desc"], *kern, sup, data["w"])
        rule, plain = _run_both(m, data["q"], spare)
        assert _ran_spare(rule, plain), (tag, "the spare form did not run")
        ref = _oracle(data["desc"], kern, sup, data["w"], data["q"])
        _check(f"({tag}) {kname} {geometry} spare", rule, ref)
        _check(f"({tag}) {kname} {geometry} plain", plain, ref)


@pytest.mark.parametrize("kname", sorted(KERNELS))
def test_queries_on_top_of_supports(data, kname, knob, spare):
    """(b) d2 = 0 for one pair per query: Polyharmonic(1)'s near-pair block takes the expanded term out and puts the direct
    one in, over the first D - 1 columns plus e"""
    from diffco_amd import _ops
    knob("nw", 4)
    knob("ys", 1)
    kern = KERNELS[kname]
    m = _ops.ScoreModel(data["desc"], *kern, data["sup"], data["w"])
    q = data["sup_q"][:B].contiguous()
    rule, plain = _run_both(m, q, spare)
    assert _ran_spare(rule, plain), "the spare form did not run"
    # (the referee walks the arm in float64: it gets ITS OWN features of the support configurations, so that the coincident
    # pairs coincide there as well - test_gpu_parity.py does the same for its r = 0 cases)
    from oracle import oracle
    sup64 = torch.from_numpy(oracle.fkine(data["desc"], data["sup_q"].cpu().numpy().astype(np.float64), dtype=np.float64).reshape(S, -1))
    ref = _oracle(data["desc"], kern, sup64, data["w"], q)
    _check(f"(b) {kname} spare", rule, ref)
    _check(f"(b) {kname} plain", plain, ref)


@pytest.mark.parametrize("route", ["device", "host"])
def test_rule_follows_the_supports_through_updates(data, route, knob, spare):
    """(d) one support off the common height: no agreed column, the model keeps the plain form - the knob changes nothing;
    (e) dcx_model_update flips the property off and on again, right after each refill; the host packing route and the
    packing kernel decide the same and build the same rows"""
    from diffco_amd import _ops
    knob("nw", 4)
    knob("ys", 1)
    kern = KERNELS["poly1"]
    put = (lambda t: t) if route == "device" else (lambda t: t.cpu())
    bent = data["sup"].clone()
    bent[5, 2] += 0.01
    other = lambda t: t.cpu() if route == "device" else t.cuda()
    for first, second in ((bent, data["sup"]), (data["sup"], bent)):
        m = _ops.ScoreModel(data["desc"], *kern, put(first), put(data["w"]), capacity=S)
        twin = _ops.ScoreModel(data["desc"], *kern, other(first), other(data["w"]), capacity=S)   # the other packing route
        for n, sup in enumerate((first, second, first)):
            if n:
                m.update(put(sup), put(data["w"]))
                twin.update(other(sup), other(data["w"]))
            rule, plain = _run_both(m, data["q"], spare)
            assert _ran_spare(rule, plain) == (sup is data["sup"]), (route, n)
            _check(f"(d/e) {route} refill {n}", rule, _oracle(data["desc"], kern, sup, data["w"], data["q"]))
            t = twin.score_grad_raw(data["q"])
            assert torch.equal(t[0], rule[0]) and torch.equal(t[1], rule[1]), (route, n, "host and device packing differ")


def test_score_only_and_trajectory_step_take_the_same_form(data, knob, spare):
    """(f) the entry points of one model agree as they do in the plain form: the score-only launch within 3e-6 of the
    score + gradient launch's (test_gpu_parity.py), the hinge gradient's score bit-identical to it (test_gpu_traj.py), the
    persistent trajectory kernel bit-identical to the launch-per-iteration loop - and each of them moved with the knob"""
    from diffco_amd import _lib, _ops
    from test_gpu_traj import _random_paths, _traj_state
    lib = _lib.require_gpu()
    knob("nw", 4)
    knob("ys", 1)
    knob("traj_ys", 1)
    kern = KERNELS["poly1"]
    m = _ops.ScoreModel(data["desc"], *kern, data["sup"], data["w"])
    q = data["q"]
    out = {}
    for v in (-1, 0):
        spare(v)
        s, g = m.score_grad_raw(q)
        s0 = m.score_raw(q)
        assert relerr(s0.cpu().numpy(), s.cpu().numpy()) < 3e-6
        sh, gh = m.score_hinge_grad_raw(q, float(s.median()), 2.5)
        assert torch.equal(sh, s)
        mask = ((s - float(s.median())) > 0).float() * 2.5
        assert relerr(gh.cpu().numpy(), (g * mask).cpu().numpy()) < 1e-6
        paths = _random_paths(data["rob"], 3, 20, seed=7)
        opt = _lib.TrajOpts(0.02, 0.9, 0.999, 1e-8, 1, 10, 10, 10, float(s.median()), 0.3, 1e9, 0.35)
        runs = []
        for fused in (0, 1):
            knob("traj_fused", fused)
            st, bufs = _traj_state(m, data["rob"], paths)
            _lib.check(lib.dcx_traj_adam_run(m._h, C.byref(st), C.byref(opt), 1, 3,
                                             C.c_void_p(torch.cuda.current_stream(m.dev).cuda_stream)))
            torch.cuda.synchronize()
            runs.append({k: t.clone() for k, t in bufs.items() if k not in ("col_score", "col_grad", "limits")})
        knob("traj_fused", -1)
        for k in runs[0]:
            assert torch.equal(runs[0][k], runs[1][k]), (v, k)
        out[v] = (s, g, s0, runs[1]["stats"], runs[1]["path"])
    assert not torch.equal(out[-1][1], out[0][1])                                   # score + gradient
    assert not torch.equal(out[-1][2], out[0][2])                                   # score only
    assert not (torch.equal(out[-1][3], out[0][3]) and torch.equal(out[-1][4], out[0][4]))   # the trajectory kernels
