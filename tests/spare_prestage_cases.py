"""The launches of tests/test_gpu_spare_prestage.py, shared with tools/record_spare_prestage_parent_bits.py (which ran them once
on the library of the commit before the pre-staged spare-slot sweep: tests/golden/spare_prestage_parent_bits.npz, keys
<case>_s / <case>_g).  Inputs the way test_gpu_spare_lean.py makes them; the seeds are here.

Baxter's left arm (agreed column 2, exchanged with column 11), B = 70 (one full tile and six lanes), S = 203 (odd slice starts and
tails), both specialised kernel functions, every block size, unsplit and split in two.  Which way each launch takes through
score_body's epilogue, by the host's rules (dcx_api.hip run_score / pick_geometry; knob min_rows = 1 keeps the asked block size
at this small S; 2 tiles x 2 super-chunks = 4 blocks, 13 accumulators):
    nw1_ys1                 one wave per block: no fold, the exchange undone where G is written
    nw{2,4,8,16}_ys1        the parallel fold (NWC = 2, 4, 8, 16), exchange undone by index in it; J^T on several waves from nw = 8
                            (its scratch needs (nw - 1) 13 >= 49 floats per lane), wave 0 alone behind the fold at nw = 2, 4
    nw1_ys2                 the one-wave in-launch hand-over (arrival counter): exchange undone in the published row
    nw{2,4}_ys2             parallel fold + split publish with the arrival counter's re-read (13 accumulators > 2 nw: no owner-polls)
    nw{8,16}_ys2            parallel fold + the owner-polls hand-over (knob owner_poll = 1 vouches for the stream)
    nw{8,16}_ys2_counter    the same blocks with owner_poll = 0: the arrival counter
    nw{1,4}_ys2_finish      split_finish_kernel = 1: the partial rows go to score_finish_kernel (no parallel fold in the block)
    nw{8,16}_ys1_jt0        jt_waves = 0: wave 0 alone takes the folded row through G and J^T
A planar arm of five links (10 features in the width 12: the padding is the agreed column, c = D - 1, the identity exchange, and
d_fk != D), Polyharmonic(1); and one of six links (12 features, no agreed column): the plain expanded kernel."""
import torch

B = 70
S = 203
SEED = 2100
KERNELS = {"poly1": (1, 1.0, 1.0), "rq2": (0, 10.0, 2.0)}
NWS = (1, 2, 4, 8, 16)
YSS = (1, 2)
KNOBS = ("nw", "ys", "spare", "min_rows", "owner_poll", "split_finish_kernel", "jt_waves")
# (name suffix, nw, ys, extra knobs)
BAXTER_LAUNCHES = [(f"nw{nw}_ys{ys}", nw, ys, {"owner_poll": 1} if (ys == 2 and nw >= 8) else {}) for nw in NWS for ys in YSS] + [
    ("nw8_ys2_counter", 8, 2, {"owner_poll": 0}), ("nw16_ys2_counter", 16, 2, {"owner_poll": 0}),
    ("nw1_ys2_finish", 1, 2, {"split_finish_kernel": 1}), ("nw4_ys2_finish", 4, 2, {"split_finish_kernel": 1}),
    ("nw8_ys1_jt0", 8, 1, {"jt_waves": 0}), ("nw16_ys1_jt0", 16, 1, {"jt_waves": 0})]
PLANAR_LAUNCHES = [(f"nw{nw}_ys{ys}", nw, ys, {}) for nw in (1, 4, 16) for ys in YSS]
PLANAR5 = [0.31, 0.27, 0.22, 0.18, 0.12]            # 10 features, compiled width 12
PLANAR6 = [0.31, 0.27, 0.22, 0.18, 0.12, 0.09]      # 12 features: nothing agreed


def baxter_inputs():
    """(robot, support configurations [S, 7], weights [S], queries [B, 7]); CPU tensors"""
    from helpers import make_robot
    rob = make_robot("baxter_left")
    g = torch.Generator().manual_seed(SEED)
    lim = rob.limits
    rnd = lambda n: torch.rand((n, rob.dof), generator=g) * (lim[:, 1] - lim[:, 0]) + lim[:, 0]  # noqa: E731
    sup_q = rnd(S)
    w = 0.05 * torch.randn(S, generator=g)
    return rob, sup_q, w, rnd(B)


def planar_inputs(links):
    """(FK description, support configurations [S, dof], weights [S], queries [B, dof])"""
    from diffco_amd import _fkdesc as fd
    desc = fd.planar_desc(list(links))
    g = torch.Generator().manual_seed(SEED + len(links))
    rnd = lambda n: 3.0 * torch.rand((n, len(links)), generator=g) - 1.5  # noqa: E731
    sup_q = rnd(S)
    w = 0.05 * torch.randn(S, generator=g)
    return desc, sup_q, w, rnd(B)


def run_all(set_knob):
    """every launch: ({"<case>": (score, gradient)} CPU numpy, {"<case>": the same launch with knob spare = 0}, context)"""
    from diffco_amd import _lib, _ops
    _lib.require_gpu()

    def launch(m, q, nw, ys, extra):
        set_knob("nw", nw)
        set_knob("ys", ys)
        for k, v in extra.items():
            set_knob(k, v)
        try:
            s, g = m.score_grad_raw(q)
            torch.cuda.synchronize()
            return s.cpu().numpy().copy(), g.cpu().numpy().copy()
        finally:
            for k in extra:
                set_knob(k, -1)

    out, plain, ctx = {}, {}, {}
    set_knob("min_rows", 1)
    set_knob("spare", -1)
    rob, sup_q, w, q = baxter_inputs()
    desc = rob.fk_desc()
    sup = _ops.fkine(desc, sup_q.cuda()).reshape(S, -1).contiguous()
    assert float(sup[:, 2].max() - sup[:, 2].min()) == 0.0 and float(sup[:, 11].max() - sup[:, 11].min()) > 0.0
    ctx["baxter"] = dict(desc=desc, sup_q=sup_q, w=w, q=q)
    models = [("baxter", kname, _ops.ScoreModel(desc, *kern, sup, w.cuda()), q.cuda(), BAXTER_LAUNCHES) for kname, kern in KERNELS.items()]
    for tag, links in (("planar5", PLANAR5), ("planar6", PLANAR6)):
        pdesc, psup_q, pw, pq = planar_inputs(links)
        psup = _ops.fkine(pdesc, psup_q.cuda()).reshape(S, -1).contiguous()
        assert psup.shape[1] == 2 * len(links)
        ctx[tag] = dict(desc=pdesc, sup_q=psup_q, w=pw, q=pq)
        models.append((tag, "poly1", _ops.ScoreModel(pdesc, *KERNELS["poly1"], psup, pw.cuda()), pq.cuda(), PLANAR_LAUNCHES))
    for tag, kname, m, qd, launches in models:
        for name, nw, ys, extra in launches:
            key = f"{tag}_{kname}_{name}"
            out[key] = launch(m, qd, nw, ys, extra)
            set_knob("spare", 0)
            try:
                plain[key] = launch(m, qd, nw, ys, extra)
            finally:
                set_knob("spare", -1)
    return out, plain, ctx


def reset_knobs(lib):
    for k in KNOBS:
        lib.dcx_debug_set(k.encode(), -1)
