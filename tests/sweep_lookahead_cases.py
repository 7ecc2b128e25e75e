"""The launches of tests/test_gpu_sweep_lookahead.py, shared with tools/record_sweep_lookahead_parent_bits.py (which ran them once
on the library of the commit before the four-row pipeline took its rows through one advancing pointer with an unclamped look-ahead:
tests/golden/sweep_lookahead_parent_bits.npz, keys <case>_s / <case>_g).  Inputs the way spare_prestage_cases.py makes them; the
seed is here.

Baxter's left arm (the spare-slot form: agreed column 2), B = 70 (one full tile and six lanes), both specialised kernel functions.
The supports of every case are the first S of one set of 2000 configurations.  What each group is for (score_kernel.h sweep_rows,
the PARTS == 0 pipeline):
    S{15,16,17,18}_nw1          one wave, one slice: every remainder of the four-row loop (3, 0, 1, 2 tail rows); the look-ahead of
                                the last iteration reaches the rows behind the model's last one
    S{63,64,65,67,68}_nw1       a slice that ends just before, on and just behind the second flush of the expanded gradient
    S2000_nw{16,8}              the skewed slices of 16- and 8-wave blocks: interior slice ends of every alignment, where the
                                look-ahead reads the next wave's rows
    cap_{dev,host}              a model created at exactly its capacity (S = 66, two tail rows) by the packing kernel and by the
                                host route: the look-ahead reads the storage's tail and nothing else
    upd_{dev,host}_{small,back} the same model refilled in place with 37 supports (the tail now stands where rows 37 .. were),
                                then with all 66 again"""
import torch

B = 70
S_MAX = 2000
SEED = 2300
KERNELS = {"poly1": (1, 1.0, 1.0), "rq2": (0, 10.0, 2.0)}
KNOBS = ("nw", "ys", "spare", "min_rows")
SLICE_SIZES = (15, 16, 17, 18)
FLUSH_SIZES = (63, 64, 65, 67, 68)
SKEW_NWS = (16, 8)
S_CAP = 66
S_SMALL = 37
ROUTES = ("dev", "host")
# (name, S, nw)
PLAIN_LAUNCHES = [(f"S{S}_nw1", S, 1) for S in SLICE_SIZES + FLUSH_SIZES] + [(f"S{S_MAX}_nw{nw}", S_MAX, nw) for nw in SKEW_NWS]
STORAGE_LAUNCHES = [(f"cap_{r}", S_CAP) for r in ROUTES] + [(f"upd_{r}_{step}", S) for r in ROUTES
                                                            for step, S in (("small", S_SMALL), ("back", S_CAP))]


def keys():
    return [f"{k}_{name}" for k in sorted(KERNELS) for name, *_ in PLAIN_LAUNCHES + STORAGE_LAUNCHES]


def size_of(key):
    name = key.split("_", 1)[1]
    return {n: s for n, s, *_ in PLAIN_LAUNCHES + STORAGE_LAUNCHES}[name]


def baxter_inputs():
    """(robot, support configurations [S_MAX, 7], weights [S_MAX], queries [B, 7]); CPU tensors"""
    from helpers import make_robot
    rob = make_robot("baxter_left")
    g = torch.Generator().manual_seed(SEED)
    lim = rob.limits
    rnd = lambda n: torch.rand((n, rob.dof), generator=g) * (lim[:, 1] - lim[:, 0]) + lim[:, 0]  # noqa: E731
    sup_q = rnd(S_MAX)
    w = 0.05 * torch.randn(S_MAX, generator=g)
    return rob, sup_q, w, rnd(B)


def run_all(set_knob):
    """every launch: ({"<case>": (score, gradient)} CPU numpy, {"<case>": the same launch with knob spare = 0}, context)"""
    from diffco_amd import _lib, _ops
    _lib.require_gpu()
    rob, sup_q, w, q = baxter_inputs()
    desc = rob.fk_desc()
    sup = _ops.fkine(desc, sup_q.cuda()).reshape(S_MAX, -1).contiguous()
    assert float(sup[:, 2].max() - sup[:, 2].min()) == 0.0      # the column the spare form lives on
    wd, qd = w.cuda(), q.cuda()
    place = {"dev": lambda t: t, "host": lambda t: t.cpu()}
    out, plain = {}, {}

    def launch(key, m, nw):
        set_knob("nw", nw)
        for dst, spare in ((out, -1), (plain, 0)):
            set_knob("spare", spare)
            try:
                s, g = m.score_grad_raw(qd)
                torch.cuda.synchronize()
                dst[key] = (s.cpu().numpy().copy(), g.cpu().numpy().copy())
            finally:
                set_knob("spare", -1)

    set_knob("min_rows", 1)
    set_knob("ys", 1)
    for kname, kern in KERNELS.items():
        for name, S, nw in PLAIN_LAUNCHES:
            launch(f"{kname}_{name}", _ops.ScoreModel(desc, *kern, sup[:S].contiguous(), wd[:S].contiguous()), nw)
        for r in ROUTES:
            at = place[r]
            m = _ops.ScoreModel(desc, *kern, at(sup[:S_CAP].contiguous()), at(wd[:S_CAP].contiguous()))
            assert m.capacity == S_CAP
            launch(f"{kname}_cap_{r}", m, 1)
            m.update(at(sup[:S_SMALL].contiguous()), at(wd[:S_SMALL].contiguous()))
            launch(f"{kname}_upd_{r}_small", m, 1)
            m.update(at(sup[:S_CAP].contiguous()), at(wd[:S_CAP].contiguous()))
            assert m.capacity == S_CAP
            launch(f"{kname}_upd_{r}_back", m, 1)
    return out, plain, dict(desc=desc, sup_q=sup_q, w=w, q=q)


def reset_knobs(lib):
    for k in KNOBS:
        lib.dcx_debug_set(k.encode(), -1)
