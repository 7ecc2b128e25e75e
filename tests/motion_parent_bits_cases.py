"""The cases of tests/test_gpu_motion_parent_bits.py, shared with tools/record_motion_parent_bits.py: the four motion calls on
edge sets that put every shared piece of motion_tile.h to work - the tile lookup (tiles holding many short edges, an edge over
three tiles, a partial last tile, an empty edge, an edge over max_samples), the interpolation under both rules, with a wrap mask
and with the open end, both block folds and the split hand-over (the launch forms) - and run_all(), which returns every output
as a numpy array."""
import numpy as np

F = np.float32
E = 130
STEP = 0.02
MAX_SAMPLES = 80
RES = 9
ZERO_EDGE, LONG_EDGE = 5, 40          # an edge of length 0 (one sample: its target) and one over max_samples (not checked)
# (fixture, wrap mask): D = 12 with one and with five classes, D = 4 on the circle, D = 24
MODELS = [("cfg2_baxter_poly1", 0), ("cfg3_baxter_rq_c5", 0), ("cfg1_planar2_rq", 0b11), ("misc_dualbaxter_poly1", 0)]
GRAD_MODELS = ("cfg2_baxter_poly1", "cfg3_baxter_rq_c5")   # dcx_motion_worst's gradients: one class and five
# tests/test_gpu_motion_worst.py test_batch_sizes_and_launch_forms' list of (ys, nw).  Under max_step the grid's bound is 163
# tiles, so ys = 4 would need 652 partial rows and runs unsplit (dcx_api.hip kMotionSplitRows); under res = 9 (19 tiles) it splits.
FORMS = [(-1, -1), (1, 16), (1, 8), (4, 16), (2, 8)]
FULL_FORMS = [(-1, -1), (2, 8)]     # the forms at which GRAD_MODELS' gradients under max_step are kept whole (the rule's form, a split one)
UNC_CAP = 64


def sample_counts():
    """the closed max_step rule's sample counts the edges are built for: 1 .. 70 drawn at random, then the layout forced"""
    n = np.random.default_rng(18).integers(1, 71, E)
    n[ZERO_EDGE] = 1
    n[LONG_EDGE] = 0                                    # (takes no room in the work list)
    start = np.concatenate([[0], np.cumsum(n)])
    e = next(i for i in range(50, E) if start[i] % 64 >= 60 and i != LONG_EDGE)
    n[e] = 70                                           # 4 or fewer samples in its first tile, 64, the rest in a third
    if n.sum() % 64 == 0:
        n[E - 1] += 1
    return n


def layout_ok(n):
    """the properties of the work list the cases exist for, from the calls' n_samples (-2 for LONG_EDGE apart)"""
    n = np.where(np.arange(E) == LONG_EDGE, 0, n).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(n)])
    first, last = start[:-1] // 64, (start[1:] - 1) // 64
    spans3 = bool(((last - first)[n > 0] >= 2).any())
    crowded = int(np.bincount(first[n > 0]).max()) >= 4
    return spans3 and crowded and int(start[-1]) % 64 != 0


def edges(q, mask):
    """E edges from the fixture's configurations with sample_counts()' counts under max_step = STEP"""
    from motion_wrap_helpers import wrap2pi32
    g = np.random.default_rng(7)
    n = sample_counts()
    qa = q[g.integers(0, len(q), E)].astype(F)
    u = g.standard_normal(qa.shape)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    length = np.where(n > 1, (n - 1.5) * STEP, 0.0)     # ceil(L / step) interior samples and the target
    length[LONG_EDGE] = 3 * MAX_SAMPLES * STEP
    qb = (qa + u * length[:, None]).astype(F)
    qb[ZERO_EDGE] = qa[ZERO_EDGE]
    if mask:                                            # the same wrapped edge, its target taken across the seam where it leaves
        qb = wrap2pi32(qb)
    return qa, qb, n


def fold(a):
    """[n, dof] float32 -> [n] uint32: FNV-1a over each row's words in column order (64-bit, its halves xor-ed), so a changed bit,
    two entries swapped or the same bit flipped in two entries all change it.  The recording keeps one word per row of the
    gradients and of the listed configurations - a tenth of their size - and GRAD_MODELS' gradients whole at FULL_FORMS."""
    w = np.ascontiguousarray(a, F).view(np.uint32).astype(np.uint64)
    h = np.full(len(w), 0xcbf29ce484222325, np.uint64)
    for j in range(w.shape[1]):
        h = (h ^ w[:, j]) * np.uint64(0x100000001b3)
    return ((h >> np.uint64(32)) ^ (h & np.uint64(0xffffffff))).astype(np.uint32)


def run_all(ops, set_knob, set_early_exit):
    """{"<fixture>|<rule>|<output>": array [len(FORMS), ...]} of every case, the launch forms stacked in FORMS' order (list
    entries behind the list's end: 0); "<output>_fold": fold() of an [E, dof] output; GRAD_MODELS' gradients under max_step also
    whole, [len(FULL_FORMS), E, dof]"""
    import torch
    from motion_worst_helpers import class_margins, fixture_model
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32, device="cuda")
    out = {}
    for name, mask in MODELS:
        d, desc, kern, sup, W = fixture_model(name)
        m = ops.ScoreModel(desc, kern[0], kern[1], kern[2], t(sup), t(W))
        lo, mg, hi = (class_margins(d["score64"], p) for p in (60, 75, 90))
        qa, qb, _ = edges(d["q"], mask)
        a, b = t(qa), t(qb)
        for rule, kw in (("res", dict(res=RES)), ("step", dict(max_step=STEP, max_samples=MAX_SAMPLES))):
            for ys, nw in FORMS:
                set_knob("ys", ys)
                set_knob("nw", nw)
                key = f"{name}|{rule}|"
                put = lambda k, v: out.setdefault(key + k, []).append(v.cpu().numpy() if torch.is_tensor(v) else v)
                for ee in (1, 0):
                    set_early_exit(ee)
                    first, n = m.check_motions(a, b, margin=mg, wrap=mask, **kw)
                    put(f"check_first_hit_ee{ee}", first)
                    put(f"check_n_samples_ee{ee}", n)
                set_early_exit(-1)
                grad = name in GRAD_MODELS
                r = m.motion_worst_raw(a, b, margin=mg, wrap=mask, grad=grad, **kw)
                for k, v in zip(("worst", "worst_idx", "worst_class", "worst_n_samples"), r):
                    put(k, v)
                whole = grad and rule == "step" and (ys, nw) in FULL_FORMS
                if grad:
                    put("worst_grad_a_fold", fold(r[4].cpu().numpy()))
                    put("worst_grad_b_fold", fold(r[5].cpu().numpy()))
                if whole:
                    put("worst_grad_a", r[4])
                    put("worst_grad_b", r[5])
                r = m.motion_band_raw(a, b, lo, hi, wrap=mask, unc_cap=UNC_CAP, **kw)
                for k in ("verdict", "first_hit", "n_samples", "n_uncertain", "unc_total"):
                    put("band_" + k, r[k])
                listed = np.arange(UNC_CAP) < int(r["unc_total"])
                put("band_unc_edge", np.where(listed, r["unc_edge"].cpu().numpy(), 0))
                put("band_unc_sample", np.where(listed, r["unc_sample"].cpu().numpy(), 0))
                put("band_unc_q_fold", np.where(listed, fold(r["unc_q"].cpu().numpy()), 0))
                for tag, oe in (("cost", False),) + ((("cost_open", True),) if rule == "step" else ()):
                    cost, ga, gb, n = m.motion_cost_raw(a, b, margin=mg, weight=0.75, open_end=oe, wrap=mask, **kw)
                    put(tag, cost)
                    put(tag + "_n_samples", n)
                    put(tag + "_grad_a_fold", fold(ga.cpu().numpy()))
                    put(tag + "_grad_b_fold", fold(gb.cpu().numpy()))
                    if whole and not oe:
                        put("cost_grad_a", ga)
                        put("cost_grad_b", gb)
    set_knob("ys", -1)
    set_knob("nw", -1)
    return {k: np.stack(v) for k, v in out.items()}
