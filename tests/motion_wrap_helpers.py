"""Shared by the CPU and GPU tests of the wrapped motion calls (dcx_check_motions_ex, dcx_motion_cost_ex): the fp32 samples
of include/dcx.h's rule formed operation by operation in numpy float32, on the pattern of helpers.motion_samples (whose tuples
they reproduce, so helpers.motion_chain and helpers.motion_oracle* take them as they are)."""
import numpy as np

F = np.float32
PI = F(3.14159265358979323846)
TWO_PI = F(6.28318530717958647692)


def wrap2pi32(x):
    """fp32 (pi + x) % (2 pi) - pi with Python's %, as the device forms it: fmodf, + 2 pi where that is negative, - pi"""
    x = np.asarray(x, F)
    r = np.fmod((PI + x).astype(F), TWO_PI).astype(F)
    r = np.where(r < 0, (r + TWO_PI).astype(F), r).astype(F)
    return (r - PI).astype(F)


def mask_bits(mask, dof):
    return np.array([bool((int(mask) >> j) & 1) for j in range(dof)])


def wrapped_delta(a, b, on):
    d = (np.asarray(b, F) - np.asarray(a, F)).astype(F)
    return np.where(on, wrap2pi32(d), d).astype(F)


def motion_samples_wrapped(qa, qb, mask, res=None, max_step=None, open_end=False, with_pre=False):
    """per edge (x [n, dof], t [n], u [dof] or None, target flags [n]) - helpers.motion_samples' tuples - for the motion
    qa -> qb along the shortest arc of the coordinates whose bit is set in `mask`; fp32, every operation rounded on its own:
        d = wrap2pi(qb - qa) on masked coordinates
        res:       x_k = wrap2pi(qa + d * (k / res))
        max_step:  L = |d| (summed in coordinate order), n = ceil(L * (1 / max_step)) interior samples
                   x_k = wrap2pi(qa + k * (d * ((1 / L) * max_step))), then the target qb as given (open_end: dropped)
    t_k the interpolation parameter along the wrapped delta, u = d / L (fp64, from the fp32 values).
    with_pre: a fifth entry, the points before their final wrap [n, dof] (the target's row: qb)."""
    out = []
    qa, qb = np.asarray(qa, F), np.asarray(qb, F)
    on = mask_bits(mask, qa.shape[1])
    for a, b in zip(qa, qb):
        d = wrapped_delta(a, b, on)
        if res is not None:
            k = np.arange(res, dtype=F)
            pre = (a[None] + (d[None] * (k / F(res))[:, None]).astype(F)).astype(F)
            p = np.where(on[None], wrap2pi32(pre), pre).astype(F)
            e = (p, k.astype(np.float64) / res, None, np.zeros(res, bool))
            out.append(e + (pre,) if with_pre else e)
            continue
        l2 = F(0)
        for v in d:
            l2 = F(l2 + F(v * v))
        L = F(np.sqrt(l2))
        steps = int(np.ceil(F(L * F(F(1) / F(max_step)))))
        frac = F(F(F(1) / L) * F(max_step)) if L > 0 else F(0)   # (L = 0: no interior sample)
        k = np.arange(steps, dtype=F)
        pre = (a[None] + (k[:, None] * (d * frac).astype(F)[None]).astype(F)).astype(F)
        p = np.where(on[None], wrap2pi32(pre), pre).astype(F)
        t = k.astype(np.float64) * max_step / float(L) if L > 0 else np.zeros(0)
        u = d.astype(np.float64) / float(L) if L > 0 else np.zeros(len(d))
        tgt = np.zeros(steps, bool)
        if not open_end:
            p = np.concatenate([p, b[None]]).astype(F)
            pre = np.concatenate([pre, b[None]]).astype(F)
            t = np.concatenate([t, [1.0]])
            tgt = np.concatenate([tgt, [True]])
        e = (p.reshape(-1, len(a)), t, u, tgt)
        out.append(e + (pre.reshape(-1, len(a)),) if with_pre else e)
    return out


def near_seam(samples_with_pre, mask, tol=1e-5):
    """per edge: some masked coordinate of a sample lies, before its wrap, within tol of an odd multiple of pi - there one ulp
    decides which end of [-pi, pi) the wrapped value takes, and a raw feature moves by 2 pi"""
    flags = []
    for p, _, _, tgt, pre in samples_with_pre:
        on = mask_bits(mask, p.shape[1])
        x = pre[~tgt][:, on].astype(np.float64)
        m = np.mod(x - np.pi, 2 * np.pi)          # distance to the nearest odd multiple of pi
        flags.append(bool((np.minimum(m, 2 * np.pi - m) <= tol).any()) if x.size else False)
    return np.array(flags, bool)


def seam_edges(q, E, seed, mask, scale=1.0):
    """E edges from the fixture's configurations with targets wrapped back into [-pi, pi) on the masked coordinates:
    qa = q_i (masked coordinates wrapped), qb = wrap2pi(qa + step), step = scale (q_j - q_i) on the plain coordinates and
    uniform in (-pi, pi) on the masked ones, so the shortest arc is the step itself.  Returns (qa, qb, crosses): crosses[e] -
    the arc passes +-pi in some masked coordinate (the straight segment qa -> qb there is longer than pi: the other way round)"""
    g = np.random.default_rng(seed)
    i, j = g.integers(0, len(q), E), g.integers(0, len(q), E)
    on = mask_bits(mask, q.shape[1])
    qa = q[i].astype(F)
    qa = np.where(on[None], wrap2pi32(qa), qa).astype(F)
    turn = g.uniform(-3.1, 3.1, qa.shape)
    step = np.where(on[None], turn, scale * (q[j] - q[i])).astype(F)
    tgt = (qa + step).astype(F)
    qb = np.where(on[None], wrap2pi32(tgt), tgt).astype(F)
    crosses = (np.abs(qb.astype(np.float64) - qa)[:, on] > np.pi).any(axis=1)
    return qa, qb, crosses


# ---------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_motion_wrap.py: plain data and the fp64 referee, importable without a GPU (the seeds below
# were chosen on the CPU: the oracle alone decides which edges are kept, and enough are)
WHEEL_ARM_URDF = """<?xml version="1.0"?>
<robot name="wheel_arm">
  <link name="base"/><link name="turret"/><link name="upper"/><link name="slide"/><link name="wheel"/>
  <joint name="yaw" type="continuous"><parent link="base"/><child link="turret"/>
    <origin xyz="0 0 0.2" rpy="0 0 0"/><axis xyz="0 0 1"/></joint>
  <joint name="shoulder" type="revolute"><parent link="turret"/><child link="upper"/>
    <origin xyz="0.1 0 0.3" rpy="0 0 0"/><axis xyz="0 1 0"/><limit lower="-1.5" upper="1.5" effort="1" velocity="1"/></joint>
  <joint name="extend" type="prismatic"><parent link="upper"/><child link="slide"/>
    <origin xyz="0.3 0 0" rpy="0 0 0"/><axis xyz="1 0 0"/><limit lower="0" upper="0.2" effort="1" velocity="1"/></joint>
  <joint name="spin" type="continuous"><parent link="slide"/><child link="wheel"/>
    <origin xyz="0.1 0 0" rpy="0 0 0"/><axis xyz="1 0 0"/></joint>
</robot>"""

# (fixture, wrap mask, margin, seed of the edges)
FIRST_HIT_CASES = [("cfg1_planar2_rq", 0b11, 0.0, 1), ("cfg4_se3_nofk_rq", 0b111000, 0.0, 1),
                   ("cfg2_baxter_rq", 0b0100101, 0.0, 1), ("cfg3_baxter_rq_c5", 0b1011010, "mixed", 1)]
COST_CASES = [("cfg1_planar2_rq", 0b11, 0.0, 1), ("cfg3_baxter_rq_c5", 0b1011010, "mixed", 1)]


def fixture_model(name):
    """(fixture, FK description, kernel, supports [S, D], weights [S, C]) of a score fixture, as the GPU tests build their model"""
    from helpers import CASE_ROBOT, case_kernel, desc_for, load
    d = load(name)
    desc = desc_for(CASE_ROBOT[name], dof=d["q"].shape[1])
    sup = d["sup_x32"].reshape(len(d["sup_x32"]), -1) if "sup_x32" in d.files and CASE_ROBOT[name] else d["sup_q"]
    sup = np.asarray(sup, dtype=F).reshape(len(sup), -1)
    return d, desc, case_kernel(d), sup, np.asarray(d["weights"], F)


def mixed_margin(d):
    """per-class margins at a high percentile of the fixture's scores: a mix of free and colliding edges"""
    C = d["score64"].shape[1]
    return np.percentile(d["score64"], 70 if C == 1 else 95, axis=0).astype(F).tolist()


def wrap_case(name, mask, margin, seed, rule, E=300, grad=False, weight=1.0, divisor=20, res=13):
    """one case of the wrapped calls: seam edges of the fixture, the rule's arguments, the referee's samples and the fp64
    oracle on them.  rule: "res", "closed" (max_step with the target) or "open" (without).  max_step = the median wrapped
    length / divisor.  A dict: qa, qb, crosses, kw, margin (a list, one per class), samples, counts, oracle (helpers.motion_oracle's
    dict), seam (near_seam's flags), model = (desc, kern, sup, W)"""
    from helpers import motion_oracle
    d, desc, kern, sup, W = fixture_model(name)
    qa, qb, crosses = seam_edges(d["q"], E, seed, mask)
    if rule == "res":
        kw = dict(res=res)
    else:
        on = mask_bits(mask, qa.shape[1])
        span = float(np.median(np.linalg.norm(wrapped_delta(qa, qb, on[None]), axis=1)))
        kw = dict(max_step=max(span / divisor, 1e-3), open_end=(rule == "open"))
    mg = mixed_margin(d) if isinstance(margin, str) else [float(margin)] * W.shape[1]
    smp = motion_samples_wrapped(qa, qb, mask, with_pre=True, **kw)
    seam = near_seam(smp, mask)
    smp = [s[:4] for s in smp]
    ref = motion_oracle(desc, kern, sup, W, smp, mg, weight=weight, grad=grad)
    return dict(qa=qa, qb=qb, crosses=crosses, kw=kw, margin=mg, samples=smp, counts=[len(s[0]) for s in smp], oracle=ref,
                seam=seam, model=(desc, kern, sup, W), fixture=d)
