"""The minimisers' trust-region loop (lt_lm.h: lm_damp, lm_step, rf_grow, lm_loop; DESIGN.md sections 19 and 28) restated
once in NumPy float64, operation by operation, with the three charts' retractions the checks rf_lm, rf_lm_terms, lc_lm
and ba_point_lm keep in front of the loop, and the free-pose bundle adjustment's ba_decide_step.  The loop takes a callback eval(p) -> (cost, g, H) -- the
product's own evaluation entry, so a replay tests the loop and not the residuals, which have their own oracles -- and
returns the final point, both costs, the iterations, the termination code and a trace with one entry per iteration, from
which `branches` derives the set of branches a solve took."""
import numpy as np

f8 = np.float64
MU0, MU_MAX, MU_MIN = f8(1e4), f8(1e16), f8(1e-32)
MIN_RATIO = f8(1e-3)
D_MIN, D_MAX = f8(1e-6), f8(1e32)
MAX_DIST = np.finfo(np.float64).max  # kMaxDist
MAX_ITER, RADIUS, ZERO_GRAD, BAD_PIVOT, BAD_MODEL, CONSTANT, EVAL_FAILED, NO_RESIDUALS = range(8)


# ---- the damped step ----
def damp(h, mu):
    """h + D^2 / mu, D = clamp(sqrt h, 1e-6, 1e32)"""
    dg = np.sqrt(f8(h))
    dg = D_MIN if dg < D_MIN else (D_MAX if dg > D_MAX else dg)
    return f8(h) + (dg * dg) / f8(mu)


def pivot_ok(v):
    return bool(v > 0.0 and v < MAX_DIST)


def step(H, g, mu):
    """(H + D^2 / mu) dl = -g by Cholesky -> (code, dl, md); dl is None after a bad pivot"""
    n = len(g)
    H = np.asarray(H, f8)
    g = np.asarray(g, f8)
    Lm = np.zeros((n, n))
    y = np.zeros(n)
    dl = np.zeros(n)
    for i in range(n):
        hii = damp(H[i, i], mu)
        for j in range(i + 1):
            s = hii if i == j else H[i, j]
            for k in range(j):
                s = s - Lm[i, k] * Lm[j, k]
            if i == j:
                if not pivot_ok(s):
                    return BAD_PIVOT, None, None
                Lm[i, i] = np.sqrt(s)
            else:
                Lm[i, j] = s / Lm[j, j]
    for i in range(n):
        s = -g[i]
        for k in range(i):
            s = s - Lm[i, k] * y[k]
        y[i] = s / Lm[i, i]
    for i in range(n - 1, -1, -1):
        s = y[i]
        for k in range(i + 1, n):
            s = s - Lm[k, i] * dl[k]
        dl[i] = s / Lm[i, i]
    gd = f8(0.0)
    dhd = f8(0.0)
    for i in range(n):
        gd = gd + g[i] * dl[i]
        hd = f8(0.0)
        for j in range(n):
            hd = hd + H[i, j] * dl[j]
        dhd = dhd + dl[i] * hd
    md = -(gd + f8(0.5) * dhd)
    if not (md > 0.0) or not (md < MAX_DIST):
        return BAD_MODEL, dl, md
    return 0, dl, md


def sums_of(H, g):
    """the sums in the order lm_step reads them: the upper triangle of H by rows, then g"""
    n = len(g)
    return np.ascontiguousarray(np.concatenate([[H[i][j] for i in range(n) for j in range(i, n)], g]), f8)


def grow_factor(ratio):
    t = f8(2.0) * f8(ratio) - f8(1.0)
    return f8(1.0) - (t * t) * t


def grow(mu, ratio):
    """the radius after an accepted step: mu / max(1/3, 1 - (2 ratio - 1)^3), capped at 1e16"""
    ff = grow_factor(ratio)
    third = f8(1.0) / f8(3.0)
    ff = third if ff < third else ff
    m = f8(mu) / ff
    return m if m < MU_MAX else MU_MAX


# ---- the charts ----
def retract_quat(q, dq):
    q0, q1, q2, q3 = (f8(x) for x in q[:4])
    r0 = ((q0 - dq[0] * q1) - dq[1] * q2) - dq[2] * q3
    r1 = ((q1 + dq[0] * q0) + dq[1] * q3) - dq[2] * q2
    r2 = ((q2 - dq[0] * q3) + dq[1] * q0) + dq[2] * q1
    r3 = ((q3 + dq[0] * q2) - dq[1] * q1) + dq[2] * q0
    nu = np.sqrt(((r0 * r0 + r1 * r1) + r2 * r2) + r3 * r3)
    return [r0 / nu, r1 / nu, r2 / nu, r3 / nu]


def retract_line(p, dl):
    """6 / 4: u+ = normalize((1, du) (x) u), w+ = normalize(w + dw (-w1, w0))"""
    w0 = p[4] - dl[3] * p[5]
    w1 = p[5] + dl[3] * p[4]
    nw = np.sqrt(w0 * w0 + w1 * w1)
    return np.array(retract_quat(p, dl) + [w0 / nw, w1 / nw], f8)


def retract_pose(p, dl):
    """7 / 6: q+ = normalize((1, dq) (x) q), t+ = t + dt"""
    return np.array(retract_quat(p, dl) + [p[4 + i] + dl[3 + i] for i in range(3)], f8)


def retract_point(p, dl):
    """3 / 4: additive; the fourth entry of the step belongs to the literal-zero column and moves nothing"""
    return np.array([p[c] + dl[c] for c in range(3)], f8)


CHARTS = {"line": (6, 4, retract_line), "pose": (7, 6, retract_pose), "point": (3, 4, retract_point)}


def normalise_q(q4):
    """lm_normalise_q: CameraPose's one normalisation"""
    q4 = np.asarray(q4, f8)
    n0 = np.sqrt((q4[0] * q4[0] + q4[2] * q4[2]) + (q4[1] * q4[1] + q4[3] * q4[3]))
    return q4 / n0 if n0 > 0.0 else q4.copy()


# ---- the loop ----
def lm_loop(chart, evaluate, p, F, max_iter, cost=None):
    """lm_loop<Chart> from the point p with the cost F -> dict(p, cost1, iterations, code, trace).  cost: the cost
    evaluation where it is not evaluate(p)[0] (a scripted group).  A trace entry:
    it, mu and nu the step was taken with, fresh (the linearisation was renewed), ratio, factor (1 - (2 ratio - 1)^3 of
    an accepted step), accepted, exit (the code that ended the solve in this iteration, or None)."""
    n_params, n_step, retract = CHARTS[chart]
    p = np.array(p, f8)
    F = f8(F)
    it, code = 0, MAX_ITER
    mu, nu = MU0, f8(2.0)
    fresh = True
    g = H = None
    trace = []
    with np.errstate(all="ignore"):
        while it < max_iter:
            e = dict(it=it, mu=mu, nu=nu, fresh=fresh, ratio=None, factor=None, accepted=None, exit=None, cost=None)
            trace.append(e)
            if fresh:
                _, g, H = evaluate(p)
                g, H = np.asarray(g, f8), np.asarray(H, f8)
                assert g.shape == (n_step,) and H.shape == (n_step, n_step)
                if all(g[c] == 0.0 for c in range(n_step)):
                    code = e["exit"] = ZERO_GRAD
                    break
                fresh = False
            rc, dl, md = step(H, g, mu)
            if rc:
                code = e["exit"] = rc
                break
            pn = retract(p, dl)
            Fn = f8(cost(pn) if cost is not None else evaluate(pn)[0])
            ratio = (F - Fn) / md
            e["ratio"], e["cost"] = ratio, Fn
            if ratio > MIN_RATIO:
                p, F = pn, Fn
                e["accepted"], e["factor"] = True, grow_factor(ratio)
                mu = grow(mu, ratio)
                nu = f8(2.0)
                fresh = True
            else:
                e["accepted"] = False
                mu = mu / nu
                nu = f8(2.0) * nu
                if mu < MU_MIN:
                    code = e["exit"] = RADIUS
                    it += 1
                    break
            it += 1
    return dict(p=p, cost1=F, iterations=it, code=code, trace=trace)


def solve(wrapper, evaluate, p0, max_iter, constant=False, n_blocks=1):
    """The wrappers' checks in their own order, then the loop -> dict(p, cost0, cost1, iterations, code, trace).
    rf_lm: constant (5), no finiteness check.  rf_lm_terms: a start that is not finite is 5 on a constant track and 6
    otherwise, then constant (5).  ba_point_lm: constant (5), then a start that is not finite (6).  lc_lm: no block (7,
    the cost is not evaluated), then a start that is not finite (6)."""
    chart = {"rf_lm": "line", "rf_lm_terms": "line", "lc_lm": "pose", "ba_point_lm": "point"}[wrapper]
    p0 = np.array(p0, f8)

    def skip(F, code):
        return dict(p=p0, cost0=F, cost1=F, iterations=0, code=code, trace=[])
    if wrapper == "lc_lm" and n_blocks <= 0:
        return skip(f8(0.0), NO_RESIDUALS)
    F = f8(evaluate(p0)[0])
    finite = bool(F <= MAX_DIST)
    if wrapper == "rf_lm":
        if constant:
            return skip(F, CONSTANT)
    elif wrapper == "rf_lm_terms":
        if not finite:
            return skip(F, CONSTANT if constant else EVAL_FAILED)
        if constant:
            return skip(F, CONSTANT)
    elif wrapper == "ba_point_lm":
        if constant:
            return skip(F, CONSTANT)
        if not finite:
            return skip(F, EVAL_FAILED)
    elif not finite:
        return skip(F, EVAL_FAILED)
    r = lm_loop(chart, evaluate, p0, F, max_iter)
    r["cost0"] = F
    return r


def branches(r, max_iter):
    """the branch set of a solve, from its trace, its code and its start cost"""
    t, code, out = r["trace"], r["code"], set()
    if code in (CONSTANT, EVAL_FAILED, NO_RESIDUALS):
        return {f"code{code}"}
    if max_iter == 0:
        out.add("max_iter_0")
    if max_iter == 1:
        out.add("max_iter_1")
    accepted_before = False
    run = 0
    for k, e in enumerate(t):
        where = "after_accept" if accepted_before else ("at_0" if k == 0 else "after_rejections")
        if e["exit"] == ZERO_GRAD:
            out.add("zero_gradient_" + where)
        elif e["exit"] == BAD_PIVOT:
            if accepted_before:
                out.add("bad_pivot_after_accept")
            else:
                out.add("bad_pivot_at_0_finite_start" if r["cost0"] <= MAX_DIST else "bad_pivot_at_0_start_not_finite")
        elif e["exit"] == BAD_MODEL:
            out.add("bad_model_" + where)
        if e["accepted"] is True:
            out.add("accept")
            if k > 0 and t[k - 1]["accepted"] is False:
                assert k + 1 >= len(t) or t[k + 1]["nu"] == 2.0
                out.add("reject_then_accept")
            out.add("grow_floor" if e["factor"] < f8(1.0) / f8(3.0) else "grow_above_floor")
            if grow(e["mu"], e["ratio"]) == MU_MAX:
                out.add("radius_cap")
            accepted_before = True
            run = 0
        elif e["accepted"] is False:
            run += 1
            if run >= 3:
                out.add("three_rejections")
            if not (e["cost"] <= MAX_DIST):
                out.add("reject_cost_not_finite")
        if e["exit"] == RADIUS:
            out.add("radius_exit")
            out.add("radius_exit_on_cap" if r["iterations"] == max_iter else
                    ("radius_exit_one_before_cap" if r["iterations"] == max_iter - 1 else "radius_exit_early"))
    if code == MAX_ITER and t:
        out.add("cap_after_accept" if t[-1]["accepted"] else "cap_after_reject")
    return out


# ---- the free-pose bundle adjustment's decision (lt_ba.h: ba_decide_init, ba_decide_step), its own copy of the
# accept / reject logic over the same rf_grow ----
def ba_decide_init(total, max_iter):
    F = f8(0.5) * f8(total)
    st = dict(F=F, F0=F, mu=MU0, nu=f8(2.0), fresh=1, iters=0, bad=0, done=0, code=MAX_ITER, max_iter=max_iter)
    if not (F <= MAX_DIST):
        st["done"], st["code"] = 1, EVAL_FAILED
    elif max_iter <= 0:
        st["done"] = 1
    return st


def ba_decide_step(st, total, md_total):
    """after an attempt: a failed factorisation (st["bad"]) or a model decrease that is not positive and finite is a
    rejected step -> accepted or not"""
    with np.errstate(all="ignore"):
        Fn, md = f8(0.5) * f8(total), -f8(md_total)
        accept, ratio = False, f8(0.0)
        if not st["bad"] and md > 0.0 and md < MAX_DIST:
            ratio = (st["F"] - Fn) / md
            accept = bool(ratio > MIN_RATIO)
        st["iters"] += 1
        st["bad"] = 0
        if accept:
            st["F"] = Fn
            st["mu"] = grow(st["mu"], ratio)
            st["nu"] = f8(2.0)
            st["fresh"] = 1
        else:
            st["fresh"] = 0
            st["mu"] = st["mu"] / st["nu"]
            st["nu"] = f8(2.0) * st["nu"]
            if st["mu"] < MU_MIN:
                st["done"], st["code"] = 1, RADIUS
                return accept
        if st["iters"] >= st["max_iter"]:
            st["done"], st["code"] = 1, MAX_ITER
    return accept
