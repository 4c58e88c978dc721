"""The global point-line association on the host: lt_fn_assoc_eval against the NumPy restatement
in longdouble, the linear solve (lt_fn_assoc_pcg) against a dense longdouble solve and against a straight NumPy loop in
the defined orders, the loop's decisions against lm_oracle's restated ba_decide_*, the cost against scipy, what the solve
means on a structured scene, SetUp and the containers against straight restatements of upstream, and determinism.  No
GPU: everything here runs lt_fn_assoc_host, the twin the device is held to bit for bit (tests/test_gpu_assoc.py)."""
import glob
import os

import numpy as np
import pytest

import assoc_oracle as ao
import assoc_scenes as sc
import lm_oracle as lo
from limap_amd import optimize, structures, vplib
from limap_amd.base import CameraView, ImageCollection, Line2d, Line3d, LineTrack, PointTrack

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "assoc")
GOLDEN_IN = ("img_ids", "k", "q", "t", "p3", "poff", "pimg", "pxy", "line6", "loff", "limg", "l2d", "l3d", "vp3", "edge_kind",
             "edge_a", "edge_b", "edge_w")
SMALL = [dict(), dict(parallel=True), dict(orth_exact=True), dict(identical=True)]


def small_scenes():
    return [sc.small_scene(seed, n_cams=n, **kw) for (seed, n), kw in zip(((0, 4), (1, 3), (2, 5), (3, 4)), SMALL)]


# ---- 1. evaluation ----
def test_eval_against_longdouble_restatement():
    """E_ref: the FP64 restatement's own maximum error against its longdouble evaluation, per quantity relative to the
    larger of 1 and the quantity's largest magnitude in the scene; ours must stay within 4 E_ref.  Measured (DESIGN
    section 29): the figures this test prints."""
    names = ("res_blk", "res_edge", "cost", "g4", "diag", "off")
    E = {k: 0.0 for k in names}
    Eref = dict(E)
    for s in small_scenes():
        kw = dict(lw_vp_collinearity=0.5)
        ours = sc.evaluate(s, sc.cfg_of(**kw))
        f64, ld = ao.evaluate(s, dtype=np.float64, **kw), ao.evaluate(s, dtype=np.longdouble, **kw)
        assert list(ours["nd"]) == ld["nd"] and np.array_equal(ours["sp"], ld["sp"])
        assert [tuple(e) for e in ours["edge_info"]] == [e[:3] for e in ld["edges"]]
        assert np.array_equal(ours["edge_w"], [e[3] for e in ld["edges"]])
        for nm in names:
            scale = max(float(np.abs(ld[nm]).max()), 1.0)
            E[nm] = max(E[nm], float(np.abs(ours[nm] - ld[nm]).max()) / scale)
            Eref[nm] = max(Eref[nm], float(np.abs(f64[nm] - ld[nm]).max()) / scale)
    print("assoc eval error, ours:", E, "restatement:", Eref)
    for nm in names:
        assert E[nm] <= 4 * Eref[nm], (nm, E[nm], Eref[nm])


def test_eval_scene_has_the_named_cases():
    s = sc.small_scene(0, parallel=True, orth_exact=True, identical=True)
    ev = sc.evaluate(s, sc.cfg_of(lw_vp_collinearity=0.5))
    NP, NL = 8, 4
    info = [tuple(e) for e in ev["edge_info"]]
    assert sum(1 for k, a, b in info if k == 0 and a == 0) == 2                   # a junction
    assert {k for k, a, b in info if b == NP + 1} == {0, 1}                       # a line tied to points and a VP
    assert ev["nd"][7] == 3 and all(7 not in (a, b) for _, a, b in info)          # a point with no edge (R1.1 keeps it free)
    assert ev["nd"][NP + NL + 2] == 0                                             # a VP with no edge is no parameter
    e_par = info.index((1, NP + NL, NP))
    assert ev["res_edge"][e_par, 0] == 1e-6                                       # parallel: sqrt(EPS)
    e_orth = next(i for i, (k, a, b) in enumerate(info) if k == 2 and a > NP + NL + 2)
    assert ev["res_edge"][e_orth, 0] == 0.0
    e_col = next(i for i, (k, a, b) in enumerate(info) if k == 3)
    assert ev["res_edge"][e_col, 0] == 1e-6


# ---- 2. the linear solve ----
def _solve_ld(A, b):
    """Gaussian elimination with partial pivoting in longdouble"""
    A = np.array(A, np.longdouble); b = np.array(b, np.longdouble)
    n = len(b)
    for k in range(n):
        piv = k + int(np.argmax(np.abs(A[k:, k])))
        if piv != k:
            A[[k, piv]] = A[[piv, k]]; b[[k, piv]] = b[[piv, k]]
        f = A[k + 1:, k] / A[k, k]
        A[k + 1:] -= f[:, None] * A[k]
        b[k + 1:] -= f * b[k]
    x = np.zeros(n, np.longdouble)
    for k in range(n - 1, -1, -1):
        x[k] = (b[k] - A[k, k + 1:] @ x[k + 1:]) / A[k, k]
    return x


def damped_system(ev, mu):
    """from lt_fn_assoc_eval's blocks: the damped diagonal blocks, and the dense system over the free slots"""
    nd = [int(x) for x in ev["nd"]]
    diag = ev["diag"].copy()
    for u, n in enumerate(nd):
        for i in range(n):
            diag[u, i, i] = ao.damp(diag[u, i, i], mu)
    NU = len(nd)
    A = np.zeros((4 * NU, 4 * NU))
    for u in range(NU):
        A[4 * u:4 * u + 4, 4 * u:4 * u + 4] = diag[u]
    for (k, a, b), E in zip(ev["edge_info"], ev["off"]):
        A[4 * a:4 * a + 4, 4 * b:4 * b + 4] += E
        A[4 * b:4 * b + 4, 4 * a:4 * a + 4] += E.T
    fs = ao.free_slots(nd)
    return nd, diag, A[np.ix_(fs, fs)], -ev["g4"].reshape(-1)[fs], fs


def test_pcg_step_equals_dense_normal_equations():
    """eta tiny, the cap large: the step against a dense longdouble solve of the damped normal equations.  Bound: 4 times
    the error of numpy.linalg.solve in float64, relative to the larger of 1 and the largest step entry.
    Measured: PCG / dense FP64 errors per scene 3.2e-16 / 1.6e-13, 1.1e-17 / 2.6e-15, 1.0e-16 / 4.7e-15,
    5.3e-17 / 3.3e-14 after 13, 5, 12 and 13 CG iterations.  With x, r and A p in plain doubles the same recurrence gave
    5.6e-13, 2.2e-14, 4.0e-14 and 2.9e-14 and missed the bound on the second and third scene: that is why they are pairs."""
    figures = []
    for s in small_scenes():
        ev = sc.evaluate(s, sc.cfg_of(lw_vp_collinearity=0.5))
        nd, diag, A, b, fs = damped_system(ev, 1e4)
        rc, x, it, end, _ = sc.pcg(nd, diag, ev["edge_info"][:, 1], ev["edge_info"][:, 2], ev["off"], -ev["g4"], 1e-15, 5000)
        assert rc == 0 and end == 0, (it, end)
        ref = _solve_ld(A, b)
        scale = max(1.0, float(np.abs(ref).max()))
        e_ref = float(np.abs(np.linalg.solve(A, b) - ref).max()) / scale
        e_ours = float(np.abs(x.reshape(-1)[fs] - ref).max()) / scale
        figures.append((e_ours, e_ref, it))
    print("assoc step error per scene (PCG, dense FP64 solve, CG iterations):", figures)
    for e_ours, e_ref, it in figures:
        assert e_ours <= 4 * e_ref, figures


def test_pcg_default_eta_meets_its_stop_rule():
    """at the default eta the true preconditioned residual of the returned step, recomputed in longdouble, is bounded by
    eta |r0| plus four times the drift a float64 NumPy run of the same recurrence shows against its own recomputation"""
    eta = 0.1
    for s in small_scenes():
        ev = sc.evaluate(s, sc.cfg_of(lw_vp_collinearity=0.5))
        nd, diag, A, b, fs = damped_system(ev, 1e4)
        ea, eb = ev["edge_info"][:, 1], ev["edge_info"][:, 2]
        rc, x, it, end, rz = sc.pcg(nd, diag, ea, eb, ev["off"], -ev["g4"], eta, 500)
        assert rc == 0 and end == 0
        # the preconditioner over the free slots: the inverse of the damped diagonal blocks
        M = np.zeros_like(A)
        pos = {int(f): i for i, f in enumerate(fs)}
        for u, n in enumerate(nd):
            if n:
                ii = [pos[4 * u + i] for i in range(n)]
                M[np.ix_(ii, ii)] = np.linalg.inv(diag[u][:n, :n])

        def pre_norm(xv):
            r = np.array(b, np.longdouble) - np.array(A, np.longdouble) @ np.array(xv, np.longdouble)
            return float(np.sqrt(r @ (np.array(M, np.longdouble) @ r)))
        xr, itr, endr = ao.pcg_loop(nd, diag, ea, eb, ev["off"], -ev["g4"], eta, 500)
        # the drift of the recurrence: its own r.z at the end against the recomputed one
        drift = abs(pre_norm(xr.reshape(-1)[fs]) - float(np.sqrt(rz[1])))
        r0 = pre_norm(np.zeros(len(fs)))
        true = pre_norm(x.reshape(-1)[fs])
        print("assoc PCG at eta 0.1: iterations", it, "true residual", true, "eta |r0|", eta * r0, "drift", drift)
        assert true <= eta * r0 + 4 * drift, (true, eta * r0, drift)


def random_system(n, seed, n_edges=None, spd=True):
    rng = np.random.default_rng(seed)
    nd = rng.integers(0, 5, n).astype(np.int32)
    nd[0] = 4
    n_edges = min(3 * n, 600) if n_edges is None else n_edges
    ea = rng.integers(0, n, n_edges)
    eb = (ea + 1 + rng.integers(0, max(n - 1, 1), n_edges)) % n
    keep = ea != eb
    ea, eb = ea[keep].astype(np.int32), eb[keep].astype(np.int32)
    off = rng.normal(size=(len(ea), 4, 4)) * 0.2
    diag = np.zeros((n, 4, 4))
    for u in range(n):
        B = rng.normal(size=(4, 6))
        diag[u] = B @ B.T + (2.0 + 0.8 * np.sum((ea == u) | (eb == u))) * np.eye(4)
    return nd, diag, ea, eb, off, rng.normal(size=(n, 4))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 64 * 256 + 3])
def test_pcg_is_the_defined_recurrence(n):
    """bit-identical to a straight NumPy loop in the defined orders, at unknown counts around a chunk and above the 64
    chunks one wave sums"""
    big = n > 1000
    nd, diag, ea, eb, off, rhs = random_system(n, n, n_edges=0 if n == 1 else (300 if big else None))
    cap = 4 if big else 40
    rc, x, it, end, _ = sc.pcg(nd, diag, ea, eb, off, rhs, 1e-8, cap)
    xr, itr, endr = ao.pcg_loop(list(nd), diag, ea, eb, off, rhs, 1e-8, cap)
    assert rc == 0 and (it, end) == (itr, endr) and it >= (1 if n == 1 else 3)
    assert np.array_equal(x, xr)
    assert np.all(x[np.arange(4)[None, :] >= nd[:, None]] == 0.0)  # the slots outside an unknown's dimensions


def test_pcg_breakdown_and_bad_pivot_are_reported():
    nd, diag, ea, eb, off, rhs = random_system(12, 5)
    off = off * 60.0  # the off-diagonal blocks dominate: the matrix is indefinite
    rc, x, it, end, _ = sc.pcg(nd, diag, ea, eb, off, rhs, 1e-12, 200)
    assert rc == 0 and end == 2
    assert ao.pcg_loop(list(nd), diag, ea, eb, off, rhs, 1e-12, 200)[2] == 2
    diag[0, 1, 1] = -1.0
    rc, x, it, end, _ = sc.pcg(nd, diag, ea, eb, off / 60.0, rhs, 1e-12, 200)
    assert rc == 0 and end == 3 and it == 0 and not x.any()


def failing_solves():
    """(name, scene, configuration): a linear solve that fails inside the loop on finite input.  breakdown: r0.z0 is finite
    and positive, the products of A p are not (k_as_alpha); pivot: a diagonal block's sums overflow (k_as_precond)"""
    return [("breakdown", sc.structured_scene(n_cams=4, seed=5), dict(sc.BREAKDOWN, max_num_iterations=20)),
            ("pivot", sc.pivot_scene(), dict(sc.PIVOT, max_num_iterations=20))]


@pytest.mark.parametrize("name", ["breakdown", "pivot"])
def test_a_failed_linear_solve_is_a_rejected_step(name):
    """every attempt's linear solve fails: the trace carries bad = 1, the point and the cost stay, the radius shrinks as
    after a rejected step (mu / nu, nu doubling) without a new linearisation, the radius ends the solve (code 1), and the
    restated decisions with the bad flags give the same radii, iterations, code and cost"""
    _, s, kw = next(c for c in failing_solves() if c[0] == name)
    ev = sc.evaluate(s, sc.cfg_of(**kw))
    if name == "pivot":
        assert np.isinf(ev["diag"]).any() and ev["cost"] == 0.0 and not ev["g4"].any()
    else:  # the start of the solve is sound and its first product is not: the failure is k_as_alpha's
        nd, diag, _, _, _ = damped_system(ev, 1e4)
        rc, x, it, end, rz = sc.pcg(nd, diag, ev["edge_info"][:, 1], ev["edge_info"][:, 2], ev["off"], -ev["g4"], 0.1, 500)
        assert rc == 0 and (it, end) == (0, 2) and 0.0 < rz[0] < np.inf and not x.any()
    rc, o, tr = sc.run_host(s, sc.cfg_of(**kw), 2, trace=64)
    rec = tr["rec"]
    assert rc == 0 and tr["n"] == len(rec) == 15 and np.all(rec[:, 1] == 1) and not rec[:, 5].any()
    assert (int(o["iterations"][0]), int(o["code"][0]), int(o["cg_iterations"][0])) == (15, 1, 0)
    assert o["cost"][0] == o["cost"][1] == ev["cost"]
    NP, NL = len(s["p3"]), len(s["line6"])
    assert np.array_equal(o["points"], ev["sp"][:NP, :3]) and np.array_equal(o["params"], ev["sp"][NP:NP + NL])
    assert np.array_equal(o["vps"], ev["sp"][NP + NL:, :3])
    assert list(rec[:, 2]) == [1.0] + [0.0] * 14  # fresh only once
    mu, nu = 1e4, 2.0
    for k in range(15):
        assert rec[k, 0] == mu
        mu, nu = mu / nu, 2.0 * nu
    assert mu < 1e-32
    st = lo.ba_decide_init(tr["total0"], kw["max_num_iterations"])
    for m, bad, fresh, total, md, cg in rec:
        assert not st["done"] and (st["mu"], st["fresh"]) == (m, int(fresh))
        st["bad"] = int(bad)
        assert lo.ba_decide_step(st, total, md) is False
    assert st["done"] and (st["iters"], st["code"]) == (15, 1) and st["F"] == st["F0"] == o["cost"][0]


# ---- 3. the loop ----
@pytest.mark.parametrize("name", ["small", "structured", "rejections", "zero_gradient"])
def test_loop_follows_the_restated_decisions(name):
    """every attempt hands (failed linear solve, cost total, model-decrease total) to ba_decide_step; the restated
    decisions on those values give the twin's radius and linearisation flag before every attempt, and its iterations,
    code and final cost"""
    s, kw = {"small": (sc.small_scene(0), dict(max_num_iterations=40)),
             "structured": (sc.structured_scene(n_cams=5, seed=3), dict(max_num_iterations=40)),
             "rejections": (sc.structured_scene(n_cams=4, seed=6, struct_sigma=0.2, vp_sigma=0.3),
                            dict(max_num_iterations=30, cg_max_iterations=1, cg_eta=1e-12)),
             "zero_gradient": (sc.stationary_vp_scene(), dict(sc.STATIONARY))}[name]
    rc, o, tr = sc.run_host(s, sc.cfg_of(**kw), 2, trace=256)
    assert rc == 0 and tr["n"] <= 256
    st = lo.ba_decide_init(tr["total0"], kw.get("max_num_iterations", 100))
    for mu, bad, fresh, total, md, cg in tr["rec"]:
        assert not st["done"] and (st["mu"], st["fresh"]) == (mu, int(fresh))
        if bad < 0:
            st["done"], st["code"] = 1, lo.ZERO_GRAD
            continue
        st["bad"] = int(bad)
        lo.ba_decide_step(st, total, md)
    assert st["done"] and (st["iters"], st["code"]) == (int(o["iterations"][0]), int(o["code"][0]))
    assert st["F0"] == o["cost"][0] and st["F"] == o["cost"][1]
    assert int(tr["rec"][:, 5].sum()) == int(o["cg_iterations"][0])
    if name == "zero_gradient":
        assert o["code"][0] == 2 and o["iterations"][0] == 0


def test_codes_2_6_7_are_reached():
    s = sc.structured_scene(n_cams=4, seed=5)
    z = sc.stationary_vp_scene()
    rc, o = sc.run_host(z, sc.cfg_of(**sc.STATIONARY))
    assert rc == 0 and o["code"][0] == 2 and o["iterations"][0] == 0 and np.array_equal(o["points"], z["p3"]) and np.array_equal(o["vps"], z["vp3"])
    rc, o = sc.run_host(s, sc.cfg_of(constant_point=1, constant_line=1, constant_vp=1))  # SetUp adds nothing at all
    assert rc == 0 and o["code"][0] == 7
    rc, o = sc.run_host(s, sc.cfg_of(constant_point=1, constant_line=1, enable_vpline=0))
    assert rc == 0 and o["code"][0] == 7 and o["iterations"][0] == 0
    bad = sc.depth_zero_scene()
    rc, o = sc.run_host(bad, sc.cfg_of(max_num_iterations=5))
    assert rc == 0 and o["code"][0] == 6 and o["iterations"][0] == 0 and np.array_equal(o["points"], bad["p3"])


def test_minimises_the_restated_cost():
    """The cost sequence over iteration caps never rises, and scipy.optimize.least_squares on the restated cost in the
    same charts, from the same start and from the solution's neighbourhood, finds nothing lower than ours beyond 10 x
    its own spread between its two starts (section 27 check 3's rule).  Measured: the figures this
    test prints."""
    from scipy.optimize import least_squares
    s = sc.structured_scene(n_cams=4, seed=1)
    seq = []
    for it in range(0, 26):
        rc, o = sc.run_host(s, sc.cfg_of(max_num_iterations=it), 1)
        assert rc == 0 and o["iterations"][0] == it
        seq.append(float(o["cost"][1]))
    assert seq[0] == float(o["cost"][0]) and all(b <= a for a, b in zip(seq, seq[1:])), seq
    rc, o = sc.run_host(s, sc.cfg_of(max_num_iterations=400, cg_eta=1e-3), 1)
    ours = float(o["cost"][1])
    pk = ao.Packed(s)
    sp0 = ao.start_params(s, pk.nd)
    assert abs(pk.cost(sp0) - float(o["cost"][0])) <= 1e-9 * float(o["cost"][0])  # the same cost at the same start
    sp1 = sp0.copy()  # the second start: ours
    NP, NL = len(s["p3"]), len(s["line6"])
    sp1[:NP, :3], sp1[NP:NP + NL], sp1[NP + NL:, :3] = o["points"], o["params"], o["vps"]
    assert abs(pk.cost(sp1) - ours) <= 1e-9 * max(ours, 1.0)
    n = int(pk.off[-1])
    sol = [least_squares(lambda y, b=base: pk.residuals(pk.point(b, y)), np.zeros(n), method="trf", xtol=1e-15, ftol=1e-15,
                         gtol=1e-15, max_nfev=300) for base in (sp0, sp1)]
    cs = [float(r.cost) for r in sol]
    spread = abs(cs[0] - cs[1])
    print("assoc cost: start", seq[0], "ours", ours, "scipy from the start / from ours", cs, "spread", spread)
    assert ours - min(cs) <= 10 * spread + 1e-9 * ours, (ours, cs)


# ---- 4. what the solve means ----
def scene_metrics(s, points, params, vps):
    import refine_oracle as ro
    d_pl, a_vl = [], []
    dirs = []
    for pp in params:
        d, m = ro.plucker(list(pp[:4]), list(pp[4:]), np.float64)
        dirs.append((np.array(d), np.array(m)))
    for p, n in s["incidences"]:
        d, m = dirs[n]
        d_pl.append(np.linalg.norm(np.cross(d, points[p]) + m) / np.linalg.norm(d))
    for n, c in enumerate(s["line_class"]):
        cs = min(abs(float(dirs[n][0] @ vps[c])) / (np.linalg.norm(dirs[n][0]) * np.linalg.norm(vps[c])), 1.0)
        a_vl.append(np.degrees(np.arccos(cs)))
    orth = [abs(float(vps[a] @ vps[b])) / (np.linalg.norm(vps[a]) * np.linalg.norm(vps[b])) for a, b in ((0, 1), (0, 2), (1, 2))]
    return float(np.mean(d_pl)), float(np.mean(a_vl)), float(np.mean(orth))


def test_solve_pulls_the_associations_together():
    import refine_oracle as ro
    s = sc.structured_scene(n_cams=5, lines_per_dir=3, points_per_line=2, seed=11, noise_px=0.5)
    rc, o = sc.run_host(s, sc.cfg_of(max_num_iterations=60))
    assert rc == 0
    before = scene_metrics(s, s["p3"], np.array([ro.minimal(l) for l in s["line6"]]), s["vp3"])
    after = scene_metrics(s, o["points"], o["params"], o["vps"])
    print("assoc meaning (mean point-line distance, mean line-VP angle, mean |cos| between VPs): before", before, "after", after)
    assert all(a < b for a, b in zip(after, before)), (before, after)


# ---- the Python surface on a scene: tracks, 2D bipartites, VP tracks ----
def associator_of(s, host_threads=2, cfg=None, **kw):
    """a GlobalAssociator over the scene: the 2D bipartites carry the scene's incidences and direction classes as edges
    (every support a keypoint on its line, every line's 2D VP that of its class)"""
    ids = [int(i) for i in s["img_ids"]]
    imagecols = ImageCollection({i: CameraView(s["k"][n], s["q"][n], s["t"][n]) for n, i in enumerate(ids)})
    NP, NL = len(s["p3"]), len(s["line6"])
    ptracks, ltracks = {}, {}
    for n in range(NP):
        a, b = int(s["poff"][n]), int(s["poff"][n + 1])
        ptracks[10 + n] = PointTrack(s["p3"][n], [int(x) for x in s["pimg"][a:b]], [n] * (b - a), [s["pxy"][i] for i in range(a, b)])
    for n in range(NL):
        a, b = int(s["loff"][n]), int(s["loff"][n + 1])
        t = LineTrack(Line3d(s["line6"][n, :3], s["line6"][n, 3:]), [int(x) for x in s["limg"][a:b]], [n] * (b - a),
                      [Line2d(s["l2d"][i, :2], s["l2d"][i, 2:]) for i in range(a, b)])
        t.line3d_list = [Line3d(s["l3d"][i, :3], s["l3d"][i, 3:]) for i in range(a, b)]
        ltracks[20 + n] = t
    bpts, bpts_vp = {}, {}
    for i in ids:
        b2, bv = structures.PL_Bipartite2d(), structures.VPLine_Bipartite2d()
        for n in range(NL):
            for j in range(int(s["loff"][n]), int(s["loff"][n + 1])):
                if int(s["limg"][j]) == i:
                    b2.add_line(s["l2d"][j].reshape(2, 2), n)
                    bv.add_line(Line2d(s["l2d"][j, :2], s["l2d"][j, 2:]), n)
        cam = ids.index(i)
        for c in range(len(s["vp3"])):
            bv.add_point(structures.VP2d(sc.bs.quat_to_rot(s["q"][cam]) @ s["vp3"][c], c), c)
        for n in range(NL):
            if bv.exist_line(n):
                bv.add_edge(int(s["line_class"][n]), n)
        for n in range(NP):
            for j in range(int(s["poff"][n]), int(s["poff"][n + 1])):
                if int(s["pimg"][j]) == i:
                    b2.add_point(structures.Point2d(s["pxy"][j], 10 + n), n)
        for p, n in s["incidences"]:
            if b2.exist_line(n) and b2.exist_point(p):
                b2.add_edge(p, n)
        bpts[i], bpts_vp[i] = b2, bv
    c = dict(constant_intrinsics=True, constant_pose=True, min_num_images=4, th_pixel=6.0)
    c.update(cfg or {})
    c.update(kw)
    A = optimize.GlobalAssociator(optimize.GlobalAssociatorConfig(c), host_threads=host_threads)
    A.InitImagecols(imagecols); A.InitPointTracks(ptracks); A.InitLineTracks(ltracks)
    A.Init2DBipartites_PointLine(bpts)
    A.InitVPTracks([vplib.VPTrack(v, [(i, c) for i in ids]) for c, v in enumerate(s["vp3"])])
    A.Init2DBipartites_VPLine(bpts_vp)
    A.SetUp()
    A.Solve()
    return A


def test_associator_recovers_incidences_and_direction_classes():
    s = sc.structured_scene(n_cams=5, lines_per_dir=3, points_per_line=2, seed=11, noise_px=0.5, count=5)
    A = associator_of(s, max_num_iterations=60)
    r = A.result()
    assert r["code"] in (0, 1, 2) and r["cost"][1] < r["cost"][0]
    # SetUp handed over exactly the scene's edges, so the arrays-level solve is the same solve
    rc, o = sc.run_host(s, sc.cfg_of(max_num_iterations=60), 2)
    assert np.array_equal(o["points"], r["points"]) and np.array_equal(o["vps"], r["vps"]) and np.array_equal(o["params"], r["params"])
    bpt = A.GetBipartite3d_PointLine()
    got = sorted((p - 10, n - 20) for p in bpt.get_point_ids() for n in bpt.neighbor_lines(p))
    assert got == sorted(s["incidences"])
    assert sorted((p - 10, n - 20) for p in bpt.get_point_ids() for n in A.GetBipartite3d_PointLine_Constraints().neighbor_lines(p)) == got
    bv = A.GetBipartite3d_VPLine()
    assert sorted((v, n - 20) for v in bv.get_point_ids() for n in bv.neighbor_lines(v)) == sorted((int(c), n) for n, c in enumerate(s["line_class"]))
    # the restatement alone recovers them too: every generated pair passes both hard gates on the restated geometry of
    # the solved point (the infinite line of the solved parameters; the uncertainty of the input point's smallest depth)
    import refine_oracle as ro
    cfg = A.config_
    for p, n in s["incidences"]:
        d, m = [np.array(v) for v in ro.plucker(list(r["params"][n][:4]), list(r["params"][n][4:]), np.float64)]
        dist = np.linalg.norm(np.cross(d, r["points"][p]) + m) / np.linalg.norm(d)
        a, b = int(s["poff"][p]), int(s["poff"][p + 1])
        unc = min((sc.bs.quat_to_rot(s["q"][c]) @ s["p3"][p] + s["t"][c])[2] / ((s["k"][c][0] + s["k"][c][1]) / 2.0)
                  for c in (list(s["img_ids"]).index(i) for i in s["pimg"][a:b]))
        assert dist <= cfg.th_hard_pl_dist3d * unc, (p, n, dist, unc)
    for n, c in enumerate(s["line_class"]):
        d, _ = ro.plucker(list(r["params"][n][:4]), list(r["params"][n][4:]), np.float64)
        d = np.array(d)
        cs = min(abs(float(d @ r["vps"][c])) / (np.linalg.norm(d) * np.linalg.norm(r["vps"][c])), 1.0)
        assert np.degrees(np.arccos(cs)) <= cfg.th_hard_vpline_angle3d, (n, c)
        others = [np.degrees(np.arccos(min(abs(float(d @ r["vps"][o])) / np.linalg.norm(d), 1.0))) for o in range(3) if o != c]
        assert min(others) > cfg.th_hard_vpline_angle3d  # and no other class would pass
    # dict round trips of the outputs
    assert structures.PL_Bipartite3d(bpt.as_dict()).as_dict().keys() == bpt.as_dict().keys()
    again = structures.VPLine_Bipartite3d(bv.as_dict())
    assert again.get_point_ids() == bv.get_point_ids() and again.count_edges() == bv.count_edges()
    t = vplib.VPTrack(A.GetOutputVPTracks()[0].as_dict())
    assert np.array_equal(t.direction, A.GetOutputVPs()[0]) and t.length() == 5


# ---- 5. set-up ----
SWITCHES = [dict(), dict(constant_point=1), dict(constant_line=1), dict(constant_vp=1), dict(constant_point=1, constant_line=1),
            dict(constant_line=1, constant_vp=1), dict(constant_point=1, constant_vp=1),
            dict(constant_point=1, constant_line=1, constant_vp=1), dict(enable_pointline=0), dict(enable_vpline=0),
            dict(enable_pointline=0, enable_vpline=0), dict(lw_point=0.0), dict(lw_point=-1.0), dict(lw_pointline_association=0.0),
            dict(lw_vpline_association=0.0), dict(lw_vp_orthogonality=0.0), dict(lw_vp_collinearity=0.7), dict(min_num_images=5)]


@pytest.mark.parametrize("kw", SWITCHES, ids=str)
def test_setup_switches(kw):
    s = sc.small_scene(0, identical=True)
    ev = sc.evaluate(s, sc.cfg_of(**kw))
    blks, edges, nd = ao.setup(s, **{k: (bool(v) if isinstance(v, int) and k != "min_num_images" else v) for k, v in kw.items()})
    assert int(ev["dims"][4]) == len(blks) and int(ev["dims"][5]) == len(edges), (ev["dims"], len(blks), len(edges))
    assert list(ev["nd"]) == nd
    assert [tuple(e) for e in ev["edge_info"]] == [e[:3] for e in edges] and np.array_equal(ev["edge_w"], [e[3] for e in edges])
    assert list(ev["blk_unk"]) == [b["s"] for b in blks]


def test_weight_thresholds_best_vp_tie_and_zero_vps():
    s = sc.structured_scene(n_cams=5, lines_per_dir=1, points_per_line=1, seed=2, junction=False)
    # construct_weights_pointline: 5 supports per edge within th_pixel
    for th, n in ((4.0, 3), (5.0, 3), (6.0, 0)):
        A = associator_of(s, max_num_iterations=0, th_weight_pointline=th)
        assert len(A.construct_weights_pointline(th)) == n, th
        assert all(w == 5.0 for w in A.construct_weights_pointline(th).values())
    A = associator_of(s, max_num_iterations=0, th_pixel=1e-9)
    assert A.construct_weights_pointline(3.0) == {} and A.construct_weights_pointline(0.0) != {}
    for th, n in ((4, 3), (5, 3), (6, 0)):
        assert len(associator_of(s, max_num_iterations=0, th_count_vpline=th).construct_weights_vpline(th)) == n, th
    # the best VP of a line: ties go to the smaller VP id
    ids = [int(i) for i in s["img_ids"]]
    for i in ids[:2]:
        A.all_bpt2ds_vp_[i].delete_edge(0, 0)
        A.all_bpt2ds_vp_[i].add_edge(2, 0)
    w = A.construct_weights_vpline(1)
    assert w[(0, 20)] == 3 and (2, 20) not in w
    A.all_bpt2ds_vp_[ids[2]].delete_edge(0, 0)  # 2 : 2 of the remaining four
    A.all_bpt2ds_vp_[ids[2]].add_point(structures.VP2d([0, 0, 1], -1), 9)
    A.all_bpt2ds_vp_[ids[2]].add_edge(9, 0)
    w = A.construct_weights_vpline(1)
    assert w[(0, 20)] == 2 and (2, 20) not in w
    # angle gates (kept away from the thresholds) and zero VPs
    assert A.construct_pairs_vp_orthogonality(80.0) == [(0, 1), (0, 2), (1, 2)] and A.construct_pairs_vp_collinearity(1.0) == []
    assert A.construct_pairs_vp_orthogonality(89.99) != [(0, 1), (0, 2), (1, 2)] and len(A.construct_pairs_vp_collinearity(95.0)) == 3
    A.InitVPTracks([])
    for b in A.all_bpt2ds_vp_.values():
        b.clear_edges()
    assert A.construct_pairs_vp_orthogonality(87.0) == [] and A.construct_pairs_vp_collinearity(1.0) == []
    A.SetUp()
    assert A.Solve() and len(A.GetOutputVPs()) == 0


def test_merge_vp_tracks_by_direction():
    def tr(d, sup):
        d = np.asarray(d, float)
        return vplib.VPTrack(d / np.linalg.norm(d), sup)
    a, b = tr([1, 0, 0], [(0, 0), (1, 0), (2, 1)]), tr([1, 0.005, 0], [(3, 0)])          # 0.29 degrees apart: merge
    c = tr([1, 0, 0.005], [(0, 2), (4, 0)])                                             # close, but shares image 0 with a
    d = tr([0, 1, 0], [(0, 1), (1, 1), (2, 0), (3, 1), (4, 1)])
    out = vplib.MergeVPTracksByDirection([a, b, c, d], 1.0)
    assert [t.length() for t in out] == [5, 4, 2]
    assert out[1].supports == a.supports + b.supports
    want = (a.direction * 3 + b.direction * 1) / 4
    assert np.allclose(out[1].direction, want / np.linalg.norm(want), rtol=0, atol=1e-15)
    assert out[2].supports == c.supports and np.array_equal(out[0].direction, d.direction)
    assert [t.length() for t in vplib.MergeVPTracksByDirection([a, b, c, d], 0.1)] == [5, 3, 2, 1]


def test_cluster_line_tracks_and_2d_vp_bipartites():
    """three images, two directions, six line tracks: the 2D VPs of a direction join one track; a VP seen by too few
    common lines stays out"""
    s = sc.structured_scene(n_cams=3, lines_per_dir=3, points_per_line=1, seed=4, n_free_points=0, junction=False)
    ids = [int(i) for i in s["img_ids"]]
    views = {i: CameraView(s["k"][n], s["q"][n], s["t"][n]) for n, i in enumerate(ids)}
    imagecols = ImageCollection(views)
    NL = len(s["line6"])
    res = {}
    for i in ids:  # image-space VP of direction c: K R d; labels by class; class 2 has no VP in the last image
        v = views[i]
        vps = [v.K() @ v.R() @ s["dirs_gt"][c] for c in range(3)]
        vps = [x / np.linalg.norm(x) for x in vps]
        labels = [int(c) if not (c == 2 and i == ids[-1]) else -1 for c in s["line_class"]]
        res[i] = vplib.VPResult(labels, vps)
    tracks = []
    for n in range(NL):
        a, b = int(s["loff"][n]), int(s["loff"][n + 1])
        tracks.append(LineTrack(Line3d(s["line6"][n, :3], s["line6"][n, 3:]), [int(x) for x in s["limg"][a:b]], [n] * (b - a),
                                [Line2d(s["l2d"][j, :2], s["l2d"][j, 2:]) for j in range(a, b)]))
    G = vplib.GlobalVPTrackConstructor(dict(min_common_lines=3, min_track_length=3))
    G.Init(res)
    out = G.ClusterLineTracks(tracks, imagecols)
    assert sorted(sorted(t.supports) for t in out) == [[(i, 0) for i in ids], [(i, 1) for i in ids]]
    for t in out:
        c = t.supports[0][1]
        assert abs(abs(float(t.direction @ s["dirs_gt"][c])) - 1.0) < 1e-12
    G2 = vplib.GlobalVPTrackConstructor(dict(min_common_lines=3, min_track_length=2))
    G2.Init(res)
    assert [t.length() for t in G2.ClusterLineTracks(tracks, imagecols)] == [3, 3, 2]
    G3 = vplib.GlobalVPTrackConstructor(dict(min_common_lines=4, min_track_length=2))
    G3.Init(res)
    assert G3.ClusterLineTracks(tracks, imagecols) == []
    # GetAllBipartites_VPLine2d over the two long tracks
    all_lines = {i: [np.zeros((2, 2)) + n for n in range(NL)] for i in ids}
    bp = structures.GetAllBipartites_VPLine2d(all_lines, res, out)
    for i in ids:
        b = bp[i]
        assert b.count_lines() == NL and sorted(b.get_point_ids()) == [0, 1]
        tid = {t.supports[0][1]: k for k, t in enumerate(out)}
        assert all(b.point(c).point3D_id == tid[c] for c in (0, 1))
        assert sorted((c, n) for c in b.get_point_ids() for n in b.neighbor_lines(c)) == \
            sorted((int(c), n) for n, c in enumerate(s["line_class"]) if c < 2)
    again = structures.VPLine_Bipartite2d(bp[ids[0]].as_dict())
    assert again.count_edges() == bp[ids[0]].count_edges() and np.array_equal(again.point(1).p, bp[ids[0]].point(1).p)


def test_refusals():
    s = sc.structured_scene(n_cams=4, seed=5)
    for kw, word in ((dict(constant_pose=False), "constant_pose"), (dict(constant_intrinsics=False), "constant_intrinsics")):
        with pytest.raises(ValueError, match=word):
            associator_of(s, **kw)
    for kw, word in ((dict(constant_pose=0), "constant_pose"), (dict(constant_intrinsics=0), "constant_intrinsics")):
        rc, _ = sc.run_host(s, sc.cfg_of(**kw))
        assert rc != 0 and word in sc.host_error()
    for key, word in (("p3", "non-finite"), ("vp3", "non-finite"), ("l2d", "non-finite"), ("edge_w", "non-finite")):
        bad = dict(s, **{key: s[key].copy()})
        bad[key].reshape(-1)[0] = np.nan
        rc, _ = sc.run_host(bad, sc.cfg_of())
        assert rc != 0 and word in sc.host_error(), key
    bad = dict(s, vp3=s["vp3"].copy())
    bad["vp3"][1] = 0.0
    rc, _ = sc.run_host(bad, sc.cfg_of())
    assert rc != 0 and "zero length" in sc.host_error()
    with pytest.raises(ValueError, match="zero length"):
        associator_of(bad)
    for key, val in (("edge_a", 10 ** 6), ("edge_b", -1), ("pimg", 999)):
        bad = dict(s, **{key: s[key].copy()})
        bad[key][0] = val
        rc, _ = sc.run_host(bad, sc.cfg_of())
        assert rc != 0 and "not in the collection" in sc.host_error(), key
    with pytest.raises(NotImplementedError):
        optimize.GlobalAssociator().ReassociateJunctions()


def test_config_keys_and_defaults():
    c = optimize.GlobalAssociatorConfig()
    assert (c.th_count_lineline, c.th_angle_lineline, c.lw_pointline_association, c.th_pixel, c.th_weight_pointline) == (3, 30.0, 10.0, 2.0, 3.0)
    assert (c.lw_vpline_association, c.th_count_vpline, c.lw_vp_orthogonality, c.th_angle_orthogonality) == (1.0, 3, 1.0, 87.0)
    assert (c.lw_vp_collinearity, c.th_angle_collinearity, c.th_hard_pl_dist3d, c.th_hard_vpline_angle3d, c.constant_vp) == (0.0, 1.0, 2.0, 5.0, False)
    assert (c.cg_eta, c.cg_max_iterations, c.lw_point, c.min_num_images) == (0.1, 500, 0.1, 4)
    assert c.point_line_association_3d_loss_function == ("HuberLoss", 0.01) and c.vp_collinearity_loss_function == ("TrivialLoss",)
    c = optimize.GlobalAssociatorConfig(dict(th_pixel_sigma=9.0, th_pixel=3.5, constant_vp=True, unknown=1))
    assert c.th_pixel == 3.5 and c.constant_vp is True and not hasattr(c, "th_pixel_sigma")


def test_solve_global_pl_association():
    s = sc.structured_scene(n_cams=5, lines_per_dir=2, points_per_line=2, seed=12)
    A = associator_of(s, max_num_iterations=0)
    bpt3d = structures.PL_Bipartite3d()
    for k, t in A.point_tracks_.items():
        bpt3d.add_point(t, k)
    for k, t in A.line_tracks_.items():
        bpt3d.add_line(t, k)
    out = optimize.solve_global_pl_association(dict(constant_intrinsics=True, constant_pose=True, th_pixel=6.0, max_num_iterations=40),
                                               A.imagecols_, bpt3d, A.all_bpt2ds_, host_threads=2)
    assert sorted((p - 10, n - 20) for p in out.get_point_ids() for n in out.neighbor_lines(p)) == sorted(s["incidences"])


# ---- 6. determinism ----
def test_two_runs_and_thread_counts_give_identical_bits():
    s = sc.structured_scene(n_cams=4, seed=7)
    cfg = sc.cfg_of(max_num_iterations=25)
    rc, a = sc.run_host(s, cfg, 1)
    rc2, b = sc.run_host(s, cfg, 4)
    rc3, c = sc.run_host(s, cfg, 4)
    assert rc == rc2 == rc3 == 0 and sc.same_bits(a, b) and sc.same_bits(b, c) and a["iterations"][0] == 25


# ---- goldens (tests/golden/make_assoc_golden.py) ----
def load_golden(path):
    """-> the scene, the configuration's keywords, the recorded outputs"""
    z = np.load(path)
    s = {k: np.ascontiguousarray(z[k]) for k in GOLDEN_IN}
    cfg = {k[4:]: z[k].item() for k in z.files if k.startswith("cfg_")}
    return s, cfg, {k[4:]: z[k] for k in z.files if k.startswith("out_")}


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "*.npz"))))
def test_goldens_reproduce(path):
    s, cfg, want = load_golden(path)
    rc, o = sc.run_host(s, sc.cfg_of(**cfg), 4)
    assert rc == 0 and set(o) == set(want)
    for k in o:
        assert np.array_equal(o[k], want[k]), (os.path.basename(path), k)


def test_goldens_exist():
    assert len(glob.glob(os.path.join(GOLDEN, "*.npz"))) >= 4


def test_sanitizer_program_of_the_host_twin():
    """tools/assoc_host_asan.cpp + lt_assoc.cpp (host-only) under AddressSanitizer and UBSan, a program of its own"""
    from helpers import run_host_asan
    run_host_asan("assoc_asan", "assoc_host_asan")
