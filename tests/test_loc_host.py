"""The point-line pose refinement (limap_amd.hybrid_localization) on the host, without a GPU:
limap's cost through lt_fn_loc_eval against the NumPy restatement (tests/loc_oracle.py) in longdouble, the minimiser
through lt_fn_loc_host against scipy, and the Python surface on its host path."""
import glob
import itertools
import os

import numpy as np
import pytest

import loc_oracle as lo
import loc_scenes as ls
from limap_amd import hybrid_localization as hl
from limap_amd import optimize

WEIGHT_NAMES = {0: None, 1: "cosine", 3: "length", 4: "invlength"}
COST_NAMES = ["MidpointDist2", "MidpointAngleDist", "PerpendicularDist2", "PerpendicularDist4", "3DLineLineDist2",
              "3DPlaneLineDist2"]
LOSS_OBJ = {0: lambda a: hl.TrivialLoss(), 1: hl.HuberLoss, 2: hl.SoftLOneLoss, 3: hl.CauchyLoss}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loc")
CSR_KEYS = ("P", "k", "q", "t", "line_off", "l3", "seg_off", "sg", "pt_off", "p3", "p2")  # hl._problem_arrays' tuple
OUT_KEYS = ("qvec", "tvec", "cost", "num_residuals", "iterations", "codes")


def struct_of(cfg):
    c = hl.LineLocConfig(dict(weight_line=cfg["weight_line"], weight_point=cfg["weight_point"],
                              loss_function=LOSS_OBJ[cfg["loss"]](cfg["loss_a"])))
    c.cost_function, c.cost_function_weight = cfg["cost"], cfg["weight"]
    return c._struct()


def ocfg(cost=2, weight=0, loss=0, loss_a=1.0, weight_line=1.0, weight_point=1.0):
    return dict(cost=cost, weight=weight, loss=loss, loss_a=loss_a, weight_line=weight_line, weight_point=weight_point)


def at_pose(pr, q, t):
    return dict(pr, qvec=np.asarray(q, float), tvec=np.asarray(t, float))


# ---- 1. the restatement ----
def _errors(cases):
    E = dict(r=0.0, cost=0.0, g=0.0, H=0.0)
    Eref = dict(E)
    for cfg, pr in cases:
        pose = np.concatenate([pr["qvec"], pr["tvec"]])
        ours = hl.loc_eval(struct_of(cfg), pr)
        f64 = lo.evaluate(pr, cfg, pose, np.float64)
        ld = lo.evaluate(pr, cfg, pose, np.longdouble)
        assert np.array_equal(np.isnan(ours[0]), np.isnan(ld[0].astype(float)))
        for nm, i in (("r", 0), ("cost", 1), ("g", 2), ("H", 3)):
            a, b, c = [np.nan_to_num(np.asarray(x, np.longdouble)) for x in (ours[i], f64[i], ld[i])]
            scale = max(float(np.abs(c).max()), 1.0)
            E[nm] = max(E[nm], float(np.abs(a - c).max()) / scale)
            Eref[nm] = max(Eref[nm], float(np.abs(b - c).max()) / scale)
    return E, Eref


def test_cost_and_derivatives_against_longdouble():
    """Every cost function x weight x loss (the point form follows the cost function, hybrid_localization.h:36-40), at
    the initial and at the GT pose, and the edge fixtures.  E_ref: the FP64 restatement's own maximum error against its
    longdouble evaluation, per quantity relative to the larger of 1 and the quantity's largest magnitude in the problem;
    ours must stay within 4 E_ref.  Measured: the figures this test prints."""
    pr = ls.make_problem(12, 14, seed=3)
    cases = []
    for cost, weight, loss in itertools.product(range(6), (0, 1, 3, 4), range(4)):
        cfg = ocfg(cost, weight, loss, loss_a=0.05 if cost in (4, 5) else 1.5, weight_line=0.7, weight_point=1.3)
        cases.append((cfg, pr))
        cases.append((cfg, at_pose(pr, pr["gt_q"], pr["gt_t"])))
    for name, over, epr in ls.edge_problems():
        for cost in ((over["cost"],) if "cost" in over else (0, 1, 2, 3)):
            for weight in (0, 1):
                cases.append((ocfg(**dict(over, cost=cost, weight=weight)), epr))
    E, Eref = _errors(cases)
    print("loc eval error, ours:", E, "restatement:", Eref)
    for nm in ("r", "cost", "g", "H"):
        assert E[nm] <= 4 * Eref[nm], (nm, E[nm], Eref[nm])


def test_edge_fixtures_take_the_intended_branches():
    edge = {n: (o, p) for n, o, p in ls.edge_problems()}
    k, q, t = list(edge["parallel"][1]["kvec"]), [1.0, 0, 0, 0], [0.0, 0, 0]
    f = np.float64
    # the 2D segment on the reprojection: both sines of the perpendicular distance are ~0, the cosine clamps at 1
    o, pr = edge["parallel"]
    sr, er = lo.world_to_pixel(k, q, t, list(pr["l3ds"][0][0])), lo.world_to_pixel(k, q, t, list(pr["l3ds"][0][1]))
    d2 = [er[0] - sr[0], er[1] - sr[1]]
    seg = pr["l2ds"][0][0]
    assert lo.cosine2d(d2, list(seg[1] - seg[0]), f) == 1.0
    seg = edge["perpendicular"][1]["l2ds"][0][0]
    assert lo.cosine2d(d2, list(seg[1] - seg[0]), f) < 1e-12
    assert lo.sine2d(d2, list(seg[1] - seg[0]), f) == 1.0
    # the ray through the first 2D endpoint is parallel to the 3D line
    o, pr = edge["ray_parallel_to_line"]
    l3, seg = pr["l3ds"][0], pr["l2ds"][0][0]
    pa = lo.pixel_to_world(k, q, t, seg[0][0], seg[0][1], 1.0)
    pb = lo.pixel_to_world(k, q, t, seg[0][0], seg[0][1], 2.0)
    d3 = (l3[1] - l3[0]) / np.linalg.norm(l3[1] - l3[0])
    n = np.cross(np.array(pb) - np.array(pa), d3)
    assert n @ n <= 1e-8
    res, _, _, _ = hl.loc_eval(struct_of(ocfg(cost=4)), pr)
    assert np.isfinite(res[0, :2]).all() and res[0, 0] > 0
    # Huber(2): the squared norms of the two point blocks are 1 and 25
    o, pr = edge["huber_sides"]
    res, cost, _, _ = hl.loc_eval(struct_of(ocfg(**o)), pr)
    s = (res[:, :2] ** 2).sum(1)
    assert s[0] < 4.0 < s[1]
    assert cost == pytest.approx(0.5 * (s[0] + (2 * 2.0 * np.sqrt(s[1]) - 4.0)), rel=1e-12)


# ---- 2. the minimiser ----
def _polish(pk, cfg, pose):
    from scipy.optimize import least_squares
    pose = np.array(pose, float)
    for _ in range(3):  # re-centre the local chart
        # trust-region reflective with the Jacobian's column scaling: MINPACK's "lm" stalls on the 3D distances, whose
        # rotation and translation columns differ by orders of magnitude
        res = least_squares(lambda dl: lo.residual_vector(pk, cfg, lo.retract(pose, dl)), np.zeros(6), method="trf",
                            x_scale="jac", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=2000)
        pose = lo.retract(pose, res.x)
    return lo.cost_only(pk, cfg, pose)


def _scipy_problem(job):
    pr, cfg, ours = job
    pk = lo.pack(pr, cfg)
    n = lambda q, t: np.concatenate([np.asarray(q) / np.linalg.norm(q), t])  # noqa: E731
    return (lo.cost_only(pk, cfg, ours), _polish(pk, cfg, n(pr["qvec"], pr["tvec"])), _polish(pk, cfg, n(pr["gt_q"], pr["gt_t"])),
            _polish(pk, cfg, ours))


@pytest.fixture(scope="module")
def solved():
    """96 noisy problems (0.5 px, 8-40 lines, 10-60 points), four configurations.  The initial pose is off by 0.05 rad and
    0.3 scene units: several times what 0.5 px of noise leaves at these counts (about 0.005 rad and 0.06 units for the
    smallest problem), so that "nearer the GT pose" is a statement about the minimiser and not about the noise."""
    out = []
    cfgs = [ocfg(2, 0, 0), ocfg(2, 1, 3, loss_a=2.0, weight_line=0.5), ocfg(0, 0, 1, loss_a=3.0), ocfg(4, 0, 3, loss_a=0.1)]
    for c, cfg in enumerate(cfgs):
        probs = [ls.make_problem(8 + (7 * n) % 33, 10 + (11 * n) % 51, seed=100 * c + n, init_rot=0.05, init_trans=0.3)
                 for n in range(24)]
        r = hl.loc_arrays(hl._problem_arrays([dict(p, l3ds=p["l3ds"], l2ds=p["l2ds"]) for p in probs]), struct_of(cfg), 4)
        out.append((cfg, probs, r))
    return out


def test_minimiser_descends_and_ends_nearer_the_gt_pose(solved):
    for cfg, probs, r in solved:
        print("cfg", cfg["cost"], cfg["loss"], "codes", np.bincount(r["codes"], minlength=8), "iterations min/median/max",
              r["iterations"].min(), np.median(r["iterations"]), r["iterations"].max())
        assert np.all(r["cost"][:, 1] <= r["cost"][:, 0]), "a cost rose"
        assert not np.any(r["codes"] == 0), "exit by the iteration cap at 100"
        assert np.all(np.isin(r["codes"], (1, 2)))
        for n, p in enumerate(probs):
            a0, d0 = ls.pose_distance(p["qvec"], p["tvec"], p["gt_q"], p["gt_t"])
            a1, d1 = ls.pose_distance(r["qvec"][n], r["tvec"][n], p["gt_q"], p["gt_t"])
            assert a1 < a0 and d1 < d0, (n, a0, a1, d0, d1)


def test_minimiser_reaches_the_minimum_scipy_finds(solved):
    """scipy.optimize.least_squares (trust-region reflective on the restated residual vector, in the chart of the retraction)
    from the initial and from the GT pose reaches one cost -- one basin, which this test checks -- and neither finds a
    lower cost than ours nor lowers ours by polishing, within 10 x scipy's own spread between its two starts.  The
    spread and the margin are printed."""
    from concurrent.futures import ProcessPoolExecutor
    jobs, ours_cost = [], []
    for cfg, probs, r in solved:
        for n, p in enumerate(probs):
            jobs.append((p, cfg, np.concatenate([r["qvec"][n], r["tvec"][n]])))
            ours_cost.append(r["cost"][n, 1])
    with ProcessPoolExecutor(max_workers=8) as ex:
        rows = np.array(list(ex.map(_scipy_problem, jobs, chunksize=4)))
    ours, c_init, c_gt, c_pol = rows.T
    assert np.allclose(ours, ours_cost, rtol=1e-9, atol=0), "the restated cost at our solution is not our cost"
    spread = float((np.abs(c_init - c_gt) / np.maximum(c_init, c_gt)).max())
    margin = 10 * spread
    print(f"scipy spread between its two starts {spread:.3e}, margin {margin:.3e}; polishing lowers ours by at most "
          f"{float(((ours - c_pol) / ours).max()):.3e}; ours above scipy's best by at most "
          f"{float(((ours - np.minimum(c_init, c_gt)) / ours).max()):.3e}")
    assert spread < 1e-6, "the fixture is not one basin"
    assert np.all(c_pol >= ours * (1 - margin)), "polishing from our solution lowered the cost"
    assert np.all(ours <= np.minimum(c_init, c_gt) * (1 + margin)), "scipy found a lower cost from the initial / GT pose"


# ---- 4. the Python surface on the host path ----
def test_names_are_reexported_from_optimize():
    for n in hl.__all__:
        assert getattr(optimize, n) is getattr(hl, n) and n in optimize.__all__


def test_aliases():
    F, W = hl.LineLocCostFunction, hl.LineLocCostFunctionWeight
    table = {F.E2DMidpointDist2: ["MidpointDist", "MidpointDist2", "2DMidpointDist", "2DMidpointDist2"],
             F.E2DMidpointAngleDist3: ["MidpointAngle", "MidpointAngleDist", "2DMidpointAngleDist"],
             F.E2DPerpendicularDist2: ["PerpendicularDist", "PerpendicularDist2", "2DPerpendicularDist", "2DPerpendicularDist2"],
             F.E2DPerpendicularDist4: ["PerpendicularDist4", "2DPerpendicularDist4"],
             F.E3DLineLineDist2: ["3DLineLineDist", "3DLineLineDist2"], F.E3DPlaneLineDist2: ["3DPlaneLineDist", "3DPlaneLineDist2"]}
    for v, names in table.items():
        assert all(hl.get_lineloc_cost_func(n) == v for n in names)
    assert [hl.get_lineloc_weight_func(n) for n in (None, "Cosine", "line3dpp", "LENGTH", "invlength")] == \
        [W.ENoneWeight, W.ECosineWeight, W.ELine3dppWeight, W.ELengthWeight, W.EInvLengthWeight]
    for f, bad in ((hl.get_lineloc_cost_func, "Nope"), (hl.get_lineloc_weight_func, "nope")):
        with pytest.raises(ValueError, match="Unknown"):
            f(bad)


def test_get_line_pairs_keeps_first_appearance_order():
    l3ds = ["a", "b", "c", "d"]
    l2ds, l3 = hl.get_line_pairs(l3ds, [2, 0, 2, 3, 0], ["s0", "s1", "s2", "s3", "s4"])
    assert l3 == ["c", "a", "d"] and l2ds == [["s0", "s2"], ["s1", "s4"], ["s3"]]
    with pytest.raises(ValueError, match="l3d_id 4"):
        hl.get_line_pairs(l3ds, [4], ["s"])
    with pytest.raises(ValueError, match="l3d_id -1"):
        hl.get_line_pairs(l3ds, [-1], ["s"])


def _K(kvec):
    return np.array([[kvec[0], 0, kvec[2]], [0, kvec[1], kvec[3]], [0, 0, 1.0]])


def test_engines_and_both_initialize_overloads():
    from limap_amd.base import Line2d, Line3d
    pr = ls.make_problem(9, 12, seed=5)
    cfg = dict(weight_line=0.8, loss_function=hl.CauchyLoss(2.0), solver_options=dict(max_num_iterations=60,
               function_tolerance=0.0, minimizer_progress_to_stdout=False, logging_type="SILENT"))
    batch = hl.solve_jointloc_batch("PerpendicularDist", cfg, [pr], "cosine", host=True)
    e1 = hl.solve_jointloc("PerpendicularDist", cfg, pr["l3ds"], pr["l3d_ids"], pr["l2ds_flat"], pr["p3ds"], pr["p2ds"],
                           _K(pr["kvec"]), pr["R0"], pr["tvec"], line_weight_func="cosine", host=True)
    # get_line_pairs regroups the shuffled flat list: other block order, the same minimum
    assert np.allclose(e1.GetFinalQ(), batch["qvec"][0], atol=1e-7) and np.allclose(e1.GetFinalT(), batch["tvec"][0], atol=1e-6)
    assert e1.IsSolutionUsable() and e1.GetFinalCost() < e1.GetInitialCost()
    assert np.allclose(e1.GetFinalR() @ e1.GetFinalR().T, np.eye(3), atol=1e-14)
    # (kvec, qvec, tvec) overload with Line3d / Line2d objects, merged pairs: the batch's own block order, bit for bit
    c = hl.LineLocConfig(cfg)
    c.cost_function, c.cost_function_weight = hl.get_lineloc_cost_func("PerpendicularDist"), hl.get_lineloc_weight_func("cosine")
    e2 = hl.JointLocEngine(c, host=True)
    e2.Initialize([Line3d(l[0], l[1]) for l in pr["l3ds"]], [[Line2d(s[0], s[1]) for s in g] for g in pr["l2ds"]],
                  list(pr["p3ds"]), list(pr["p2ds"]), pr["kvec"], pr["qvec"], pr["tvec"])
    e2.SetUp()
    assert e2.Solve() is True
    assert np.array_equal(e2.GetFinalQ(), batch["qvec"][0]) and np.array_equal(e2.GetFinalT(), batch["tvec"][0])
    r = e2.result()
    assert e2.GetInitialCost() == np.sqrt(r["cost"][0, 0] / r["num_residuals"][0])
    assert r["num_residuals"][0] == 2 * sum(len(g) for g in pr["l2ds"]) + 2 * len(pr["p3ds"])
    # the (K, R, T) overload: R goes through Eigen's matrix-to-quaternion procedure
    e3 = hl.JointLocEngine(c, host=True)
    e3.Initialize(pr["l3ds"], pr["l2ds"], pr["p3ds"], pr["p2ds"], _K(pr["kvec"]), pr["R0"], pr["tvec"])
    e3.Solve()
    assert np.allclose(e3.GetFinalQ(), e2.GetFinalQ(), atol=1e-9)
    # LineLocEngine: no points, weight_line not applied
    e4 = hl.solve_lineloc("PerpendicularDist", pr["l3ds"], pr["l3d_ids"], pr["l2ds_flat"], _K(pr["kvec"]), pr["R0"], pr["tvec"],
                          lineloc_cfg=dict(weight_line=123.0), host=True)
    e5 = hl.solve_lineloc_merged("PerpendicularDist", None, hl.get_line_pairs(pr["l3ds"], pr["l3d_ids"], pr["l2ds_flat"]),
                                 _K(pr["kvec"]), pr["R0"], pr["tvec"], host=True)
    assert np.array_equal(e4.GetFinalQ(), e5.GetFinalQ()) and e4.result()["cost"][0, 0] == e5.result()["cost"][0, 0]
    assert e4.result()["num_residuals"][0] == 2 * len(pr["l2ds_flat"])


def test_pl_estimate_absolute_pose_null_path_with_inlier_masks():
    pr = ls.make_problem(10, 20, seed=8)
    cfg = dict(ransac=dict(method=None), line_cost_func="PerpendicularDist", line_weight=2.0,
               optimize=dict(loss_func="HuberLoss", loss_func_args=[3.0]))
    in_p = np.ones(20, bool); in_p[[1, 5]] = False
    in_l = np.ones(len(pr["l3d_ids"]), bool); in_l[0] = False
    start = hl.CameraPose(pr["qvec"], pr["tvec"])
    pose, stats = hl.pl_estimate_absolute_pose(cfg, pr["l3ds"], pr["l3d_ids"], pr["l2ds_flat"], pr["p3ds"], pr["p2ds"],
                                               _K(pr["kvec"]), start, inliers_line=in_l, inliers_point=in_p, host=True)
    assert stats is None
    ids = [i for i, m in zip(pr["l3d_ids"], in_l) if m]
    segs = [s for s, m in zip(pr["l2ds_flat"], in_l) if m]
    e = hl.solve_jointloc("PerpendicularDist", dict(loss_function=hl.HuberLoss(3.0), weight_line=2.0, weight_point=1.0),
                          pr["l3ds"], ids, segs, pr["p3ds"][in_p], pr["p2ds"][in_p], _K(pr["kvec"]), start.R(), start.T(),
                          host=True)
    assert np.array_equal(pose.qvec, e.GetFinalQ() / np.linalg.norm(e.GetFinalQ())) and np.array_equal(pose.tvec, e.GetFinalT())
    a1, d1 = ls.pose_distance(pose.qvec, pose.tvec, pr["gt_q"], pr["gt_t"])
    a0, d0 = ls.pose_distance(pr["qvec"], pr["tvec"], pr["gt_q"], pr["gt_t"])
    assert a1 < a0 and d1 < d0
    for method in ("ransac", "solver", "hybrid"):
        with pytest.raises(NotImplementedError, match=method):
            hl.pl_estimate_absolute_pose(dict(cfg, ransac=dict(method=method)), [], [], [], [], [], _K(pr["kvec"]), start)


def test_a_problem_without_residuals_keeps_its_pose():
    pr = ls.make_problem(3, 4, seed=2)
    e = hl.JointLocEngine(None, host=True)
    e.Initialize([], [], [], [], pr["kvec"], pr["qvec"], pr["tvec"])
    e.SetUp()
    assert e.Solve() is False and not e.IsSolutionUsable()
    r = e.result()
    assert r["codes"][0] == 7 and r["iterations"][0] == 0 and r["num_residuals"][0] == 0
    assert np.array_equal(e.GetFinalQ(), pr["qvec"] / np.sqrt((pr["qvec"][[0, 2]] ** 2).sum() + (pr["qvec"][[1, 3]] ** 2).sum()))
    assert np.array_equal(e.GetFinalT(), pr["tvec"])
    # a 3D line without 2D segments adds no block either
    e.Initialize([pr["l3ds"][0]], [[]], [], [], pr["kvec"], pr["qvec"], pr["tvec"])
    assert e.Solve() is False


def test_rejections():
    pr = ls.make_problem(4, 5, seed=4)

    def solve(over=None, cfg=None, weight=None, cost="PerpendicularDist"):
        return hl.solve_jointloc_batch(cost, cfg, [dict(pr, **(over or {}))], weight, host=True)
    solve()
    bad_l3 = pr["l3ds"].copy(); bad_l3[1, 1] = bad_l3[1, 0]
    nan_p = pr["p3ds"].copy(); nan_p[0, 0] = np.nan
    zero_l2 = [list(g) for g in pr["l2ds"]]; zero_l2[2] = [np.array([[5.0, 6.0], [5.0, 6.0]])] * len(zero_l2[2])
    for over, msg in ((dict(l3ds=bad_l3), "zero length"), (dict(p3ds=nan_p), "non-finite"),
                      (dict(tvec=np.array([0.0, np.inf, 0.0])), "non-finite"), (dict(l2ds=zero_l2), "sum_lengths == 0")):
        with pytest.raises(ValueError, match=msg):
            solve(over)
    with pytest.raises(ValueError, match="line3dpp"):
        solve(weight="line3dpp")
    for loss in (hl.HuberLoss, hl.SoftLOneLoss, hl.CauchyLoss):
        for a in (0.0, -1.0, np.nan):
            with pytest.raises(ValueError, match="must be > 0"):
                loss(a)
    c = hl.LineLocConfig(dict(loss_function=hl.HuberLoss(1.0)))
    c.loss_function.a = 0.0  # past the value class: the native check
    with pytest.raises(ValueError, match="loss parameter"):
        hl.loc_arrays(hl._problem_arrays([pr]), c._struct(), 1)
    with pytest.raises(ValueError, match="function_tolerance"):
        hl.LineLocConfig(dict(solver_options=dict(function_tolerance=1e-6)))
    for key in ("trust_region_strategy_type", "linear_solver_type", "use_nonmonotonic_steps", "initial_trust_region_radius"):
        with pytest.raises(ValueError, match=key):
            hl.LineLocConfig(dict(solver_options={key: 1}))
    with pytest.raises(ValueError, match="l3d_id 9"):
        hl.solve_jointloc("PerpendicularDist", None, pr["l3ds"], [9], [pr["l2ds_flat"][0]], [], [], pr["kvec"], pr["qvec"],
                          pr["tvec"], host=True)


def test_host_result_does_not_depend_on_threads_or_problem_order():
    probs = [ls.make_problem(5 + 13 * n, 3 + 29 * n, seed=40 + n) for n in range(6)] + [dict(ls.make_problem(2, 2, seed=1), l3ds=np.zeros((0, 2, 3)), l2ds=[], p3ds=[], p2ds=[])]
    cfg = dict(loss_function=hl.SoftLOneLoss(1.0))
    a = hl.solve_jointloc_batch("PerpendicularDist4", cfg, probs, "length", host_threads=1)
    b = hl.solve_jointloc_batch("PerpendicularDist4", cfg, probs[::-1], "length", host_threads=4)
    for key in ("qvec", "tvec", "cost", "num_residuals", "iterations", "codes"):
        assert np.array_equal(a[key], b[key][::-1]), key
    assert a["codes"][-1] == 7


# ---- goldens (tests/golden/make_loc_golden.py) ----
def load_golden(path):
    """-> the CSR tuple of hl.loc_arrays, the configuration struct, the recorded outputs"""
    z = np.load(path)
    csr = (int(z["in_P"]),) + tuple(np.ascontiguousarray(z["in_" + k]) for k in CSR_KEYS[1:])
    s = struct_of({k[4:]: z[k].item() for k in z.files if k.startswith("cfg_")})
    s.max_num_iterations = int(z["max_num_iterations"])
    return csr, s, {k: z["out_" + k] for k in OUT_KEYS}


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "*.npz"))))
def test_goldens_reproduce(path):
    csr, s, want = load_golden(path)
    r = hl.loc_arrays(csr, s, 4)
    for k in OUT_KEYS:
        assert np.array_equal(r[k], want[k]), (os.path.basename(path), k)


def test_goldens_exist():
    assert len(glob.glob(os.path.join(GOLDEN, "*.npz"))) >= 7


# ---- 3. pose scoring ----
# a cell whose threshold quantity lies this close to its threshold may fall on either side: FP64 rounding of a chain of
# about a hundred operations on coordinates up to 1e3 is below 1e-10 of a cosine or a depth and below 1e-9 of a pixel
SCORE_MARGIN = 1e-8
SCORE_COSTS = {"MidpointDist": 0, "PerpendicularDist": 2, "PerpendicularDist4": 3, "3DLineLineDist": 4, "3DPlaneLineDist": 5}


@pytest.fixture(scope="module")
def score_ref():
    """the fixture with the restatement's tables (float64, longdouble) and margins, computed once"""
    fx = ls.score_fixture()
    out = {}
    for name in ("PerpendicularDist", "PerpendicularDist4", "3DLineLineDist"):
        args = (SCORE_COSTS[name], fx["kvec"], fx["poses"], fx["l3ds"], fx["l3d_ids"], fx["l2ds"], fx["p3ds"], fx["p2ds"], 0.0, 10.0)
        out[name] = lo.score_table(*args, np.float64) + (lo.score_table(*args, np.longdouble)[0],)
    return fx, out


def test_score_fixture_reaches_every_cheirality_test_and_stays_clear_of_the_margins(score_ref):
    fx, ref = score_ref
    n_pts = len(fx["p3ds"])
    causes = set()
    for h, pose in enumerate(fx["poses"]):
        for i in range(n_pts + len(fx["l2ds"])):
            ms = []
            j = i - n_pts
            v = (lo.score_cell(2, fx["kvec"], pose[:4], pose[4:], 1, fx["p3ds"][i], fx["p2ds"][i], None, 0.0, 10.0, np.float64, ms)
                 if i < n_pts else
                 lo.score_cell(2, fx["kvec"], pose[:4], pose[4:], 0, None, fx["l2ds"][j], fx["l3ds"][fx["l3d_ids"][j]], 0.0, 10.0,
                               np.float64, ms))
            if v == lo.DBL_MAX:
                tag = ms[-1][0] if ms else "nan"
                if tag == "depth":
                    tag = "point_depth" if i < n_pts else "unprojection_depth"
                causes.add(tag)
    assert causes == {"nan", "point_depth", "angle", "unprojection_depth", "overlap"}, causes
    for name, (tab, mar, _) in ref.items():
        inside = float((mar < SCORE_MARGIN).mean())
        print(name, "cells inside a margin:", inside, "DBL_MAX cells:", float((tab == lo.DBL_MAX).mean()))
        assert inside <= 0.02
        assert 0.1 < (tab == lo.DBL_MAX).mean() < 0.9


@pytest.mark.parametrize("name", ["PerpendicularDist", "PerpendicularDist4", "3DLineLineDist"])
def test_score_host_against_the_restatement(score_ref, name):
    fx, ref = score_ref
    tab64, mar, tabld = ref[name]
    thr, wts = (4.0, 9.0), (1.0, 0.5)
    r = hl.score_poses(name, fx["l3ds"], fx["l3d_ids"], fx["l2ds"], fx["p3ds"], fx["p2ds"], fx["kvec"], fx["poses"],
                       thresholds=thr, weights=wts, host=True)
    ours = r["residuals"]
    clear = mar >= SCORE_MARGIN
    assert np.array_equal((ours == lo.DBL_MAX)[clear], (tab64 == lo.DBL_MAX)[clear])
    assert np.array_equal((ours == lo.DBL_MAX)[clear], (tabld.astype(float) >= lo.DBL_MAX)[clear])
    fin = clear & (ours < lo.DBL_MAX) & (tab64 < lo.DBL_MAX)
    scale = max(1.0, float(np.abs(tabld[fin]).max()))
    E = float(np.abs(ours[fin] - tabld[fin]).max()) / scale
    Eref = float(np.abs(tab64[fin] - tabld[fin]).max()) / scale
    print(name, "score error, ours:", E, "restatement:", Eref)
    assert E <= 4 * Eref
    scores, inl = lo.msac_from_table(ours, len(fx["p3ds"]), thr, wts)
    assert np.array_equal(scores, r["scores"]) and np.array_equal(inl, r["inliers"])
    # without thresholds: the table alone
    r2 = hl.score_poses(name, fx["l3ds"], fx["l3d_ids"], fx["l2ds"], fx["p3ds"], fx["p2ds"], fx["kvec"], fx["poses"], host=True)
    assert np.array_equal(r2["residuals"], ours) and r2["scores"] is None and r2["inliers"] is None


def test_score_rejections():
    fx = ls.score_fixture(4, 4, 2)
    a = (fx["l3ds"], fx["l3d_ids"], fx["l2ds"], fx["p3ds"], fx["p2ds"], fx["kvec"], fx["poses"])
    with pytest.raises(ValueError, match="MidpointAngleDist3"):
        hl.score_poses("MidpointAngle", *a, host=True)
    with pytest.raises(ValueError, match="l3d_id 99"):
        hl.score_poses("PerpendicularDist", fx["l3ds"], [99] * len(fx["l2ds"]), *a[2:], host=True)
    bad = fx["l3ds"].copy(); bad[0, 1] = bad[0, 0]
    with pytest.raises(ValueError, match="zero length"):
        hl.score_poses("PerpendicularDist", bad, *a[1:], host=True)
    badp = fx["p2ds"].copy(); badp[0, 0] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        hl.score_poses("PerpendicularDist", *a[:4], badp, *a[5:], host=True)
    empty = hl.score_poses("PerpendicularDist", *a[:6], np.zeros((0, 7)), thresholds=(1.0, 1.0), host=True)
    assert empty["residuals"].shape == (0, len(fx["p3ds"]) + len(fx["l2ds"])) and len(empty["scores"]) == 0
