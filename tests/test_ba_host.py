"""The bundle adjustment with free poses, points and lines (limap_amd.optimize.solve_hybrid_bundle_adjustment, DESIGN.md
section 27) on the host, without a GPU: limap's own part through lt_fn_ba_eval against the NumPy restatement
(tests/ba_oracle.py) in longdouble, the linear algebra (the Schur route against the dense normal equations, the defined
Cholesky recurrence against a straight loop), the minimiser through lt_fn_ba_host against scipy, upstream's switches,
determinism and the Python surface on its host path."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import ba_oracle as bo
import ba_scenes as bs
import refine_oracle as ro
import refine_scenes as rs
from limap_amd import _capi, optimize
from limap_amd.base import CameraView, ImageCollection, Line2d, Line3d, LineTrack, PointTrack

p = _capi.ptr
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ba")
GOLDEN_IN = ("img_ids", "k", "q", "t", "p3", "poff", "pimg", "pxy", "line6", "loff", "limg", "l2d", "l3d")


@pytest.fixture(scope="module")
def L():
    return _capi.load_library()


@pytest.fixture(scope="module")
def hybrid():
    """4 cameras, 24 points, 6 lines, half a pixel of noise, poses and structure perturbed within one basin"""
    return bs.make_scene(n_cams=4, n_points=24, n_lines=6, seed=0)


def eval_ours(L, s, cfg, params6=None, mu=None):
    dims = np.zeros(4, np.int64)
    a = bs.args_of(s, cfg)
    pp = None if params6 is None else p(np.ascontiguousarray(params6, float), C.c_double)
    assert L.lt_fn_ba_eval(*a, pp, p(dims, C.c_int64), None, None, None, None, None, 0.0, None) == 0, L.lt_fn_ba_host_error()
    nb, nu = int(dims[1]), int(dims[2])
    r = np.zeros((nb, 2)); c = C.c_double(); g = np.zeros(nu); H = np.zeros((nu, nu)); step = np.zeros(nu)
    info = np.zeros((nb, 3), np.int32)
    assert L.lt_fn_ba_eval(*a, pp, p(dims, C.c_int64), p(info, C.c_int32), p(r, C.c_double), C.byref(c), p(g, C.c_double),
                           p(H, C.c_double), float(mu or 1.0), p(step, C.c_double) if mu else None) == 0
    return dict(r=r, cost=c.value, g=g, H=H, step=step, info=info, dims=dims)


def edge_ba_scene():
    """section 19's edge fixtures (the fallback basis, wvec = (1, 0), the |x| kink, cosine near the clamp, two supports in
    one image) as line tracks of a bundle adjustment, their minimal parameters given"""
    e = rs.edge_scene()
    s = dict(img_ids=e["img_ids"], k=e["k"], q=e["q"], t=e["t"], p3=np.zeros((0, 3)), poff=np.zeros(1, np.int64),
             pimg=np.zeros(0, np.int32), pxy=np.zeros((0, 2)), line6=e["line6"], loff=e["off"], limg=e["img"], l2d=e["l2d"],
             l3d=e["l3d"])
    return s, np.array([pp for _, _, _, pp in rs.edge_tracks()])


# ---- 1. the restatement ----
def test_eval_against_longdouble_restatement(L):
    """E_ref: the FP64 restatement's own maximum error against its longdouble evaluation, per quantity relative to the
    larger of 1 and the quantity's largest magnitude in the scene; ours must stay within 4 E_ref.  Measured (DESIGN
    section 27): the figures this test prints."""
    cases = []
    for n_cams, seed in ((3, 1), (6, 2)):
        s = bs.make_scene(n_cams=n_cams, n_points=8, n_lines=6, seed=seed, point_obs=[1, 15, 16, 17, 33, 2 * n_cams],
                          line_obs=[1, 15, 16, 17, 33])
        cases.append((s, np.array([ro.minimal(l) for l in s["line6"]]), dict(min_num_images=1)))
    cases.append((bs.make_scene(n_cams=5, n_points=6, n_lines=4, seed=3), None, {}))
    es, epp = edge_ba_scene()
    assert epp[0][5] == 0.0 and epp[0][4] == 1.0  # wvec = (1, 0): the |x| kink and the fallback basis of a line through the origin
    cases.append((es, epp, dict(min_num_images=1)))
    E = dict(r=0.0, cost=0.0, g=0.0, H=0.0); Eref = dict(E)
    for s, pp, sw in cases:
        if pp is None:
            pp = np.array([ro.minimal(l) for l in s["line6"]])
        ours = eval_ours(L, s, bs.cfg_of(num_outliers_aggregator=0, **sw), pp)  # (a track with one support has two values)
        f64 = bo.evaluate(s, np.float64, params6=pp, **sw)
        ld = bo.evaluate(s, np.longdouble, params6=pp, **sw)
        assert ours["H"].shape == ld[3].shape
        for nm, i in (("r", 0), ("cost", 1), ("g", 2), ("H", 3)):
            scale = max(float(np.abs(ld[i]).max()), 1.0)
            E[nm] = max(E[nm], float(np.abs(ours[nm] - ld[i]).max()) / scale)
            Eref[nm] = max(Eref[nm], float(np.abs(f64[i] - ld[i]).max()) / scale)
    print("ba eval error, ours:", E, "restatement:", Eref)
    for nm in ("r", "cost", "g", "H"):
        assert E[nm] <= 4 * Eref[nm], (nm, E[nm], Eref[nm])


# ---- 2. the linear algebra ----
def _solve_ld(A, b):
    """Gaussian elimination with partial pivoting in longdouble (numpy's solvers stop at float64)"""
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


def test_schur_step_equals_dense_normal_equations(L, hybrid):
    """The step of the Schur route (damping, V^-1, S, the defined Cholesky, back substitution) against the solution of
    the full dense damped normal equations built from lt_fn_ba_eval's H and g, solved in longdouble.  Bound: 4 times the
    FP64 dense solve's own error against longdouble (numpy.linalg.solve), relative to the larger of 1 and the largest
    step entry.  Measured: the figures this test prints."""
    mu = 1e4
    ev = eval_ours(L, hybrid, bs.cfg_of(), mu=mu)
    H, g = ev["H"], ev["g"]
    assert H.shape == (4 * 6 + 24 * 3 + 6 * 4,) * 2 and np.all(np.isfinite(ev["step"]))
    D = np.clip(np.sqrt(np.diag(H)), 1e-6, 1e32)
    A = H + np.diag(D * D / mu)
    ref = _solve_ld(A, -g)
    f64 = np.linalg.solve(A, -g)
    scale = max(1.0, float(np.abs(ref).max()))
    e_ref = float(np.abs(f64 - ref).max()) / scale
    e_ours = float(np.abs(ev["step"] - ref).max()) / scale
    print("ba step error, Schur route:", e_ours, "dense FP64 solve:", e_ref)
    assert e_ours <= 4 * e_ref, (e_ours, e_ref)


@pytest.mark.parametrize("n", [1, 6, 7, 64, 65, 258])
def test_cholesky_is_the_defined_recurrence(L, n):
    rng = np.random.default_rng(n)
    A = rng.normal(size=(n, n + 3))
    S = A @ A.T + 0.1 * np.eye(n)
    rhs = rng.normal(size=n)
    Lo = np.zeros((n, n)); x = np.zeros(n)
    assert L.lt_fn_ba_cholesky(n, p(np.ascontiguousarray(S), C.c_double), p(rhs, C.c_double), p(Lo, C.c_double), p(x, C.c_double)) == 0
    Lr, xr = bo.cholesky_loop(S, rhs)
    assert np.array_equal(Lo, Lr) and np.array_equal(x, xr)
    assert np.allclose(Lo @ Lo.T, S, rtol=1e-10, atol=1e-10)
    S[n // 2, n // 2] = -1.0  # a non-positive pivot is reported, not factorised
    assert L.lt_fn_ba_cholesky(n, p(np.ascontiguousarray(S), C.c_double), p(rhs, C.c_double), p(Lo, C.c_double), p(x, C.c_double)) != 0


# ---- 3. it minimises ----
def test_minimises_the_restated_cost(L, hybrid):
    """The accepted-step cost sequence never rises; the final cost is not above the cost at the ground truth; and
    scipy.optimize.least_squares on the restated cost in the same chart, from the same start and from the ground truth,
    finds nothing lower than ours beyond 10 x its own spread between its two starts (section 19 test 4's rule).
    Measured: the figures this test prints."""
    from scipy.optimize import least_squares
    seq = []
    for it in range(0, 31):
        rc, o = bs.run_host(hybrid, bs.cfg_of(max_num_iterations=it), 1)
        assert rc == 0 and o["iterations"][0] == it
        seq.append(float(o["cost"][1]))
    assert seq[0] == float(o["cost"][0])
    assert all(b <= a for a, b in zip(seq, seq[1:])), seq
    assert seq[-1] < 0.05 * seq[0]
    rc, o = bs.run_host(hybrid, bs.cfg_of(max_num_iterations=100), 1)
    ours = float(o["cost"][1])
    pk = bo.Packed(hybrid)
    x0, xg = pk.start(hybrid), pk.start(bs.at_ground_truth(hybrid))
    assert abs(pk.cost(x0) - float(o["cost"][0])) <= 1e-9 * float(o["cost"][0])  # the same cost at the same start
    gt_cost = pk.cost(xg)
    sol = []
    for x in (x0, xg):  # the same chart as the minimiser's: local steps around the start, through the project's retractions
        to_point, nu = pk.chart(x)
        assert np.allclose(to_point(np.zeros(nu)), x, rtol=0, atol=1e-15)  # (the retractions renormalise: last bits)
        sol.append(least_squares(lambda y: pk.residuals(to_point(y)), np.zeros(nu), method="trf", xtol=1e-15, ftol=1e-15,
                                 gtol=1e-15, max_nfev=400))
    sc = [float(r.cost) for r in sol]
    spread = abs(sc[0] - sc[1])
    print("ba cost: ours", ours, "ground truth", gt_cost, "scipy from the start / from the ground truth", sc, "spread", spread,
          "differences", [ours - c for c in sc])
    assert min(sc) <= gt_cost  # the scene: scipy itself is not above the ground truth
    assert ours <= gt_cost
    assert ours - min(sc) <= 10 * spread, (ours, sc)


# ---- 4. the switches ----
def _poses_moved(s, o):
    return not np.array_equal(o["tvec"], s["t"])


def test_constant_point(hybrid):
    rc, o = bs.run_host(hybrid, bs.cfg_of(constant_point=1, max_num_iterations=20))
    assert rc == 0 and np.array_equal(o["points"], hybrid["p3"]) and _poses_moved(hybrid, o)
    assert o["cost"][1] < o["cost"][0]


def test_constant_line_and_min_num_images(hybrid):
    nl = bs.without_lines(hybrid, [])
    rc, base = bs.run_host(nl, bs.cfg_of(max_num_iterations=10))
    for sw, keep in ((dict(constant_line=1), [0, 1, 2, 3, 4, 5]), (dict(min_num_images=5), [0])):
        s = bs.without_lines(hybrid, keep)
        rc, o = bs.run_host(s, bs.cfg_of(max_num_iterations=10, **sw))
        assert rc == 0
        pp0 = np.array([ro.minimal(l) for l in s["line6"]])
        assert np.allclose(o["params"], pp0, rtol=0, atol=1e-15)
        rc, z = bs.run_host(s, bs.cfg_of(max_num_iterations=0, **sw))
        assert np.array_equal(o["params"], z["params"])  # the line is unchanged bit for bit
        assert np.array_equal(o["segments"], z["segments"]) and np.all(np.isfinite(o["segments"]))  # and its segment re-cut
        assert not np.array_equal(o["segments"][:, :3], s["line6"][:, :3])
        # its blocks were added: the cameras' result differs from the run without the track
        assert not np.array_equal(o["tvec"], base["tvec"]) and o["cost"][0] > base["cost"][0]


def test_lw_point_zero_equals_no_point_tracks(hybrid):
    rc, a = bs.run_host(hybrid, bs.cfg_of(lw_point=0.0, max_num_iterations=15))
    rc2, b = bs.run_host(bs.without_points(hybrid), bs.cfg_of(max_num_iterations=15))
    assert rc == 0 and rc2 == 0
    assert np.array_equal(a["points"], hybrid["p3"])
    for k in ("qvec", "tvec", "params", "segments", "cost", "iterations", "code"):
        assert np.array_equal(a[k], b[k]), k


def test_image_without_observations_keeps_its_pose():
    s = bs.make_scene(n_cams=4, n_points=12, n_lines=4, seed=4, extra_images=(9,))  # ids 5 8 9 11 14: 9 in the middle
    base = bs.make_scene(n_cams=4, n_points=12, n_lines=4, seed=4)
    row = int(np.where(s["img_ids"] == 9)[0][0])
    assert 0 < row < len(s["img_ids"]) - 1
    rc, o = bs.run_host(s, bs.cfg_of(max_num_iterations=15))
    rc2, b = bs.run_host(base, bs.cfg_of(max_num_iterations=15))
    assert rc == 0 and rc2 == 0
    assert np.array_equal(o["qvec"][row], s["q"][row]) and np.array_equal(o["tvec"][row], s["t"][row])
    others = [n for n in range(len(s["img_ids"])) if n != row]
    assert np.array_equal(o["qvec"][others], b["qvec"]) and np.array_equal(o["tvec"][others], b["tvec"])
    assert np.array_equal(o["points"], b["points"]) and np.array_equal(o["cost"], b["cost"])


def one_point(s, n):
    """the scene with point track n alone"""
    g = bs.without_lines(s, [])
    a, b = int(s["poff"][n]), int(s["poff"][n + 1])
    g.update(p3=np.ascontiguousarray(s["p3"][n:n + 1]), poff=np.array([0, b - a], np.int64),
             pimg=np.ascontiguousarray(s["pimg"][a:b]), pxy=np.ascontiguousarray(s["pxy"][a:b]))
    return g


def test_constant_pose_with_points_is_block_diagonal():
    """constant_pose=True: every point equals its own one-point solve bit for bit, the poses keep their input"""
    s = bs.without_lines(bs.make_scene(n_cams=6, n_points=9, n_lines=0, seed=7, point_obs=[1, 15, 16, 17, 33, 2]), [])
    rc, o = bs.run_host(s, bs.cfg_of(constant_pose=1, max_num_iterations=30))
    assert rc == 0 and np.array_equal(o["qvec"], s["q"]) and np.array_equal(o["tvec"], s["t"])
    # (the poses stay at their perturbed start, so the cost falls only as far as the points alone can take it)
    assert o["cost"][1] < o["cost"][0] and not np.array_equal(o["points"], s["p3"])
    cost0 = cost1 = 0.0
    iters = []
    for n in range(len(s["p3"])):
        rc, one = bs.run_host(one_point(s, n), bs.cfg_of(constant_pose=1, max_num_iterations=30), 1)
        assert rc == 0 and np.array_equal(one["points"][0], o["points"][n]), n
        cost0, cost1 = cost0 + one["cost"][0], cost1 + one["cost"][1]
        iters.append(int(one["iterations"][0]))
    assert len(set(iters)) > 1  # every track its own radius and its own end
    assert o["cost"][0] == cost0 and o["cost"][1] == cost1 and o["iterations"][0] == max(iters)
    # a point seen once moves along its ray only as far as the damping lets it and stays finite
    assert np.all(np.isfinite(o["points"]))
    # constant_point too: R1.1 is skipped, no residual block is left
    rc, z = bs.run_host(s, bs.cfg_of(constant_pose=1, constant_point=1))
    assert rc == 0 and z["code"][0] == 7 and np.array_equal(z["points"], s["p3"])
    # thread counts
    rc, o1 = bs.run_host(s, bs.cfg_of(constant_pose=1, max_num_iterations=30), 1)
    assert bs.same_bits(o, o1)


# ---- goldens (tests/golden/make_ba_golden.py) ----
def load_golden(path):
    """-> the scene, the configuration's keywords, the recorded outputs"""
    z = np.load(path)
    s = {k: np.ascontiguousarray(z[k]) for k in GOLDEN_IN}
    cfg = {k[4:]: z[k].item() for k in z.files if k.startswith("cfg_")}
    return s, cfg, {k[4:]: z[k] for k in z.files if k.startswith("out_")}


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "*.npz"))))
def test_goldens_reproduce(path):
    s, cfg, want = load_golden(path)
    rc, o = bs.run_host(s, bs.cfg_of(**cfg), 4)
    assert rc == 0 and set(o) == set(want)
    for k in o:
        assert np.array_equal(o[k], want[k]), (os.path.basename(path), k)


def test_goldens_exist():
    assert len(glob.glob(os.path.join(GOLDEN, "*.npz"))) >= 7


def test_no_residuals_is_code_7(hybrid):
    s = bs.without_lines(hybrid, [])
    rc, o = bs.run_host(s, bs.cfg_of(lw_point=0.0))
    assert rc == 0 and o["code"][0] == 7 and o["iterations"][0] == 0
    assert np.array_equal(o["qvec"], s["q"]) and np.array_equal(o["tvec"], s["t"]) and np.array_equal(o["points"], s["p3"])


def test_point_in_a_cameras_plane_is_code_6():
    s = bs.make_scene(n_cams=3, n_points=5, n_lines=0, seed=5)
    # an identity rotation and t = (0, 0, 5): the point (x, y, -5) has depth exactly 0 in that camera
    s["q"][0] = [1.0, 0.0, 0.0, 0.0]
    s["t"][0] = [0.0, 0.0, 5.0]
    s["p3"][2] = [0.3, 0.2, -5.0]
    rc, o = bs.run_host(s, bs.cfg_of())
    assert rc == 0 and o["code"][0] == 6 and o["iterations"][0] == 0 and not np.isfinite(o["cost"][0])
    assert np.array_equal(o["points"], s["p3"]) and np.array_equal(o["tvec"], s["t"])
    qn = np.array([ro.normalise_q(q, np.float64) for q in s["q"]])
    assert np.array_equal(o["qvec"], qn)


def test_argument_errors(L, hybrid):
    def err(s, **kw):
        rc, _ = bs.run_host(s, bs.cfg_of(**kw))
        assert rc != 0
        return L.lt_fn_ba_host_error().decode()
    assert "constant_intrinsics" in err(hybrid, constant_intrinsics=0)
    assert "constant_pose" in err(hybrid, constant_pose=1)
    big = bs.chain_scene(L.lt_ba_max_images() + 1, seed=6)
    assert "LT_BA_MAX_IMAGES" in err(big)
    assert L.lt_ba_max_images() >= 128
    bad = dict(hybrid); bad["pimg"] = hybrid["pimg"].copy(); bad["pimg"][3] = 999
    assert "not in the collection" in err(bad)
    bad = dict(hybrid); bad["pxy"] = hybrid["pxy"].copy(); bad["pxy"][0, 0] = np.nan
    assert "non-finite" in err(bad)
    bad = dict(hybrid); bad["line6"] = hybrid["line6"].copy(); bad["line6"][1, 3:] = bad["line6"][1, :3]
    assert "zero length" in err(bad)
    assert "constant_principal_point" not in err(hybrid, constant_intrinsics=0, constant_principal_point=0)
    rc, _ = bs.run_host(hybrid, bs.cfg_of(constant_principal_point=0, max_num_iterations=1))
    assert rc == 0  # accepted, no effect


# ---- 5. determinism ----
def test_two_runs_and_thread_counts_give_identical_bits(hybrid):
    cfg = bs.cfg_of(max_num_iterations=25)
    rc, a = bs.run_host(hybrid, cfg, 1)
    rc, b = bs.run_host(hybrid, cfg, 1)
    rc, c = bs.run_host(hybrid, cfg, 4)
    assert bs.same_bits(a, b) and bs.same_bits(a, c)
    assert a["iterations"][0] == 25


# ---- 6. the Python surface on the host path ----
def _py_scene(s):
    views = {int(i): CameraView(s["k"][n], s["q"][n], s["t"][n], image_name=f"im{int(i)}", hw=(600, 800)) for n, i in enumerate(s["img_ids"])}
    pts = [PointTrack(s["p3"][n], s["pimg"][a:b], list(range(a, b)), s["pxy"][a:b])
           for n, (a, b) in enumerate(zip(s["poff"][:-1], s["poff"][1:]))]
    lines = []
    for n, (a, b) in enumerate(zip(s["loff"][:-1], s["loff"][1:])):
        t = LineTrack(Line3d(s["line6"][n, :3], s["line6"][n, 3:]), [int(i) for i in s["limg"][a:b]], list(range(b - a)),
                      [Line2d(x) for x in s["l2d"][a:b]])
        t.line3d_list = [Line3d(x[:3], x[3:]) for x in s["l3d"][a:b]]
        lines.append(t)
    return ImageCollection(views), pts, lines


def test_python_surface(hybrid):
    imagecols, pts, lines = _py_scene(hybrid)
    cfg = dict(min_num_images=4, num_outliers_aggregator=2)
    with pytest.raises(ValueError, match="constant_intrinsics"):
        optimize.solve_hybrid_bundle_adjustment(cfg, imagecols, pts, lines, host_threads=1)
    # the runner's snippet (runners/hypersim/refine_sfm.py) and the one line it needs here
    cfg_ba = optimize.HybridBAConfig(cfg)
    cfg_ba.constant_intrinsics = True
    ba_engine = optimize.solve_hybrid_bundle_adjustment(cfg_ba, imagecols, pts, lines, max_num_iterations=20, host_threads=1)
    new_imagecols = ba_engine.GetOutputImagecols()
    rc, o = bs.run_host(hybrid, bs.cfg_of(max_num_iterations=20), 1)
    r = ba_engine.result()
    assert np.array_equal(r["qvec"], o["qvec"]) and np.array_equal(r["points"], o["points"]) and np.array_equal(r["cost_ba"], o["cost"])
    assert r["code"] == int(o["code"][0]) and r["iterations_ba"] == 20 and optimize.TERMINATION[7] == "no_residuals"
    # dicts as the second Init*Tracks overloads: the same solve
    e2 = optimize.solve_hybrid_bundle_adjustment(cfg_ba, imagecols, {10 + n: t for n, t in enumerate(pts)},
                                                 {20 + n: t for n, t in enumerate(lines)}, max_num_iterations=20, host_threads=1)
    assert sorted(e2.GetOutputPoints()) == [10 + n for n in range(len(pts))]
    assert np.array_equal(e2.result()["points"], r["points"]) and sorted(e2.GetOutputLineTracks(2)) == [20 + n for n in range(len(lines))]
    # point tracks from dicts (as_dict round trip)
    e3 = optimize.solve_point_bundle_adjustment(cfg_ba, imagecols, [PointTrack(t.as_dict()) for t in pts], max_num_iterations=5,
                                                host_threads=1)
    rc, o3 = bs.run_host(bs.without_lines(hybrid, []), bs.cfg_of(max_num_iterations=5), 1)
    assert np.array_equal(e3.result()["points"], o3["points"])
    # outputs
    out_pts, out_tracks = ba_engine.GetOutputPoints(), ba_engine.GetOutputPointTracks()
    assert np.array_equal(out_pts[3], o["points"][3]) and np.array_equal(out_tracks[3].p, o["points"][3])
    assert out_tracks[3].image_id_list == pts[3].image_id_list and out_tracks[3].count_images() == 4
    lt = ba_engine.GetOutputLineTracks(num_outliers=2)
    assert np.array_equal(np.concatenate([lt[1].line.start, lt[1].line.end]), o["segments"][1])
    assert len(ba_engine.GetOutputLineTracks(num_outliers=0)) == len(lines)
    # GetOutputImagecols round-trips through CameraView: the arrays a next call would send are the solved ones
    from limap_amd.triangulation import _view_arrays
    for n, i in enumerate(hybrid["img_ids"]):
        k, q, t = _view_arrays(new_imagecols.camview(int(i)))
        assert np.array_equal(q, o["qvec"][n]) and np.array_equal(t, o["tvec"][n]) and np.array_equal(k, hybrid["k"][n])
        assert new_imagecols.camview(int(i)).image_name() == f"im{int(i)}"
    assert not np.array_equal(_view_arrays(imagecols.camview(5))[2], o["tvec"][0])  # the input collection is a copy's source
    # above the image cap: a ValueError that names the constant, before any solve
    big_cols, big_pts, _ = _py_scene(bs.chain_scene(optimize.BA_MAX_IMAGES + 1, seed=6))
    with pytest.raises(ValueError, match="LT_BA_MAX_IMAGES"):
        optimize.solve_point_bundle_adjustment(cfg_ba, big_cols, big_pts, host_threads=1)
    # a length mismatch inside a track
    bad = PointTrack(pts[0].p, pts[0].image_id_list, pts[0].p2d_id_list, pts[0].p2d_list[:-1])
    with pytest.raises(ValueError, match="point track 0"):
        optimize.solve_point_bundle_adjustment(cfg_ba, imagecols, [bad], host_threads=1)


def test_constant_pose_line_tracks_delegate_bit_for_bit(hybrid):
    imagecols, pts, lines = _py_scene(hybrid)
    cfg_ba = optimize.HybridBAConfig(dict(min_num_images=3))
    cfg_ba.set_constant_camera()
    a = optimize.solve_hybrid_bundle_adjustment(cfg_ba, imagecols, {}, lines, max_num_iterations=30, host_threads=1)
    b = optimize.solve_line_bundle_adjustment(cfg_ba, imagecols, lines, max_num_iterations=30, host_threads=1)
    ra, rb = a.result(), b.result()
    for k in ("params", "segments", "cost", "iterations", "codes"):
        assert np.array_equal(ra[k], rb[k]), k
    assert np.all(rb["iterations"] > 0)
    v = a.GetOutputImagecols().camview(5)
    assert np.array_equal(v.tvec, imagecols.camview(5).tvec)
    # with point tracks too the tracks still separate: the same lines, every point its own solve, the views kept
    h = optimize.solve_hybrid_bundle_adjustment(cfg_ba, imagecols, pts, lines, max_num_iterations=30, host_threads=1)
    rh = h.result()
    for k in ("params", "segments", "cost", "iterations", "codes"):
        assert np.array_equal(rh[k], rb[k]), k
    rc, o = bs.run_host(bs.without_lines(hybrid, []), bs.cfg_of(constant_pose=1, max_num_iterations=30), 1)
    assert rc == 0 and np.array_equal(rh["points"], o["points"]) and not np.array_equal(o["points"], hybrid["p3"])
    assert np.array_equal(h.GetOutputPoints()[2], o["points"][2])
    assert np.array_equal(h.GetOutputImagecols().camview(8).tvec, imagecols.camview(8).tvec)
    only = optimize.solve_point_bundle_adjustment(cfg_ba, imagecols, pts, max_num_iterations=30, host_threads=1)
    assert np.array_equal(only.result()["points"], o["points"]) and only.GetOutputLineTracks(2) == {}
    # the existing rejections stay
    free = optimize.HybridBAConfig(dict(constant_intrinsics=True))
    with pytest.raises(ValueError, match="constant_pose"):
        optimize.solve_line_bundle_adjustment(free, imagecols, lines, host_threads=1)


def test_sanitizer_program_of_the_host_twin():
    """tools/ba_host_asan.cpp + lt_ba.cpp (host-only) under AddressSanitizer and UBSan, a program of its own"""
    from helpers import run_host_asan
    run_host_asan("ba_asan", "ba_host_asan")
