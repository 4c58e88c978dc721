"""The geometric line refinement (limap_amd.optimize) on the host, without a GPU: limap's own part
through lt_fn_refine_eval / lt_fn_refine_minimal / lt_fn_refine_infinite against the NumPy restatement
(tests/refine_oracle.py), the module's exp and log against numpy, the minimiser through lt_fn_refine_host against
scipy, and the Python surface on its host path."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import refine_oracle as ro
import refine_scenes as rs
from limap_amd import _capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refine")
p = _capi.ptr


@pytest.fixture(scope="module")
def L():
    return _capi.load_library()


def cfg_of(L, **kw):
    c = _capi.LtRefineConfig()
    L.lt_refine_config_default(C.byref(c))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def run_host(L, s, cfg, threads=4):
    T = len(s["off"]) - 1
    P = np.zeros((T, 6)); seg = np.zeros((T, 6)); cost = np.zeros((T, 2))
    it = np.zeros(T, np.int32); code = np.zeros(T, np.int32)
    rc = L.lt_fn_refine_host(len(s["img_ids"]), p(s["img_ids"], C.c_int32), p(s["k"], C.c_double), p(s["q"], C.c_double),
                             p(s["t"], C.c_double), T, p(s["line6"], C.c_double), p(s["off"], C.c_int64),
                             p(s["img"], C.c_int32), p(s["l2d"], C.c_double), p(s["l3d"], C.c_double), C.byref(cfg),
                             threads, p(P, C.c_double), p(seg, C.c_double), p(cost, C.c_double), p(it, C.c_int32),
                             p(code, C.c_int32))
    return rc, dict(params=P, segments=seg, cost=cost, iterations=it, codes=code)


def eval_ours(L, cam, sg, pp, alpha=10.0):
    K = len(sg)
    cam, sg, pp = np.ascontiguousarray(cam), np.ascontiguousarray(sg), np.ascontiguousarray(pp)
    r = np.zeros(2 * K); c = C.c_double(); g = np.zeros(4); H = np.zeros(16)
    assert L.lt_fn_refine_eval(K, p(cam, C.c_double), p(sg, C.c_double), p(pp, C.c_double), alpha, p(r, C.c_double),
                               C.byref(c), p(g, C.c_double), p(H, C.c_double)) == 0
    return r, c.value, g, H.reshape(4, 4)


def minimal_ours(L, line6):
    out = np.zeros(6)
    assert L.lt_fn_refine_minimal(p(np.ascontiguousarray(line6, float), C.c_double), p(out, C.c_double)) == 0
    return out


# ---- 1. residual and derivatives ----
def test_residual_and_derivatives_against_longdouble(L):
    """E_ref: the FP64 restatement's own maximum error against its longdouble evaluation over the fixture, per quantity
    relative to the larger of 1 and the quantity's largest magnitude in the track (residuals are pixels: where a
    fixture puts them at zero, what is left is rounding of coordinates of a few hundred); ours must stay within 4 E_ref (the operation order
    differs: one 3x6 matrix per support instead of upstream's matrix products).  Measured: the
    figures this test prints."""
    s = rs.make_tracks(60, seed=1)
    cases = [rs.track_supports(s, n) + (ro.minimal(s["line6"][n]),) for n in range(60)]
    cases += [(c, sg, pp) for _, c, sg, pp in rs.edge_tracks()]
    E = dict(r=0.0, g=0.0, H=0.0, cost=0.0); Eref = dict(E)
    for cam, sg, pp in cases:
        ours = eval_ours(L, cam, sg, pp)
        f64 = ro.evaluate(cam, sg, pp, 10.0, np.float64)
        ld = ro.evaluate(cam, sg, pp, 10.0, np.longdouble)
        for nm, i in (("r", 0), ("cost", 1), ("g", 2), ("H", 3)):
            scale = max(float(np.abs(ld[i]).max()), 1.0)
            E[nm] = max(E[nm], float(np.abs(ours[i] - ld[i]).max()) / scale)
            Eref[nm] = max(Eref[nm], float(np.abs(f64[i] - ld[i]).max()) / scale)
    print("refine eval error, ours:", E, "restatement:", Eref)
    for nm in ("r", "g", "H"):
        assert E[nm] <= 4 * Eref[nm], (nm, E[nm], Eref[nm])


def test_edge_fixtures_take_the_intended_branches(L):
    ed = {n: (c, sg, pp) for n, c, sg, pp in rs.edge_tracks()}
    cam, sg, pp = ed["origin_parallel"]
    assert pp[5] == 0.0  # m = 0: the fallback basis, |w1| at 0
    r, cost, g, H = eval_ours(L, cam, sg, pp)
    assert np.all(np.isfinite(r)) and np.all(np.isfinite(g)) and np.all(np.isfinite(H))
    assert np.abs(r).max() < 1e-6  # the supports lie on the projection, cosine 1: weight exp(0)
    # d|w1|/dw1 = +1 at 0: moving along +dw and -dw gives the same line, the one-sided derivative is the +dw one
    rn = eval_ours(L, *ed["origin_parallel_noisy"])
    f64 = ro.evaluate(*ed["origin_parallel_noisy"], 10.0, np.float64)
    assert np.allclose(rn[2], f64[2], rtol=1e-9, atol=1e-12) and abs(rn[2][3]) > 0
    # perpendicular supports: weight exp(alpha (1 - cosine)) near exp(10)
    cam, sg, pp = ed["origin_perpendicular"]
    r, _, _, _ = eval_ours(L, cam, sg, pp)
    f = ro.evaluate(cam, sg, pp, 10.0, np.float64)
    assert np.allclose(r, f[0], rtol=1e-9) and np.abs(r).max() > 1e4
    # towards the clamp: supports parallel to the projection, beside it.  The cosine is |a . b| / (sqrt(|a|^2 + EPS)
    # sqrt(|b|^2 + EPS)) with |a| < 1 (dir2d is itself divided by a norm with EPS), so it stays below 1 by about
    # EPS / 2 = 5e-13, thousands of ulps: upstream's `cosine > 1` branch cannot be reached through the residual with
    # finite input.  What can be pinned is the neighbourhood: cosine within 1e-11 of 1, non-zero residuals, and r, g, H
    # equal to the restatement's, which carries the same clamp
    cam, sg, pp = ed["clamped"]
    r, _, g, H = eval_ours(L, cam, sg, pp)
    f = ro.evaluate(cam, sg, pp, 10.0, np.float64)
    u = [np.float64(x) for x in pp[:4]]; w = [np.float64(x) for x in pp[4:]]
    d, m = ro.plucker(u, w, np.float64)
    raw = []
    for k in range(len(sg)):
        co = ro.world_to_pixel(cam[k, :4], ro.normalise_q(cam[k, 4:8], np.float64), cam[k, 8:], d, m, np.float64)
        dn = np.sqrt(co[0] * co[0] + co[1] * co[1] + ro.EPS)
        a = [-co[1] / dn, co[0] / dn]; b = [sg[k, 2] - sg[k, 0], sg[k, 3] - sg[k, 1]]
        n1 = np.sqrt(a[0] * a[0] + a[1] * a[1] + ro.EPS); n2 = np.sqrt(b[0] * b[0] + b[1] * b[1] + ro.EPS)
        raw.append(abs((a[0] * b[0] + a[1] * b[1]) / (n1 * n2)))
    print("clamped fixture: unclamped cosines", raw)
    assert 1.0 - 1e-11 < max(raw) < 1.0 and np.abs(r).min() > 0.1
    assert np.allclose(r, f[0], rtol=1e-9) and np.allclose(g, f[2], rtol=1e-9) and np.allclose(H, f[3], rtol=1e-9)
    assert np.abs(g).max() > 0
    cam, sg, pp = ed["two_in_one_image"]
    assert np.array_equal(cam[0], cam[1])
    assert np.allclose(eval_ours(L, cam, sg, pp)[3], ro.evaluate(cam, sg, pp)[3], rtol=1e-9)


# ---- 2. exp / log ----
EXP_ULP_MEASURED, LOG_ULP_MEASURED = 1.146, 1.858  # the maxima this test measures


def test_lt_exp_and_lt_log_against_numpy(L):
    rng = np.random.default_rng(0)
    x = np.concatenate([np.linspace(0, 10, 100001), rng.uniform(0, 700, 100000), [0.0, 10.0, 700.0]])
    o = np.zeros_like(x)
    assert L.lt_fn_refine_explog(0, len(x), p(x, C.c_double), p(o, C.c_double)) == 0
    ref = np.exp(x.astype(np.longdouble))
    ulp_exp = float((np.abs(o - ref) / np.spacing(np.exp(x))).max())
    y = np.concatenate([1 + rng.uniform(0, 1, 100000) ** 3 * 1e3, np.exp(rng.uniform(0, 700, 100000)),
                        [1.0, 2.0, 1.7e308, 1 + 2.0 ** -52]])
    o = np.zeros_like(y)
    assert L.lt_fn_refine_explog(1, len(y), p(y, C.c_double), p(o, C.c_double)) == 0
    ref = np.log(y.astype(np.longdouble))
    ulp_log = float((np.abs(o - ref) / np.spacing(np.maximum(np.log(y), 1e-300))).max())
    print(f"lt_exp max ulp error {ulp_exp:.3f}, lt_log max ulp error {ulp_log:.3f}")
    assert o[-4] == 0.0 and x[0] == 0.0
    assert ulp_exp <= 2 * EXP_ULP_MEASURED and ulp_log <= 2 * LOG_ULP_MEASURED
    bad = np.array([-1.0])
    assert L.lt_fn_refine_explog(0, 1, p(bad, C.c_double), p(o, C.c_double)) == -2
    bad = np.array([0.5])
    assert L.lt_fn_refine_explog(1, 1, p(bad, C.c_double), p(o, C.c_double)) == -2


# ---- 3. conversions ----
def test_minimal_round_trips_the_pluecker_line(L):
    rng = np.random.default_rng(3)
    lines = [rng.uniform(-5, 5, 6) for _ in range(200)] + [np.array([-1.0, 0, 0, 1, 0, 0]), np.array([0, 0, -2.0, 0, 0, 3]),
                                                           np.array([0.0, 1e-14, 0, 1, 1e-14, 0])]
    for l in lines:
        pp = minimal_ours(L, l)
        assert np.array_equal(pp, ro.minimal(l)), l
        dm = np.zeros(6)
        assert L.lt_fn_refine_infinite(p(pp, C.c_double), p(dm, C.c_double)) == 0
        d = (l[3:] - l[:3]) / np.linalg.norm(l[3:] - l[:3])
        m = np.cross(l[:3], d)
        sgn = 1.0 if np.dot(dm[:3], d) > 0 else -1.0
        assert np.allclose(sgn * dm[:3], d, atol=1e-12) and np.allclose(sgn * dm[3:], m, atol=1e-11 * max(1, np.abs(m).max()))
        od, om = ro.infinite(pp)
        assert np.array_equal(dm[:3], od) and np.array_equal(dm[3:], om)
    zero = np.array([1.0, 2, 3, 1, 2, 3])
    assert L.lt_fn_refine_minimal(p(zero, C.c_double), p(np.zeros(6), C.c_double)) == -2


def _cut_scene():
    s = rs.make_tracks(30, seed=5)
    # ties: repeated 3D supports and identical endpoints
    a, b = int(s["off"][0]), int(s["off"][1])
    s["l3d"][a + 1] = s["l3d"][a]
    s["l3d"][a + 2, 3:] = s["l3d"][a + 2, :3]
    return s


def test_segment_cut_equals_the_sorted_selection(L):
    s = _cut_scene()
    kmin = int(np.diff(s["off"]).min())
    for n_out in (0, 1, 2, 2 * kmin - 1):  # the last one: the largest value legal for every track
        rc, r = run_host(L, s, cfg_of(L, num_outliers_aggregator=n_out, max_num_iterations=200))
        assert rc == 0
        for n in range(len(s["line6"])):
            a, b = int(s["off"][n]), int(s["off"][n + 1])
            want = ro.cut(r["params"][n], s["l3d"][a:b], n_out)
            assert np.array_equal(r["segments"][n], want), (n_out, n)
    rc, _ = run_host(L, s, cfg_of(L, num_outliers_aggregator=2 * kmin))
    assert rc == -2
    rc, _ = run_host(L, s, cfg_of(L, num_outliers_aggregator=-1))
    assert rc == -2


def test_constant_tracks_keep_their_parameters_and_get_the_recut_segment(L):
    s = _cut_scene()
    for kw in (dict(constant_line=1), dict(min_num_images=1000)):
        rc, r = run_host(L, s, cfg_of(L, **kw))
        assert rc == 0 and np.all(r["codes"] == 5) and np.all(r["iterations"] == 0)
        assert np.array_equal(r["cost"][:, 0], r["cost"][:, 1])
        for n in range(len(s["line6"])):
            a, b = int(s["off"][n]), int(s["off"][n + 1])
            pp = ro.minimal(s["line6"][n])
            assert np.array_equal(r["params"][n], pp)
            assert np.array_equal(r["segments"][n], ro.cut(pp, s["l3d"][a:b], 2))
            assert not np.array_equal(r["segments"][n], s["line6"][n])


def test_validation_returns_argument_errors(L):
    s = rs.make_tracks(5, seed=2)
    ok = cfg_of(L)
    assert run_host(L, s, ok)[0] == 0
    bad = dict(s); bad["line6"] = s["line6"].copy(); bad["line6"][2, 3:] = bad["line6"][2, :3]
    assert run_host(L, bad, ok)[0] == -2  # zero-length track line
    bad = dict(s); bad["off"] = s["off"].copy(); bad["off"][2] = bad["off"][1]
    assert run_host(L, bad, ok)[0] == -2  # a track without supports
    bad = dict(s); bad["img"] = s["img"].copy(); bad["img"][3] = 10 ** 6
    assert run_host(L, bad, ok)[0] == -2  # an image id that is not in the collection
    bad = dict(s); bad["l2d"] = s["l2d"].copy(); bad["l2d"][0, 0] = np.nan
    assert run_host(L, bad, ok)[0] == -2
    assert run_host(L, s, cfg_of(L, geometric_alpha=1e3))[0] == -2


def test_host_result_does_not_depend_on_threads_or_track_order(L):
    s = rs.make_tracks(40, seed=7)
    c = cfg_of(L, max_num_iterations=200)
    _, a = run_host(L, s, c, 1)
    _, b = run_host(L, s, c, 8)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    T = len(s["line6"])
    perm = np.random.default_rng(0).permutation(T)
    idx = np.concatenate([np.arange(s["off"][n], s["off"][n + 1]) for n in perm])
    sp = dict(s, line6=np.ascontiguousarray(s["line6"][perm]), img=np.ascontiguousarray(s["img"][idx]),
              off=np.concatenate([[0], np.cumsum(np.diff(s["off"])[perm])]).astype(np.int64),
              l2d=np.ascontiguousarray(s["l2d"][idx]), l3d=np.ascontiguousarray(s["l3d"][idx]))
    _, b = run_host(L, sp, c, 3)
    for k in a:
        assert np.array_equal(a[k][perm], b[k]), k


def test_edge_fixtures_through_the_whole_step(L):
    """one-track scenes from the edge fixtures: the fallback basis of rf_minimal (the line through the origin:
    wvec = (1, 0)), LM from the |x| kink, the cut; the results are pinned by a golden the device test replays"""
    s = rs.edge_scene()
    rc, r = run_host(L, s, cfg_of(L, min_num_images=1, max_num_iterations=200, num_outliers_aggregator=0))
    assert rc == 0
    n_origin = sum(1 for n, *_ in rs.edge_tracks() if n != "two_in_one_image")
    for n, (name, cam, sg, pp) in enumerate(rs.edge_tracks()):
        p0 = minimal_ours(L, s["line6"][n])
        assert np.array_equal(p0, pp), name
        assert np.all(np.isfinite(r["params"][n])) and np.all(np.isfinite(r["segments"][n])), name
        # (origin_perpendicular, weights near exp(10), is still moving at 200 iterations: code 0 is legal here)
        assert r["cost"][n, 1] <= r["cost"][n, 0] and r["codes"][n] in (0, 1, 2), (name, r["codes"][n])
        a, b = int(s["off"][n]), int(s["off"][n + 1])
        assert np.array_equal(r["segments"][n], ro.cut(r["params"][n], s["l3d"][a:b], 0)), name
    assert n_origin == 4 and np.all(s["line6"][:4, 1:3] == 0)


def test_cut_alone_and_nan_parameters(L):
    s = _cut_scene()
    _, r = run_host(L, s, cfg_of(L))
    a, b = int(s["off"][0]), int(s["off"][1])
    l3 = np.ascontiguousarray(s["l3d"][a:b]); seg = np.zeros(6)
    for n_out in (0, 1, 2):
        pp = np.ascontiguousarray(r["params"][0])
        assert L.lt_fn_refine_cut(b - a, p(l3, C.c_double), p(pp, C.c_double), n_out, p(seg, C.c_double)) == 0
        assert np.array_equal(seg, ro.cut(pp, l3, n_out))
    assert L.lt_fn_refine_cut(b - a, p(l3, C.c_double), p(pp, C.c_double), 2 * (b - a), p(seg, C.c_double)) == -2
    bad = np.array([1.0, 0, 0, 0, 0.0, 1.0])  # wvec[0] = 0: m is infinite, the values are NaN
    assert L.lt_fn_refine_cut(b - a, p(l3, C.c_double), p(bad, C.c_double), 1, p(seg, C.c_double)) == 0
    assert np.all(np.isnan(seg))


# ---- 4. the minimiser minimises ----
def _scipy_min(cam_n, sg, p0):
    from scipy.optimize import minimize
    pp = np.array(p0, float)
    for _ in range(2):  # re-centre the local chart; derivative-free: BFGS on difference quotients stalls on this cost
        res = minimize(lambda dl: ro.cost_only(cam_n, sg, ro.retract(pp, dl)), np.zeros(4), method="Nelder-Mead",
                       options=dict(xatol=1e-13, fatol=1e-16, maxiter=3000, maxfev=3000, adaptive=True))
        pp = ro.retract(pp, res.x)
    return pp, ro.cost_only(cam_n, sg, pp)


def _scipy_track(job):
    """(cost of our solution on the restated cost, scipy from the initial line, from the GT line, from ours)"""
    cam, sg, line6, gt6, ours = job
    cam_n = np.asarray(ro.cams_normalised(cam, np.float64))
    return (ro.cost_only(cam_n, sg, ours), _scipy_min(cam_n, sg, ro.minimal(line6))[1],
            _scipy_min(cam_n, sg, ro.minimal(gt6))[1], _scipy_min(cam_n, sg, ours)[1])


def test_minimiser_reaches_the_minimum_scipy_finds(L):
    """Fixture: 200 tracks, 0.1 px endpoint noise, initial endpoints off by 0.002: one basin, which this test checks --
    scipy (Nelder-Mead on the restated cost, in the chart of the retraction) reaches the same cost from the initial line
    and from the GT line.  The margin is scipy's own spread between its two starts, times 10; measured on this
    fixture: spread 8.0e-12, polishing lowers our cost by at most 4.6e-11 of it (both printed)."""
    from concurrent.futures import ProcessPoolExecutor
    s = rs.make_tracks(200, seed=12, noise_px=0.1, init_sigma=0.002)
    rc, r = run_host(L, s, cfg_of(L, max_num_iterations=200))
    assert rc == 0
    codes, iters, cost = r["codes"], r["iterations"], r["cost"]
    print("termination codes", np.bincount(codes, minlength=6), "iterations min/median/max", iters.min(),
          np.median(iters), iters.max())
    assert not np.any(codes == 0), "max_num_iterations exit at 200"
    assert np.all(cost[:, 1] <= cost[:, 0])
    assert np.all(np.isin(codes, (1, 2, 5)))
    opt = np.flatnonzero(codes != 5)
    assert len(opt) > 150 and np.all(iters[opt] >= 1) and np.all(iters[opt] < 120) and np.all(iters[codes == 5] == 0)
    jobs = [rs.track_supports(s, n) + (s["line6"][n], s["gt6"][n], r["params"][n]) for n in opt]
    with ProcessPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        rows = np.array(list(ex.map(_scipy_track, jobs, chunksize=4)))
    ours, c_init, c_gt, c_pol = rows.T
    assert np.allclose(ours, cost[opt, 1], rtol=1e-10, atol=0), "the restated cost at our solution is not our cost"
    spread = float((np.abs(c_init - c_gt) / np.maximum(c_init, c_gt)).max())
    margin = 10 * spread
    print(f"scipy spread between its two starts {spread:.3e}, margin {margin:.3e}; polishing lowers ours by at most "
          f"{float(((ours - c_pol) / ours).max()):.3e}; ours above scipy's best by at most "
          f"{float(((ours - np.minimum(c_init, c_gt)) / ours).max()):.3e}")
    assert spread < 1e-9, "the fixture is not one basin"
    assert np.all(c_pol >= ours * (1 - margin)), "polishing from our solution lowered the cost"
    assert np.all(ours <= np.minimum(c_init, c_gt) * (1 + margin)), "scipy found a lower cost from the initial / GT line"


# ---- goldens ----
@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "*.npz"))))
def test_goldens_reproduce(L, path):
    z = np.load(path)
    s = {k: z[k] for k in ("img_ids", "k", "q", "t", "line6", "off", "img", "l2d", "l3d")}
    c = cfg_of(L, **{k[4:]: z[k].item() for k in z.files if k.startswith("cfg_")})
    rc, r = run_host(L, s, c)
    assert rc == 0
    for k in r:
        assert np.array_equal(r[k], z["out_" + k]), k


def test_goldens_exist():
    assert len(glob.glob(os.path.join(GOLDEN, "*.npz"))) >= 7


# ---- 5. Python surface (host path) ----
def _linetracks(s):
    from limap_amd.base import Line2d, Line3d, LineTrack
    out = []
    for n in range(len(s["line6"])):
        a, b = int(s["off"][n]), int(s["off"][n + 1])
        t = LineTrack(Line3d(s["line6"][n, :3], s["line6"][n, 3:]), s["img"][a:b].tolist(), list(range(b - a)),
                      [Line2d(x[:2], x[2:]) for x in s["l2d"][a:b]])
        t.line3d_list = [Line3d(x[:3], x[3:]) for x in s["l3d"][a:b]]
        out.append(t)
    return out


REFINEMENT_CFG = dict(disable=False, constant_intrinsics=True, constant_principal_point=True, constant_pose=True,
                      constant_line=False, min_num_images=4, num_outliers_aggregator=2, use_geometric=True,
                      geometric_alpha=10.0, use_vp=False, vp_multiplier=0.1, use_heatmap=False, use_feature=False)


def test_runner_snippet_on_linetrack_lists(L):
    from limap_amd import optimize
    from limap_amd.base import ImageCollection
    s = rs.make_tracks(30, seed=13)
    imagecols = ImageCollection.from_arrays(s["img_ids"], s["k"], s["q"], s["t"])
    linetracks = _linetracks(s)
    cfg = {"refinement": dict(REFINEMENT_CFG)}
    cfg_ba = optimize.HybridBAConfig(cfg["refinement"]); cfg_ba.set_constant_camera()
    ba_engine = optimize.solve_line_bundle_adjustment(cfg["refinement"], imagecols, linetracks, max_num_iterations=200,
                                                      host_threads=2)
    linetracks_map = ba_engine.GetOutputLineTracks(num_outliers=cfg["refinement"]["num_outliers_aggregator"])
    new = [track for (track_id, track) in linetracks_map.items()]
    _, r = run_host(L, s, cfg_of(L, max_num_iterations=200))
    assert sorted(linetracks_map) == list(range(30))
    for n, t in enumerate(new):
        assert np.array_equal(np.concatenate([t.line.start, t.line.end]), r["segments"][n])
        assert t.image_id_list == linetracks[n].image_id_list and len(t.line3d_list) == len(linetracks[n].line3d_list)
    lines = ba_engine.GetOutputLines(2)
    assert np.array_equal(lines[3].start, new[3].line.start)
    # the per-track entry points: RefinementConfig's max_num_iterations is 100
    _, r = run_host(L, s, cfg_of(L, max_num_iterations=100))
    out = optimize.line_refinement(dict(REFINEMENT_CFG), linetracks, imagecols, n_visible_views=4, host_threads=2)
    for n, t in enumerate(linetracks):
        if t.count_images() >= 4:
            assert np.array_equal(np.concatenate([out[n].line.start, out[n].line.end]), r["segments"][n])
            views = [imagecols.camview(i) for i in t.GetSortedImageIds()]
            e = optimize.solve_line_refinement(dict(REFINEMENT_CFG), t, views, host_threads=1)
            assert np.array_equal(e.GetLine3d().start, out[n].line.start)
        else:
            assert out[n] is t
            assert optimize.solve_line_refinement(dict(REFINEMENT_CFG), t, [], host_threads=1) is None


@pytest.mark.parametrize("key,value", [("constant_intrinsics", False), ("constant_pose", False), ("use_vp", True),
                                       ("use_heatmap", True), ("use_feature", True)])
def test_unsupported_keys_raise(key, value):
    from limap_amd import optimize
    from limap_amd.base import ImageCollection
    s = rs.make_tracks(3, seed=1)
    imagecols = ImageCollection.from_arrays(s["img_ids"], s["k"], s["q"], s["t"])
    cfg = dict(REFINEMENT_CFG); cfg[key] = value
    with pytest.raises(ValueError, match=key):
        optimize.solve_line_bundle_adjustment(cfg, imagecols, _linetracks(s), host_threads=1)
    if key.startswith("use_"):
        with pytest.raises(ValueError, match=key):
            optimize.line_refinement(cfg, _linetracks(s), imagecols, host_threads=1)


def test_default_config_has_cameras_free_like_upstream_and_is_rejected():
    from limap_amd import optimize
    c = optimize.HybridBAConfig()
    assert (c.constant_intrinsics, c.constant_pose, c.min_num_images, c.geometric_alpha) == (False, False, 4, 10.0)
    with pytest.raises(ValueError, match="constant_intrinsics"):
        c._check()
    c.set_constant_camera()
    c._check()
    with pytest.raises(ValueError, match="p_vpresults"):
        optimize.solve_line_refinement({}, None, [], p_vpresults=[1])
