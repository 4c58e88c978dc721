"""The VP and the heatmap term of the line refinement (limap_amd.optimize) on the host, without a
GPU: the residual blocks through lt_fn_refine_eval_terms against the NumPy restatement (tests/refine_terms_oracle.py),
the branch fixtures, the whole step through lt_fn_refine_host_terms, the minimiser against a search that is not the code
under test, the Python surface on its host path and the goldens."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import refine_oracle as ro
import refine_scenes as rs
import refine_terms_oracle as to
import refine_terms_scenes as ts
from limap_amd import _capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refine_terms")
COUNTS = [1, 4, 5, 15, 16, 17, 33]  # around the group width of 16 lanes
KEYS = ("params", "segments", "cost", "iterations", "codes")


@pytest.fixture(scope="module")
def L():
    return _capi.load_library()


@pytest.fixture(scope="module")
def scene():
    return ts.make_scene(COUNTS, seed=1)


def by_id(s, dtype=np.float16):
    tex = ts.texels(s, dtype)
    return tex, dict(zip(map(int, tex[0]), tex[3]))


def same(a, b, what):
    for k in KEYS:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


TERM_CASES = {"vp": dict(use_geometric=False, use_vp=True), "heatmap": dict(use_geometric=False, use_heatmap=True),
              "all": dict(use_vp=True, use_heatmap=True)}


# ---- 1. residuals, cost, g, H ----
@pytest.mark.parametrize("case", sorted(TERM_CASES))
def test_blocks_against_longdouble(L, scene, case):
    """The criterion of test_refine_host.test_residual_and_derivatives_against_longdouble, here for the cost too (it
    comes from rf_cost_terms, another function than the linearisation, and the ratio test of the minimiser runs on it):
    E_ref is the FP64
    restatement's own maximum error against its longdouble evaluation over the fixture, per quantity relative to the
    larger of 1 and the quantity's largest magnitude in the track; ours stays within 4 E_ref (another operation order:
    one 3x6 matrix per support, block sums before the loss).  Condition, asserted from the restatement alone: every
    sample's row and column is at least 1e-6 px from an integer, so floor() is the same in both precisions.
    Fixture: the scene and its long-support variant (samples clamped on all four sides), FP16 texels.
    Measured: the figures this test prints."""
    kw = TERM_CASES[case]
    terms = ts.terms_struct(L, **{k: int(v) for k, v in kw.items()})
    E = dict(r=0.0, g=0.0, H=0.0, cost=0.0); Eref = dict(E)
    for s in (scene, ts.long_supports(scene)):
        _, arrs = by_id(s)
        for n in range(len(COUNTS)):
            cam, sg, flag, vp3, hms = ts.track_inputs(s, n, arrs)
            pp = ro.minimal(s["line6"][n])
            ours = ts.eval_ours(L, cam, sg, pp, terms, flag, vp3, hms)
            f64 = to.evaluate(cam, sg, pp, to.terms_of(**kw), flag, vp3, hms, 10.0, np.float64)
            ld = to.evaluate(cam, sg, pp, to.terms_of(**kw), flag, vp3, hms, 10.0, np.longdouble)
            assert not ours["failed"] and not ld["failed"]
            if kw.get("use_heatmap"):
                for e in (f64, ld):
                    assert np.abs(e["xy"] - np.round(e["xy"])).min() >= 1e-6, "a sample sits on a texel boundary"
            assert np.array_equal(np.isnan(ours["r"]), np.isnan(f64["r"])), "another set of blocks"
            for nm in E:
                want = np.nan_to_num(np.asarray(ld[nm], np.longdouble))
                scale = max(float(np.abs(want).max()), 1.0)
                E[nm] = max(E[nm], float(np.abs(np.nan_to_num(ours[nm]) - want).max()) / scale)
                Eref[nm] = max(Eref[nm], float(np.abs(np.nan_to_num(np.asarray(f64[nm])) - want).max()) / scale)
    print(f"refine terms eval error ({case}), ours:", E, "restatement:", Eref)
    for nm in ("r", "cost", "g", "H"):
        assert E[nm] <= 4 * Eref[nm], (nm, E[nm], Eref[nm])


# ---- 2. branch fixtures ----
def test_samples_outside_the_image_and_in_its_last_rows_and_columns(L, scene):
    s = ts.long_supports(scene)
    _, arrs = by_id(s)
    kw = dict(use_geometric=False, use_heatmap=True, n_samples_heatmap=11)
    terms = ts.terms_struct(L, use_geometric=0, use_heatmap=1, n_samples_heatmap=11)
    sides, last = np.zeros(4, bool), np.zeros(2, bool)
    for n in range(len(COUNTS)):
        cam, sg, flag, vp3, hms = ts.track_inputs(s, n, arrs)
        pp = ro.minimal(s["line6"][n])
        e = to.evaluate(cam, sg, pp, to.terms_of(**kw), flag, vp3, hms)
        for k in range(len(sg)):
            h, w = hms[k].shape
            x, y = e["xy"][k, :, 0], e["xy"][k, :, 1]
            sides |= [np.any(x < 0), np.any(x > w - 1), np.any(y < 0), np.any(y > h - 1)]
            last |= [np.any((np.floor(y) >= h - 2) & (np.floor(y) <= h - 1)), np.any((np.floor(x) >= w - 2) & (np.floor(x) <= w - 1))]
        o = ts.eval_ours(L, cam, sg, pp, terms, flag, vp3, hms)
        assert np.allclose(o["r"][:, 3:], e["r"][:, 3:], rtol=0, atol=1e-12) and np.allclose(o["g"], e["g"], rtol=1e-9, atol=1e-15)
        assert np.allclose(o["H"], e["H"], rtol=1e-9, atol=1e-15)
    assert sides.all(), "left, right, top, bottom"
    assert last.all(), "the +1 / +2 clamps of the last row and column"


def test_vp_labels_and_the_track_without_one(L, scene):
    flag = scene["vp_flag"]
    mixed = [n for n in range(len(COUNTS)) if 0 < flag[scene["off"][n]:scene["off"][n + 1]].sum() < COUNTS[n]]
    assert mixed, "no track with a label -1 among labelled supports"
    _, arrs = by_id(scene)
    n = mixed[0]
    cam, sg, fl, vp3, hms = ts.track_inputs(scene, n, arrs)
    o = ts.eval_ours(L, cam, sg, ro.minimal(scene["line6"][n]), ts.terms_struct(L, use_vp=1), fl, vp3, hms)
    assert np.array_equal(~np.isnan(o["r"][:, 2]), fl != 0)
    # no labelled support at all: the same bits as without use_vp, through the old kernel's twin and through the new one
    s = dict(scene, vp_flag=np.zeros_like(flag))
    tex = ts.texels(s)
    c = ts.cfg_struct(L, num_outliers_aggregator=0, min_num_images=1)
    for extra in (dict(), dict(use_heatmap=1)):
        rc, a = ts.run_host(L, s, c, ts.terms_struct(L, use_vp=1, **extra), tex)
        rc2, b = ts.run_host(L, s, c, ts.terms_struct(L, **extra), tex)
        assert rc == 0 and rc2 == 0
        same(a, b, extra)


def test_evaluation_failure_at_the_start(L, scene):
    f = ts.failing_track()
    tex, arrs = by_id(f)
    cam, sg, flag, vp3, hms = ts.track_inputs(f, 0, arrs)
    pp = ro.minimal(f["line6"][0])
    e = to.evaluate(cam, sg, pp, to.terms_of(use_heatmap=True), flag, vp3, hms)
    o = ts.eval_ours(L, cam, sg, pp, ts.terms_struct(L, use_heatmap=1), flag, vp3, hms)
    assert e["failed"] and o["failed"] and o["cost"] == np.inf
    m = ts.merge(scene, f)
    rc, r = ts.run_host(L, m, ts.cfg_struct(L, num_outliers_aggregator=0), ts.terms_struct(L, use_heatmap=1), ts.texels(m))
    assert rc == 0
    assert r["codes"][-1] == 6 and r["iterations"][-1] == 0 and np.all(r["codes"][:-1] != 6)
    assert np.array_equal(r["params"][-1], pp) and np.all(np.isinf(r["cost"][-1]))
    assert np.array_equal(r["segments"][-1], ro.cut(pp, f["l3d"], 0))
    from limap_amd import optimize
    assert optimize.TERMINATION[6] == "evaluation_failed"


def test_huber_inside_and_outside_its_threshold(L, scene):
    _, arrs = by_id(scene)
    cam, sg, flag, vp3, hms = ts.track_inputs(scene, 3, arrs)
    pp = ro.minimal(scene["line6"][3])
    kw = dict(use_geometric=False, use_heatmap=True)
    e = to.evaluate(cam, sg, pp, to.terms_of(**kw), flag, vp3, hms)
    assert e["huber_s"].min() > to.HUBER_A ** 2, "outside"
    c = ts.checker_heatmaps(scene)
    _, arrs2 = by_id(c)
    hms2 = ts.track_inputs(c, 3, arrs2)[4]
    e2 = to.evaluate(cam, sg, pp, to.terms_of(n_samples_heatmap=2, **kw), flag, vp3, hms2)
    assert 0 < e2["huber_s"].max() < to.HUBER_A ** 2 and np.abs(e2["g"]).max() > 0, "inside, with a gradient"
    for ee, hm, n in ((e, hms, 10), (e2, hms2, 2)):
        o = ts.eval_ours(L, cam, sg, pp, ts.terms_struct(L, use_geometric=0, use_heatmap=1, n_samples_heatmap=n), flag, vp3, hm)
        assert np.isclose(o["cost"], float(ee["cost"]), rtol=1e-12) and np.allclose(o["g"], ee["g"], rtol=1e-9, atol=1e-18)


def test_vp_sine_next_to_its_clamp(L, scene):
    s = ts.perpendicular_vps(scene)
    _, arrs = by_id(s)
    cam, sg, flag, vp3, hms = ts.track_inputs(s, 3, arrs)
    pp = ro.minimal(s["line6"][3])
    kw = dict(use_geometric=False, use_vp=True)
    e = to.evaluate(cam, sg, pp, to.terms_of(**kw), flag, vp3, hms)
    o = ts.eval_ours(L, cam, sg, pp, ts.terms_struct(L, use_geometric=0, use_vp=1), flag, vp3, hms)
    print("sines at the clamp: 1 - sine =", 1 - e["r"][:, 2])
    # |a x b|^2 + EPS with |a|, |b| = 1 / sqrt(1 + EPS) stays below 1 by about EPS: the branch `sine > 1` cannot be
    # reached with finite input, like the cosine's of the geometric term; its neighbourhood is pinned
    assert np.all(e["r"][:, 2] > 1 - 1e-11) and np.all(e["r"][:, 2] <= 1.0)
    assert np.allclose(o["r"][:, 2], e["r"][:, 2], rtol=0, atol=1e-15) and np.allclose(o["H"], e["H"], rtol=1e-6, atol=1e-18)


# ---- 3. no extra term: the old entry point ----
def test_neither_term_is_the_geometric_call(L):
    s = rs.make_tracks(40, seed=7)
    c = ts.cfg_struct(L, max_num_iterations=200)
    from test_refine_host import run_host as run_old
    rc, old = run_old(L, s, c, 4)
    rc2, new = ts.run_host(L, s, c, ts.terms_struct(L))
    assert rc == 0 and rc2 == 0
    same(old, new, "no term")


def test_argument_errors(L, scene):
    tex = ts.texels(scene)
    c = ts.cfg_struct(L, num_outliers_aggregator=0)

    def rc(terms, s=scene, tex=tex, **kw):
        return ts.run_host(L, s, c, ts.terms_struct(L, **terms), tex, **kw)[0]
    assert rc(dict(use_heatmap=1, use_vp=1)) == 0
    assert rc(dict(use_heatmap=1, n_samples_heatmap=1)) == -2
    assert rc(dict(use_vp=1, vp_multiplier=np.inf)) == -2
    assert rc(dict(use_heatmap=1, heatmap_multiplier=np.nan)) == -2
    assert rc(dict(use_heatmap=1, sample_range_max=np.inf)) == -2
    assert rc(dict(use_geometric=0)) == -2  # no term left
    bad = dict(scene, vp3=scene["vp3"].copy()); bad["vp3"][np.flatnonzero(scene["vp_flag"])[0], 1] = np.nan
    assert rc(dict(use_vp=1), bad) == -2
    few = tuple(x[1:] for x in tex)  # the first image supports tracks and has no heatmap
    assert int(tex[0][0]) in scene["img"] and rc(dict(use_heatmap=1), tex=few) == -2
    hw = dict(scene, hw=scene["hw"].copy()); hw["hw"][0, 0] += 1
    assert rc(dict(use_heatmap=1), hw) == -2 and rc(dict(use_heatmap=1), hw, view_hw=False) == 0
    assert rc(dict(use_heatmap=1, texel_type=_capi.TEXEL_F32), tex=ts.texels(scene, np.float32)) == 0
    assert ts.run_host(L, scene, c, ts.terms_struct(L, use_heatmap=1, texel_type=7), tex)[0] == -2
    zero = dict(scene, l2d=scene["l2d"].copy()); zero["l2d"][0, 2:] = zero["l2d"][0, :2]
    assert rc(dict(use_heatmap=1), zero) == -2


def test_float32_texels_and_thread_counts(L, scene):
    c = ts.cfg_struct(L, num_outliers_aggregator=0)
    t16, t32 = ts.texels(scene, np.float16), ts.texels(scene, np.float32)
    wide = (t16[0], t16[1], t16[2], [a.astype(np.float32) for a in t16[3]])  # the FP16 values as floats
    terms = dict(use_heatmap=1, use_vp=1)
    _, a = ts.run_host(L, scene, c, ts.terms_struct(L, **terms), t16, threads=1)
    _, b = ts.run_host(L, scene, c, ts.terms_struct(L, texel_type=_capi.TEXEL_F32, **terms), wide, threads=8)
    same(a, b, "the same values in both texel types")
    rc, d = ts.run_host(L, scene, c, ts.terms_struct(L, texel_type=_capi.TEXEL_F32, **terms), t32)
    assert rc == 0 and not np.array_equal(a["params"], d["params"]), "float texels keep what FP16 rounds away"


# ---- 4. the minimiser minimises ----
HEAT_ONLY = to.terms_of(use_geometric=False, use_heatmap=True)


def _scipy_track(job):
    """Nelder-Mead on the restatement's cost in the chart of the retraction, re-centred once (as test_refine_host does
    for the geometric term) -> the parameters it ends at"""
    from scipy.optimize import minimize
    cam_n, sg, flag, vp3, hms, p0 = job
    pp = np.array(p0, float)
    for _ in range(2):
        res = minimize(lambda dl: to.cost_only(cam_n, sg, ro.retract(pp, dl), HEAT_ONLY, flag, vp3, hms), np.zeros(4),
                       method="Nelder-Mead", options=dict(xatol=1e-9, fatol=1e-14, maxiter=400, maxfev=400, adaptive=True,
                                                          initial_simplex=np.vstack([np.zeros(4), 0.01 * np.eye(4)])))
        pp = ro.retract(pp, res.x)
    return pp


@pytest.fixture(scope="module")
def ridge_scene():
    return ts.make_scene([6] * 12, seed=5, sizes=((48, 64), (60, 80)), n_views=8, init_sigma=0.02, sigma_px=2.0, noise_px=0.3)


def _median_distance(s, segs):
    return float(np.median([ts.line_distance(segs[n], s["gt6"][n]) for n in range(len(segs))]))


def test_heatmap_term_pulls_the_lines_onto_the_ridges(L, ridge_scene):
    """Gaussian ridges (sigma 2 px) along the true projections, FP16 texels, initial endpoints off by N(0, 0.02):
    with use_geometric=False, use_heatmap=True the median distance of the refined lines to the GT lines is smaller
    than the initial lines', and no track's cost rises.  The same inequality holds for scipy's Nelder-Mead on the
    restatement's cost from the same initial lines, all twelve tracks (checked here).  Measured:
    medians 0.0197 initial, 0.0109 ours; scipy's is printed."""
    s = ridge_scene
    tex, arrs = by_id(s)
    rc, r = ts.run_host(L, s, ts.cfg_struct(L), ts.terms_struct(L, use_geometric=0, use_heatmap=1), tex)
    assert rc == 0
    d0, d1 = _median_distance(s, s["line6"]), _median_distance(s, r["segments"])
    print(f"heatmap only: median distance to GT initial {d0:.4f}, refined {d1:.4f}; codes {np.bincount(r['codes'], minlength=7)}")
    assert d1 < d0 and np.all(r["cost"][:, 1] <= r["cost"][:, 0])
    from concurrent.futures import ProcessPoolExecutor
    T = len(s["line6"])
    jobs = []
    for n in range(T):
        cam, sg, flag, vp3, hms = ts.track_inputs(s, n, arrs)
        cam_n = np.asarray(ro.cams_normalised(cam, np.float64))
        jobs.append((cam_n, sg, flag, vp3, hms, ro.minimal(s["line6"][n])))
        assert np.isclose(to.cost_only(cam_n, sg, r["params"][n], HEAT_ONLY, flag, vp3, hms), r["cost"][n, 1], rtol=1e-9)
    with ProcessPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        found = list(ex.map(_scipy_track, jobs))
    segs = np.array([ro.cut(found[n], s["l3d"][s["off"][n]:s["off"][n + 1]], 2) for n in range(T)])
    ds = _median_distance(s, segs)
    print(f"scipy (Nelder-Mead) on the restatement's cost, all {T} tracks: median distance initial {d0:.4f}, found {ds:.4f}")
    assert ds < d0


def test_vp_term_aligns_parallel_lines_with_their_vp(L):
    d = np.array([0.6, -0.3, 0.74]); d /= np.linalg.norm(d)
    s = ts.make_scene([6] * 10, seed=9, direction=d, init_sigma=0.03, vp_label_rate=1.0)
    rc, r = ts.run_host(L, s, ts.cfg_struct(L), ts.terms_struct(L, use_vp=1, vp_multiplier=100.0))
    assert rc == 0

    def spread(segs):
        v = segs[:, 3:] - segs[:, :3]
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        return float(np.median(np.degrees(np.arcsin(np.linalg.norm(np.cross(v, d), axis=1)))))
    a0, a1 = spread(s["line6"]), spread(r["segments"])
    print(f"VP term: median angle to the VP direction initial {a0:.3f} deg, refined {a1:.3f} deg")
    assert a1 < a0 and np.all(r["cost"][:, 1] <= r["cost"][:, 0])


# ---- 5. goldens ----
def load_golden(path):
    z = np.load(path)
    s = {k: np.ascontiguousarray(z[k]) for k in ("img_ids", "k", "q", "t", "hw", "line6", "off", "img", "l2d", "l3d", "vp_flag", "vp3")}
    ids = z["hm_ids"]
    tex = (ids, z["hm_h"], z["hm_w"], [np.ascontiguousarray(z[f"hm_{int(i)}"]) for i in ids])
    cfg = {k[4:]: z[k].item() for k in z.files if k.startswith("cfg_")}
    terms = {k[6:]: z[k].item() for k in z.files if k.startswith("terms_")}
    return s, tex, cfg, terms, {k: z["out_" + k] for k in KEYS}


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "*.npz"))))
def test_goldens_reproduce(L, path):
    s, tex, cfg, terms, want = load_golden(path)
    rc, r = ts.run_host(L, s, ts.cfg_struct(L, **cfg), ts.terms_struct(L, **terms), tex)
    assert rc == 0
    same(r, want, os.path.basename(path))


def test_goldens_exist():
    assert len(glob.glob(os.path.join(GOLDEN, "*.npz"))) >= 4


# ---- 6. Python surface (host path) ----
def _linetracks(s):
    from limap_amd.base import Line2d, Line3d, LineTrack
    out = []
    for n in range(len(s["line6"])):
        a, b = int(s["off"][n]), int(s["off"][n + 1])
        t = LineTrack(Line3d(s["line6"][n, :3], s["line6"][n, 3:]), s["img"][a:b].tolist(), list(range(a, b)),
                      [Line2d(x[:2], x[2:]) for x in s["l2d"][a:b]])
        t.line3d_list = [Line3d(x[:3], x[3:]) for x in s["l3d"][a:b]]
        out.append(t)
    return out


def _imagecols(s):
    from limap_amd.base import CameraView, ImageCollection
    return ImageCollection({int(i): CameraView(s["k"][n], s["q"][n], s["t"][n], hw=tuple(int(x) for x in s["hw"][n]))
                            for n, i in enumerate(s["img_ids"])})


CFG = dict(min_num_images=4, num_outliers_aggregate=2, use_geometric=True, geometric_alpha=10.0, use_vp=True, vp_multiplier=0.1,
           use_heatmap=True, sample_range_min=0.05, sample_range_max=0.95, n_samples_heatmap=10, heatmap_multiplier=1.0,
           use_feature=False, dtype="float16")


VP_CFG = dict(method="jlinkage", min_length=2.0, min_num_supports=3, num_hypotheses=200)


def test_runner_sequence_on_linetrack_lists(L, tmp_path):
    from limap_amd import optimize, vplib
    # parallel lines, 24 in every image (the detector wants 20): one VP per image
    s = ts.make_scene([8, 8, 8, 3] + [8] * 21, seed=21, direction=(0.6, -0.3, 0.74), sizes=((48, 64), (60, 80)))
    tracks, imagecols = _linetracks(s), _imagecols(s)
    # the runner: detect the vanishing points of every image's lines, save the heatmaps, refine
    all_lines = {int(i): [] for i in s["img_ids"]}
    for t in tracks:
        for k, i in enumerate(t.image_id_list):
            t.line_id_list[k] = len(all_lines[i])
            all_lines[i].append(t.line2d_list[k])
    # (the detector's host path: no device in this test; the device test runs get_vp_detector(...).detect_vp_all_images)
    vpresults = vplib.detect_vps_host(all_lines, VP_CFG, n_threads=2)
    assert sum(int(np.sum(np.asarray(v.labels) >= 0)) for v in vpresults.values()) >= 10, "the detector labels nothing"
    for i, a in s["heatmaps"].items():
        np.save(os.path.join(tmp_path, f"heatmap_{i}.npy"), a)
    out = optimize.line_refinement(dict(CFG), tracks, imagecols, heatmap_dir=str(tmp_path), vpresults=vpresults, host_threads=2)
    out2 = optimize.line_refinement(dict(CFG), tracks, imagecols, heatmaps=s["heatmaps"], vpresults=vpresults, host_threads=1)
    assert out[3] is tracks[3]  # three images: passes through
    moved = 0
    for n, t in enumerate(tracks):
        a, b = np.concatenate([out[n].line.start, out[n].line.end]), np.concatenate([out2[n].line.start, out2[n].line.end])
        assert np.array_equal(a, b), "heatmaps= is heatmap_dir="
        if t.count_images() < 4:
            continue
        moved += not np.array_equal(a, np.concatenate([t.line.start, t.line.end]))
        ids = t.GetSortedImageIds()
        e = optimize.solve_line_refinement(dict(CFG), t, [imagecols.camview(i) for i in ids], p_vpresults=[vpresults[i] for i in ids],
                                           p_heatmaps=[s["heatmaps"][i] for i in ids], host_threads=1)
        assert np.array_equal(np.concatenate([e.GetLine3d().start, e.GetLine3d().end]), a), "per track is the scene call"
    assert moved == 24
    # against the C entry point on the same arrays: labels -> flags
    flag = np.array([vpresults[i].labels[t.line_id_list[k]] >= 0 for t in tracks for k, i in enumerate(t.image_id_list)], np.int32)
    vp3 = np.array([vpresults[i].vps[vpresults[i].labels[t.line_id_list[k]]] if vpresults[i].labels[t.line_id_list[k]] >= 0
                    else np.zeros(3) for t in tracks for k, i in enumerate(t.image_id_list)]).reshape(-1, 3)
    s2 = dict(s, vp_flag=flag, vp3=np.ascontiguousarray(vp3))
    rc, r = ts.run_host(L, s2, ts.cfg_struct(L), ts.terms_struct(L, use_vp=1, use_heatmap=1, vp_multiplier=0.1), ts.texels(s))
    assert rc == 0
    for n in (0, 1, 2, 4, 24):
        assert np.array_equal(np.concatenate([out[n].line.start, out[n].line.end]), r["segments"][n])


def test_texel_types_and_rounding(L):
    from limap_amd import optimize
    s = ts.make_scene([5, 6], seed=22)
    tracks, imagecols = _linetracks(s), _imagecols(s)
    cfg = dict(CFG, use_vp=False)
    def lines(hm, **kw):
        out = optimize.line_refinement(dict(cfg, **kw), tracks, imagecols, heatmaps=hm, host_threads=1)
        return np.array([np.concatenate([t.line.start, t.line.end]) for t in out])
    f64 = s["heatmaps"]
    f32 = {i: a.astype(np.float32) for i, a in f64.items()}
    # float64 and float32 input with dtype float16: one astype(np.float16) of what was given
    assert np.array_equal(lines(f64), lines({i: a.astype(np.float16) for i, a in f64.items()}))
    assert np.array_equal(lines(f32), lines({i: a.astype(np.float16) for i, a in f32.items()}))
    ref = lines(f64)
    h = optimize.Heatmaps(s["heatmaps"], "float16")
    assert all(a.dtype == np.float16 and np.array_equal(a, s["heatmaps"][int(i)].astype(np.float16)) for i, a in zip(h.ids, h.arrays))
    assert np.array_equal(lines(f64, dtype="float32"), lines(f32, dtype="float32"))
    assert not np.array_equal(lines(f64, dtype="float32"), ref), "float texels keep what FP16 rounds away"
    with pytest.raises(ValueError, match="dtype"):
        optimize.line_refinement(dict(cfg, dtype="float64"), tracks, imagecols, heatmaps=s["heatmaps"], host_threads=1)


def test_value_errors_of_the_python_surface(L):
    from limap_amd import optimize
    s = ts.make_scene([5, 6], seed=22)
    tracks, imagecols = _linetracks(s), _imagecols(s)
    with pytest.raises(ValueError, match="use_vp"):
        optimize.line_refinement(dict(CFG), tracks, imagecols, heatmaps=s["heatmaps"], host_threads=1)
    with pytest.raises(ValueError, match="use_heatmap"):
        optimize.line_refinement(dict(CFG, use_vp=False), tracks, imagecols, host_threads=1)
    for key in ("use_vp", "use_heatmap", "use_feature"):
        with pytest.raises(ValueError, match=key):
            optimize.solve_line_bundle_adjustment(dict(use_geometric=True, constant_intrinsics=True, constant_pose=True, **{key: True}),
                                                  imagecols, tracks, host_threads=1)
    with pytest.raises(ValueError, match="use_feature"):
        optimize.line_refinement(dict(CFG, use_feature=True), tracks, imagecols, host_threads=1)
    with pytest.raises(ValueError, match="p_patches"):
        optimize.solve_line_refinement({}, tracks[0], [], p_patches=[1])
    with pytest.raises(ValueError, match="p_heatmaps"):
        optimize.solve_line_refinement({}, None, [], p_heatmaps=[1])
    with pytest.raises(ValueError, match="use_geometric"):
        optimize.line_refinement(dict(use_geometric=False), tracks, imagecols, host_threads=1)
    missing = {i: a for i, a in s["heatmaps"].items() if i != int(tracks[0].image_id_list[0])}
    with pytest.raises(ValueError, match="no heatmap"):
        optimize.line_refinement(dict(CFG, use_vp=False), tracks, imagecols, heatmaps=missing, host_threads=1)
    # use_geometric=False with another term on is allowed
    out = optimize.line_refinement(dict(CFG, use_vp=False, use_geometric=False), tracks, imagecols, heatmaps=s["heatmaps"], host_threads=1)
    assert not np.array_equal(out[0].line.start, tracks[0].line.start)
