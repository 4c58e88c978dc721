"""CPU checks of the line fitter's contract (no GPU): the Bresenham restatement and its closed form, the oracle's front
half against the reference's NumPy formula, the options and NumRequiredIterations, the oracle on noise-free walls, the
C ABI surface and the argument checks the Python layer makes before any device work."""
import math
import os
import re

import numpy as np
import pytest

import fit_oracle as fo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bresenham_is_8_connected_monotone_and_ends_on_both_endpoints():
    rng = np.random.default_rng(0)
    for _ in range(300):
        x0, y0, x1, y1 = (int(v) for v in rng.integers(-60, 60, 4))
        px = fo.bresenham_seq(x0, y0, x1, y1)
        assert px[0] == (x0, y0) and px[-1] == (x1, y1)
        assert len(px) == max(abs(x1 - x0), abs(y1 - y0)) + 1
        for (a, b), (c, d) in zip(px, px[1:]):
            assert max(abs(c - a), abs(d - b)) == 1
        xs, ys = [p[0] for p in px], [p[1] for p in px]
        assert xs == sorted(xs) or xs == sorted(xs, reverse=True)
        assert ys == sorted(ys) or ys == sorted(ys, reverse=True)


def test_bresenham_closed_form_equals_the_recurrence():
    for dx in range(-40, 41):
        for dy in range(-40, 41):
            seq = fo.bresenham_seq(5, -3, 5 + dx, -3 + dy)
            assert [fo.bresenham_closed(5, -3, 5 + dx, -3 + dy, i) for i in range(len(seq))] == seq, (dx, dy)


def test_raster_equals_the_filtered_sequence():
    rng = np.random.default_rng(1)
    w, h = 37, 23
    for _ in range(500):
        s = rng.uniform(-30, 70, 4)
        px, py = fo.raster(s, w, h)
        seq = [(x, y) for x, y in fo.bresenham_seq(*(int(v) for v in s)) if 0 <= x < w and 0 <= y < h]
        assert list(zip(px.tolist(), py.tolist())) == seq


def _view(seed):
    from limap_amd import base
    rng = np.random.default_rng(seed)
    q = rng.normal(size=4)
    return base.CameraView([300.0 + seed, 310.0, 80.5, 61.25], q, rng.normal(size=3))


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.uint16])
def test_front_half_against_the_reference_formula(dtype):
    rng = np.random.default_rng(2)
    h, w = 120, 160
    view = _view(3)
    depth = rng.uniform(0.5, 9.0, (h, w))
    if dtype == np.uint16:
        depth = rng.integers(1, 5000, (h, w)).astype(np.uint16)
    else:
        depth = depth.astype(dtype)
        depth[rng.uniform(size=(h, w)) < 0.2] = np.inf
    n_cmp = 0
    for _ in range(60):
        s = rng.uniform(-40, 200, 4)
        ref = fo.ref_front_half(s, depth, view.K(), view.R(), view.T(), 5.0, 0.75)
        got = fo.front_half(s, depth, view.kvec, view._qvec_given, view.tvec, 5.0, 0.75)
        assert np.array_equal(got["px"], ref["px"]) and np.array_equal(got["py"], ref["py"])
        assert np.array_equal(got["depth"], ref["depth"])
        if ref["median"] is None:
            assert got["points"] is None
            continue
        n_cmp += 1
        assert got["median"] == ref["median"] and np.asarray(got["median"]).dtype == np.asarray(ref["median"]).dtype
        assert np.float64(0.75 * got["unc"]).tobytes() == np.float64(ref["th"]).tobytes()
        scale = np.maximum(1.0, np.linalg.norm(ref["points"], axis=1))[:, None]
        assert np.all(np.abs(got["points"] - ref["points"]) <= 1e-14 * scale * 8)
    assert n_cmp > 20


def test_float32_median_of_an_even_count_is_taken_in_float32():
    d = np.array([1.0000001, 1.0000002, 3.0, 7.0], np.float32)
    assert fo.median_of(d) == np.median(d) and fo.median_of(d).dtype == np.float32
    d = np.array([np.float32(16777216.0), np.float32(16777218.0)], np.float32)
    assert fo.median_of(d) == np.median(d)


def test_options_fields_and_defaults():
    from limap_amd import fitting
    o = fitting.LORansacOptions()
    assert (o.min_num_iterations_, o.max_num_iterations_, o.success_probability_) == (100, 10000, 0.9999)
    assert (o.num_lo_steps_, o.num_lsq_iterations_, o.min_sample_multiplicator_) == (10, 4, 7)
    assert (o.non_min_sample_multiplier_, o.lo_starting_iterations_, o.final_least_squares_) == (3, 50, False)
    assert o.threshold_multiplier_ == math.sqrt(2.0) and o.random_seed_ == 0
    assert vars(o).keys() == vars(fo.Options()).keys()


def test_num_required_iterations_edges():
    f = fo.num_required_iterations
    assert f(0.0, 1e-4, 2, 100, 10000) == 10000
    assert f(-1.0, 1e-4, 2, 100, 10000) == 10000
    assert f(1.0, 1e-4, 2, 100, 10000) == 100
    assert f(1e-8, 1e-4, 2, 100, 10000) == 10000  # 1 - r^2 >= 0.99999999999999
    assert f(0.5, 1e-4, 2, 0, 10000) == math.ceil(math.log(1e-4) / math.log(0.75) + 0.5)
    assert f(0.5, 1e-4, 2, 100, 10000) == 100
    assert f(0.01, 1e-4, 2, 0, 1000) == 1000
    assert f(0.9, 0.0, 2, 5, 777) == 777  # log(0) = -inf: as many as allowed
    assert f(0.9, 1.0, 2, 0, 777) == 1
    for x in (1e-300, 1e-4, 0.37, 0.9999, 1.0, 2.0, 1e300):
        assert abs(fo.lt_log(x) - math.log(x)) <= 4e-16 * max(1.0, abs(math.log(x)))


def test_oracle_recovers_noise_free_wall_lines():
    """a horizontal image segment on a wall: its pixels unproject onto the wall plane and the plane of the image row,
    so the fitted segment lies on their intersection line"""
    from limap_amd import synthetic as syn
    base_sc = syn.make_scene(n_views=2, n_segs=4, n_neighbors=1, seed=5)
    h, w = 90, 120
    sc = syn.resize_scene(base_sc, h, w)
    depths = syn.render_depths(base_sc, h, w, dtype=np.float64)
    n_ok = 0
    for n, i in enumerate(sc.img_ids):
        R = fo.cam_R(sc.qvec[n])
        R = np.array(R).reshape(3, 3)
        Cc = -R.T @ sc.tvec[n]
        fx, fy, cx, cy = sc.kvec[n]
        for y in (10, 30, 45, 60, 80):
            for x0, x1 in ((2.0, 40.0), (40.0, 80.0), (80.0, w - 3.0)):
                seg = [x0, y, x1, y]
                fh = fo.front_half(seg, depths[int(i)], sc.kvec[n], sc.qvec[n], sc.tvec[n])
                if fh["points"] is None:
                    continue
                P = fh["points"]
                walls = np.stack([np.abs(P[:, 0]), np.abs(P[:, 0] - 10.0), np.abs(P[:, 1]), np.abs(P[:, 1] - 8.0),
                                  np.abs(P[:, 2]), np.abs(P[:, 2] - 3.0)], 1)
                wall = np.argmin(walls, 1)
                if not (wall == wall[0]).all():
                    continue  # the row crosses a corner
                r = fo.fit_segment(seg, depths[int(i)], sc.kvec[n], sc.qvec[n], sc.tvec[n], int(i), 0, fo.Options())
                assert r["status"] == 0 and r["inliers"] == len(P)
                row_n = R.T @ np.cross([1.0, 0.0, 0.0], [0.0, (y - cy) / fy, 1.0])  # the row's plane (world)
                for p in r["seg"]:
                    assert abs(row_n @ (p - Cc)) <= 1e-9 * max(1.0, np.linalg.norm(p - Cc))
                    assert walls.shape[1] == 6
                    plane = [p[0], p[0] - 10.0, p[1], p[1] - 8.0, p[2], p[2] - 3.0][wall[0]]
                    assert abs(plane) <= 1e-9
                n_ok += 1
    assert n_ok >= 4


def test_header_and_library_symbols():
    text = open(os.path.join(ROOT, "include", "limap_amd.h")).read()
    for sig in (r"int lt_fit_segs\(lt_ctx \*ctx, int img_begin, int n_maps, const lt_depth_map \*maps",
                r"int lt_fit_points\(lt_ctx \*ctx, int64_t n_sets, const int64_t \*off, const double \*xyz",
                r"int lt_fit_get_timers\(lt_ctx \*ctx, double out\[4\]\)",
                r"void lt_fit_config_default\(lt_fit_config \*cfg\)", r"typedef struct lt_fit_config",
                r"typedef struct lt_depth_map"):
        assert re.search(sig, text), sig
    from limap_amd import _capi
    L = _capi.load_library()
    for name in ("lt_fit_segs", "lt_fit_points", "lt_fit_get_timers", "lt_fit_config_default"):
        assert hasattr(L, name) and name in _capi.EXPORTED_SYMBOLS
    c = _capi.LtFitConfig()
    L.lt_fit_config_default(c)
    o = fo.Options()
    assert (c.min_num_iterations, c.max_num_iterations, c.num_lo_steps, c.lo_starting_iterations) == (100, 10000, 10, 50)
    assert c.threshold_multiplier == o.threshold_multiplier_ and c.success_probability == 0.9999
    assert (c.ransac_th, c.min_percentage_inliers, c.var2d, c.seed) == (0.75, 0.6, 5.0, 0)


def test_argument_errors_before_device_work():
    from limap_amd import base, fitting
    bad = fitting.LORansacOptions()
    bad.success_probability_ = 1.5
    with pytest.raises(ValueError):
        fitting.fit_points_arrays([np.zeros((5, 3))], bad)
    bad = fitting.LORansacOptions()
    bad.max_num_iterations_ = -1
    with pytest.raises(ValueError):
        fitting.Fit3DPoints(np.zeros((3, 5)), bad)
    with pytest.raises(ValueError):
        fitting.Fit3DPoints(np.zeros((5, 3)), fitting.LORansacOptions())
    ic = base.ImageCollection({3: base.CameraView([100.0, 100.0, 50.0, 40.0], [1.0, 0, 0, 0], [0.0, 0, 0])})
    segs = {3: np.array([[1.0, 2.0, 30.0, 20.0]])}
    with pytest.raises(ValueError):
        fitting.fit_3d_segs_arrays(segs, ic, {3: np.ones((80, 100), np.float16)})
    with pytest.raises(ValueError):
        fitting.fit_3d_segs_arrays(segs, ic, {3: np.ones((80, 100, 2), np.float32)})
    with pytest.raises(ValueError):
        fitting.fit_3d_segs_arrays({3: np.array([[np.nan, 2.0, 30.0, 20.0]])}, ic, {3: np.ones((80, 100))})
    with pytest.raises(KeyError):
        fitting.fit_3d_segs_arrays(segs, ic, {4: np.ones((80, 100))})
    with pytest.raises(ValueError):
        fitting.fit_3d_segs_arrays(segs, ic, {3: np.ones((80, 100))}, dict(ransac_th=float("nan")))
    with pytest.raises(ValueError):
        fitting.estimate_seg3d_from_depth(segs[3][0], np.ones((80, 100), np.float16), ic.camview(3))
