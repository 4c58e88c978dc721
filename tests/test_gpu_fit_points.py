"""lt_fit_points (Fit3DPoints / estimate_seg3d on the GPU) against tests/fit_oracle.py, bit for bit: status, inlier set,
endpoint bits, iteration and LO counts."""
import numpy as np
import pytest

import fit_oracle as fo

pytestmark = pytest.mark.gpu


def _line_set(rng, n, noise=0.002, out_frac=0.2):
    t = rng.uniform(-1, 1, (n, 1))
    p = np.array([0.3, -1.2, 4.0]) + t * np.array([1.0, 0.4, -0.7]) + rng.normal(0, noise, (n, 3))
    m = rng.uniform(size=n) < out_frac
    p[m] += rng.normal(0, 0.5, (int(m.sum()), 3))
    return p


def _opts(**kw):
    from limap_amd import fitting
    o = fitting.LORansacOptions()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _check(sets, opt_kw, min_pct=0.0):
    from limap_amd import fitting
    r = fitting.fit_points_arrays(sets, _opts(**opt_kw), min_percentage_inliers=min_pct)
    for s, P in enumerate(sets):
        ref = fo.fit_points(P, fo.Options(**opt_kw), img_id=-1, line=s)
        where = f"set {s} (n={len(P)}, {opt_kw})"
        mask = r["inlier_mask"][r["off"][s]:r["off"][s + 1]]
        assert np.nonzero(mask)[0].tolist() == [int(i) for i in ref["inliers"]], where
        st = r["stats"][s]
        assert int(st[1]) == ref["best_num_inliers"], where
        assert int(st[2]) == ref["num_iterations"], f"{where}: iterations {st[2]} vs {ref['num_iterations']}"
        assert int(st[3]) == ref["number_lo_iterations"], where
        assert bool(st[4]) == ref["from_lo"], where
        ok = not (ref["inlier_ratio"] < min_pct)
        assert int(r["status"][s]) == (0 if ok else 2), where
        exp = np.stack([ref["start"], ref["end"]]) if ok else np.zeros((2, 3))
        assert np.array_equal(r["seg"][s].view(np.uint64), exp.view(np.uint64)), f"{where}: {r['seg'][s]} vs {exp}"
    return r


@pytest.mark.parametrize("n", [0, 1, 2, 6, 7, 63, 64, 65, 1000, 5000])
def test_sizes(n):
    rng = np.random.default_rng(n)
    _check([_line_set(rng, n)], dict(squared_inlier_threshold_=0.01 ** 2), min_pct=0.6)


def test_degenerate_sets():
    rng = np.random.default_rng(7)
    same = np.tile([[1.0, 2.0, 3.0]], (20, 1))
    dup = np.repeat(_line_set(rng, 10, 0.0, 0.0), 3, axis=0)
    coll = np.array([[0.0, 0.0, 0.0]]) + np.arange(30)[:, None] * np.array([[0.5, 0.25, -1.0]])
    nanp = _line_set(rng, 40)
    nanp[7, 1] = np.nan
    sets = [same, dup, coll, nanp, _line_set(rng, 50)]
    for kw in (dict(squared_inlier_threshold_=1e-4), dict(squared_inlier_threshold_=0.0),
               dict(squared_inlier_threshold_=1e-4, final_least_squares_=True)):
        _check(sets, kw, min_pct=0.6)


def test_isotropic_clump_lo_model_wins():
    flags = []
    for seed in range(12):
        rng = np.random.default_rng(100 + seed)
        clump = rng.normal(0, 1.0, (40, 3))
        r = _check([clump], dict(squared_inlier_threshold_=100.0, random_seed_=seed))
        flags.append(bool(r["stats"][0][4]))
    assert any(flags), "the least-squares model never won on an isotropic clump"


@pytest.mark.parametrize("kw", [
    dict(lo_starting_iterations_=0), dict(lo_starting_iterations_=50), dict(lo_starting_iterations_=500),
    dict(min_num_iterations_=37, max_num_iterations_=37), dict(num_lo_steps_=0), dict(final_least_squares_=True),
    dict(random_seed_=12345), dict(num_lsq_iterations_=1), dict(min_num_iterations_=300, max_num_iterations_=20),
])
def test_option_sweeps(kw):
    rng = np.random.default_rng(3)
    sets = [_line_set(rng, n) for n in (8, 30, 100, 300)]
    kw = dict(kw, squared_inlier_threshold_=0.01 ** 2)
    _check(sets, kw, min_pct=0.6)


def test_python_surface():
    from limap_amd import fitting
    rng = np.random.default_rng(11)
    P = _line_set(rng, 200)
    o = fitting.LORansacOptions()
    o.squared_inlier_threshold_ = 0.01 ** 2
    line, st = fitting.Fit3DPoints(P.T, o)
    ref = fo.fit_points(P, fo.Options(squared_inlier_threshold_=0.01 ** 2), img_id=-1, line=0)
    assert st.inlier_indices == [int(i) for i in ref["inliers"]]
    assert st.inlier_ratio == ref["inlier_ratio"] and st.num_iterations == ref["num_iterations"]
    assert np.array_equal(line.start, ref["start"]) and np.array_equal(line.end, ref["end"])
    r = fitting.estimate_seg3d(P.T, ransac_th=0.01, min_percentage_inliers=0.6)
    assert r is not None and np.array_equal(r[0], ref["start"])
    assert fitting.estimate_seg3d(P.T, ransac_th=0.01, min_percentage_inliers=0.99) is None
