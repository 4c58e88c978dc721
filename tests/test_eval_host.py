"""limap.evaluation without a GPU: the NumPy restatement (tests/eval_oracle.py) equals every output of the reference's own
code (tests/golden/eval/*.npz, make_eval_golden.py) bit for bit, and limap_amd.evaluation validates its inputs before
any launch."""
import glob
import os

import numpy as np
import pytest

import eval_oracle as eo
from limap_amd import evaluation as ev
from limap_amd.base import Line3d, LineTrack

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval")
FILES = sorted(glob.glob(os.path.join(GOLD, "eval_*.npz")))
N_SAMPLES = (1000, 37)


def load(name):
    return dict(np.load(os.path.join(GOLD, f"eval_{name}.npz")))


def same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def test_goldens_present():
    names = {os.path.basename(f) for f in FILES}
    assert {"eval_random.npz", "eval_edges.npz", "eval_single.npz", "eval_empty.npz"} <= names


@pytest.mark.parametrize("name", ["random", "edges", "single", "empty"])
def test_restatement_equals_reference(name):
    g = load(name)
    pts, lines, refl, th = g["points"], g["lines"].reshape(-1, 6), g["ref_lines"].reshape(-1, 6), g["thresholds"]
    assert same(eo.nearest_dists(pts, g["query_points"]), g["out_dist_points"])
    for n in (1000, 3):
        got = [eo.dist_line(pts, lines[k], n) for k in range(lines.shape[0])]
        assert same(np.array(got).reshape(-1), g[f"out_dist_line_{n}"].reshape(-1)), n
    for n in N_SAMPLES:
        assert same(eo.inlier_ratios(pts, lines, th, n).reshape(lines.shape[0], th.size), g[f"out_ratios_{n}"]), n
        assert same(eo.recall_length(refl, lines, th, n), g[f"out_recall_ref_{n}"]), n
        assert same(eo.recall_length(lines, refl, th, n), g[f"out_recall_tested_{n}"]), n
        for t_i in g["seg_th_idx"].tolist():
            for inl, key in ((True, "insegs"), (False, "outsegs")):
                assert same(eo.segs(pts, lines, th[t_i], n, inl), g[f"out_{key}_{t_i}_{n}"].reshape(-1, 6)), key
    assert same(eo.dists_for_each_point(pts, lines), g["out_dists_each"])
    assert same(eo.sum_length(refl), g["out_sum_length"])


def test_edge_scenes_cover_the_contract():
    g = load("edges")
    lines = g["lines"].reshape(-1, 6)
    assert (eo.length(lines) == 0).any() and (eo.length(g["ref_lines"].reshape(-1, 6)) == 0).any()
    pts = g["points"]
    assert len(np.unique(pts, axis=0)) < len(pts)  # duplicate points
    # thresholds equal to sampled distances: <= and < disagree there, and the goldens record which one is used
    d = eo.nearest_dists(pts, eo.samples_center(lines, 1000).reshape(-1, 3))
    th = g["thresholds"]
    assert any(((d == t).any() and t > 0) for t in th)
    le = np.stack([(d.reshape(len(lines), -1) <= t).sum(1) for t in th], 1) / 1000.0
    lt = np.stack([(d.reshape(len(lines), -1) < t).sum(1) for t in th], 1) / 1000.0
    assert same(le, g["out_ratios_1000"]) and not same(lt, g["out_ratios_1000"])
    assert load("single")["points"].shape == (1, 3)
    e = load("empty")
    assert e["lines"].size == 0 and (e["out_dists_each"] == np.finfo(np.float64).max).all()


def test_refline_distance_quirk_and_eps():
    """DistPointLine is the distance to the INFINITE line clipped by the endpoints' distances; below EPS it is 0"""
    a = np.array([[0.0, 0, 0, 1, 0, 0]])
    p = np.array([[3.0, 1.0, 0.0], [0.5, 1e-13, 0.0]])
    d = eo.dist_point_lines(p, a)
    assert d[0] == 1.0  # the segment distance would be sqrt(5)
    assert d[1] == 0.0
    assert eo.dists_for_each_point(p[:1], a)[0] == np.sqrt(5.0)


def test_line_inputs():
    a = np.array([[0.0, 1, 2, 3, 4, 5], [1, 1, 1, 2, 2, 2]])
    l3 = [Line3d(r[:3], r[3:]) for r in a]
    assert same(ev.lines_array(a), a)
    assert same(ev.lines_array(a.reshape(2, 2, 3)), a)
    assert same(ev.lines_array(l3), a)
    assert same(ev.lines_array([LineTrack(line=x) for x in l3]), a)
    assert ev.lines_array([]).shape == (0, 6)
    assert same(ev.line_lengths(a), eo.length(a))


def test_input_validation_before_any_launch():
    with pytest.raises(ValueError, match="empty"):
        ev.PointCloudEvaluator(np.zeros((0, 3)))
    with pytest.raises(ValueError, match="empty"):
        ev.PointCloudEvaluator([])
    with pytest.raises(ValueError, match="non-finite"):
        ev.PointCloudEvaluator(np.array([[0.0, 1.0, np.nan]]))
    with pytest.raises(ValueError, match="non-finite"):
        ev.PointCloudEvaluator(np.array([[0.0, 1.0, np.inf]], np.float32))
    e = ev.PointCloudEvaluator(np.zeros((4, 3)))  # constructing does not touch the device
    with pytest.raises(ValueError, match="non-finite"):
        e.ComputeInlierRatios(np.array([[0.0, 0, 0, np.nan, 0, 0]]), [0.1])
    with pytest.raises(ValueError, match="n_samples"):
        e.ComputeInlierRatios(np.zeros((1, 6)), [0.1], n_samples=0)
    with pytest.raises(ValueError, match="n_samples"):
        e.ComputeInlierSegs(np.zeros((1, 6)), 0.1, n_samples=-3)
    for n in (2, 1, 0):
        with pytest.raises(ValueError, match=">= 3"):
            e.ComputeDistLine(Line3d([0, 0, 0], [1, 0, 0]), n_samples=n)
    with pytest.raises(ValueError, match="non-finite"):
        e.ComputeDistPoint([np.inf, 0, 0])
    with pytest.raises(ValueError, match="64"):
        e.ComputeInlierRatios(np.zeros((1, 6)), np.zeros(65))
    r = ev.RefLineEvaluator(np.zeros((1, 6)))
    with pytest.raises(ValueError, match="n_samples"):
        r.ComputeRecallRef(np.zeros((1, 6)), 0.1, num_samples=0)
    with pytest.raises(ValueError, match="non-finite"):
        ev.RefLineEvaluator(np.array([[np.nan, 0, 0, 0, 0, 0]]))


def test_kdtree_name_raises():
    e = ev.PointCloudEvaluator(np.zeros((4, 3)))
    with pytest.raises(NotImplementedError, match="ComputeDistsforEachPoint"):
        e.ComputeDistsforEachPoint_KDTree([Line3d([0, 0, 0], [1, 0, 0])])


def test_load_rejects_foreign_files(tmp_path):
    e = ev.PointCloudEvaluator(np.zeros((4, 3)))
    f = tmp_path / "kdtree.bin"
    f.write_bytes(np.arange(40, dtype=np.uint64).tobytes())  # what a nanoflann index file starts like: raw sizes
    with pytest.raises(ValueError, match="nanoflann"):
        e.Load(str(f))


def test_sum_length_needs_no_device():
    g = load("random")
    assert same(ev.RefLineEvaluator(g["ref_lines"]).SumLength(), g["out_sum_length"])


def test_package_import_is_lazy():
    import limap_amd
    assert "evaluation" in limap_amd.__all__
    assert limap_amd.evaluation is ev
