"""limap_amd.evaluation on the device: bit-for-bit against the reference's goldens (tests/golden/eval) and against the NumPy
restatement (tests/eval_oracle.py), zero tolerance, on scenes that stress the index (degenerate boxes, far clusters, far
queries, a 10^6-point cloud, chunk edges) and through every input form."""
import os

import numpy as np
import pytest

import eval_oracle as eo

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval")


@pytest.fixture(scope="module")
def ev():
    from limap_amd import evaluation
    return evaluation


def same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def rand_lines(rng, n, lo, hi, max_len):
    s = rng.uniform(lo, hi, (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([s, s + d * rng.uniform(0.0, max_len, (n, 1))], 1)


@pytest.mark.parametrize("name", ["random", "edges", "single", "empty"])
def test_device_equals_reference_goldens(ev, name):
    from limap_amd.base import Line3d
    g = dict(np.load(os.path.join(GOLD, f"eval_{name}.npz")))
    pts, lines, refl, th = g["points"], g["lines"].reshape(-1, 6), g["ref_lines"].reshape(-1, 6), g["thresholds"]
    E = ev.PointCloudEvaluator(pts)
    E.Build()
    assert same(E.ComputeDistPoints(g["query_points"]), g["out_dist_points"])
    assert same([E.ComputeDistPoint(q) for q in g["query_points"][:5]], g["out_dist_points"][:5])
    l3 = [Line3d(r[:3], r[3:]) for r in lines]
    for n in (1000, 3):
        assert same(np.array([E.ComputeDistLine(x, n_samples=n) for x in l3]).reshape(-1),
                    g[f"out_dist_line_{n}"].reshape(-1))
    for n in (1000, 37):
        assert same(E.ComputeInlierRatios(lines, th, n_samples=n), g[f"out_ratios_{n}"].reshape(len(lines), th.size))
        for t_i in g["seg_th_idx"].tolist():
            for fn, key in ((E.ComputeInlierSegs, "insegs"), (E.ComputeOutlierSegs, "outsegs")):
                got = fn(l3, float(th[t_i]), n_samples=n)
                arr = np.array([np.concatenate([s.start, s.end]) for s in got]).reshape(-1, 6)
                assert same(arr, g[f"out_{key}_{t_i}_{n}"].reshape(-1, 6)), (key, t_i, n)
        R = ev.RefLineEvaluator(refl)
        assert same(R.ComputeRecallRefs(lines, th, num_samples=n), g[f"out_recall_ref_{n}"])
        assert same(R.ComputeRecallTesteds(lines, th, num_samples=n), g[f"out_recall_tested_{n}"])
    assert same(E.ComputeDistsforEachPoint(l3), g["out_dists_each"])
    if len(lines):
        k = min(3, len(lines) - 1)
        assert E.ComputeInlierRatio(l3[k], float(th[1])) == g["out_ratios_1000"][k, 1]
        assert ev.RefLineEvaluator(refl).ComputeRecallRef(l3, float(th[0])) == g["out_recall_ref_1000"][0]


def scene_clouds():
    rng = np.random.default_rng(11)
    out = {}
    out["random"] = rng.normal(size=(20000, 3))
    plane = rng.uniform(-1, 1, (8000, 3))
    plane[:, 2] = 0.25
    out["coplanar"] = plane
    t = rng.uniform(-2, 2, 5000)
    out["collinear"] = np.stack([t, 0.5 * t + 1.0, np.full_like(t, -3.0)], 1)
    a = rng.uniform(0, 1, (4000, 3))
    out["two_clusters"] = np.concatenate([a, a[:3000] + 1e4], 0)
    return out


@pytest.mark.parametrize("name", ["random", "coplanar", "collinear", "two_clusters"])
def test_device_equals_restatement_on_hard_clouds(ev, name):
    pts = scene_clouds()[name]
    rng = np.random.default_rng(5)
    lo, hi = pts.min(0), pts.max(0)
    ext = float(np.max(hi - lo))
    lines = np.concatenate([rand_lines(rng, 20, lo.min(), hi.max(), ext / 3),
                            rand_lines(rng, 4, hi.max() + 1e3 * ext, hi.max() + 1e3 * ext + 1, ext)], 0)  # far lines
    q = np.concatenate([rng.uniform(lo - 0.1, hi + 0.1, (2000, 3)), pts[:300],
                        rng.normal(size=(200, 3)) * 1e3 * ext], 0)  # 10^3 x the extent away
    E = ev.PointCloudEvaluator(pts)
    assert same(E.ComputeDistPoints(q), eo.nearest_dists(pts, q))
    th = np.array([1e-3, 1e-2, 0.1 * ext])
    assert same(E.ComputeInlierRatios(lines, th, n_samples=100), eo.inlier_ratios(pts, lines, th, 100))
    assert same(E.ComputeDistsforEachPoint(lines), eo.dists_for_each_point(pts, lines))
    R = ev.RefLineEvaluator(lines[:10])
    assert same(R.ComputeRecallTesteds(lines[10:], th, num_samples=50), eo.recall_length(lines[10:], lines[:10], th, 50))


def test_million_point_cloud_on_subsets(ev):
    rng = np.random.default_rng(3)
    n = 1_000_000
    pts = rng.uniform(0, 10, (n, 3))
    face = rng.integers(0, 6, n)
    pts[np.arange(n), face % 3] = np.where(face < 3, 0.0, 10.0)
    lines = rand_lines(rng, 500, 0, 10, 1.0)
    E = ev.PointCloudEvaluator(pts)
    # nearest distances of 2000 line samples against the brute-force minimum over all 10^6 points
    d = E._samples(lines, 0, 1000)[0].reshape(-1)
    pick = rng.choice(d.size, 2000, replace=False)
    assert same(d[pick], eo.nearest_dists(pts, eo.samples_center(lines, 1000).reshape(-1, 3)[pick], block=256))
    # inverse recall: 2000 cloud points against all lines
    de = E.ComputeDistsforEachPoint(lines)
    pp = rng.choice(n, 2000, replace=False)
    assert same(de[pp], eo.dists_for_each_point(pts[pp], lines))


@pytest.mark.parametrize("chunk", [64, 1000])
def test_chunk_edges(ev, chunk):
    rng = np.random.default_rng(chunk)
    for n_pts in (chunk - 1, chunk, chunk + 1):
        pts = rng.uniform(0, 1, (n_pts, 3))
        E = ev.PointCloudEvaluator(pts, chunk=chunk)
        for nq in (chunk - 1, chunk, chunk + 1):
            q = rng.uniform(-0.2, 1.2, (nq, 3))
            assert same(E.ComputeDistPoints(q), eo.nearest_dists(pts, q))
        lines = rand_lines(rng, 7, 0, 1, 0.5)
        assert same(E.ComputeDistsforEachPoint(lines), eo.dists_for_each_point(pts, lines))
        th = [0.01, 0.05]
        for n_s in (chunk // 4 - 1, chunk // 4, chunk // 4 + 1):  # 4 lines of samples per chunk, then across
            assert same(E.ComputeInlierRatios(lines, th, n_samples=n_s), eo.inlier_ratios(pts, lines, th, n_s))
        R = ev.RefLineEvaluator(lines[:3], chunk=chunk)
        assert same(R.ComputeRecallRefs(lines[3:], th, num_samples=chunk // 3 + 1),
                    eo.recall_length(lines[:3], lines[3:], th, chunk // 3 + 1))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_torch_tensor_points(ev, dtype):
    import torch
    rng = np.random.default_rng(8)
    pts = rng.uniform(0, 1, (5000, 3)).astype(dtype)
    lines = rand_lines(rng, 10, 0, 1, 0.5)
    Et = ev.PointCloudEvaluator(torch.from_numpy(pts).cuda())
    En = ev.PointCloudEvaluator(pts)
    ref = pts.astype(np.float64)  # float32 widens exactly
    th = [0.01, 0.02]
    want = eo.inlier_ratios(ref, lines, th, 200)
    assert same(Et.ComputeInlierRatios(lines, th, n_samples=200), want)
    assert same(En.ComputeInlierRatios(lines, th, n_samples=200), want)
    assert same(Et.ComputeDistsforEachPoint(lines), eo.dists_for_each_point(ref, lines))
    with pytest.raises(ValueError, match="non-finite"):
        ev.PointCloudEvaluator(torch.tensor([[0.0, 1.0, float("nan")]], device="cuda"))


def test_save_load_round_trip(ev, tmp_path):
    rng = np.random.default_rng(9)
    pts = rng.uniform(0, 1, (7000, 3))
    lines = rand_lines(rng, 12, 0, 1, 0.5)
    E = ev.PointCloudEvaluator(pts)
    E.Build()
    f = str(tmp_path / "index.bin")
    E.Save(f)
    E2 = ev.PointCloudEvaluator(pts)
    E2.Load(f)
    th = [0.005, 0.02]
    assert same(E2.ComputeInlierRatios(lines, th), E.ComputeInlierRatios(lines, th))
    assert same(E2.ComputeInlierRatios(lines, th), eo.inlier_ratios(pts, lines, th, 1000))
    other = pts.copy()
    other[0, 0] += 1e-9
    with pytest.raises(ValueError, match="other points"):
        ev.PointCloudEvaluator(other).Load(f)


def test_per_call_and_batched_forms_agree(ev):
    from limap_amd.base import Line3d
    rng = np.random.default_rng(10)
    pts = rng.uniform(0, 1, (3000, 3))
    lines = rand_lines(rng, 9, 0, 1, 0.6)
    l3 = [Line3d(r[:3], r[3:]) for r in lines]
    th = [0.002, 0.01, 0.03]
    E = ev.PointCloudEvaluator(pts)
    B = E.ComputeInlierRatios(l3, th)
    single = np.array([[E.ComputeInlierRatio(x, t) for t in th] for x in l3])
    assert same(B, single)
    q = rng.uniform(0, 1, (50, 3))
    assert same(E.ComputeDistPoints(q), [E.ComputeDistPoint(x) for x in q])
    R = ev.RefLineEvaluator(lines[:4])
    assert same(R.ComputeRecallRefs(l3[4:], th), [R.ComputeRecallRef(l3[4:], t) for t in th])
    assert same(R.ComputeRecallTesteds(l3[4:], th), [R.ComputeRecallTested(l3[4:], t) for t in th])


def test_end_to_end_scene(ev):
    """triangulated tracks of a synthetic scene against a GT cloud unprojected from its depth maps (eval_hypersim.py)"""
    from limap_amd import synthetic as syn, triangulation as tri
    sc = syn.make_scene(n_views=12, n_segs=80, n_neighbors=6, seed=3)
    T = tri.GlobalLineTriangulator(syn.default_triangulation_cfg())
    T.SetRanges(sc.ranges)
    T.InitArrays(sc.img_ids, sc.kvec, sc.qvec, sc.tvec, [sc.segs_of(i) for i in range(sc.n_images)])
    for i in sc.img_ids:
        T.TriangulateImage(int(i), sc.matches_of(int(i)))
    tracks = T.ComputeLineTracks()
    assert len(tracks) > 10
    h, w = 48, 64
    depths = syn.render_depths(sc, h=h, w=w, dtype=np.float64)
    small = syn.resize_scene(sc, h, w)
    xs, ys = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    cloud = []
    for n, img_id in enumerate(small.img_ids):
        fx, fy, cx, cy = small.kvec[n]
        R = syn.quat_to_rot(small.qvec[n])
        C = -R.T @ small.tvec[n]
        z = depths[int(img_id)]
        rc = np.stack([(xs - cx) / fx * z, (ys - cy) / fy * z, z], -1).reshape(-1, 3)
        ok = np.isfinite(rc).all(1)
        cloud.append(rc[ok] @ R + C)
    cloud = np.concatenate(cloud, 0)
    E = ev.PointCloudEvaluator(cloud)
    th = [0.01, 0.05, 0.1]
    rep = ev.report_error_to_GT(E, tracks, th, n_samples=200)
    lines = ev.lines_array(tracks)
    ratios = eo.inlier_ratios(cloud, lines, th, 200)
    lengths = eo.length(lines)
    assert same(rep["ratios"], ratios)
    assert same(rep["recall"], [(lengths * ratios[:, t]).sum() for t in range(3)])
    assert same(rep["precision"], [100 * (ratios[:, t] > 0).astype(int).sum() / len(lines) for t in range(3)])
    assert rep["precision"][-1] > 0.0
    pr = ev.report_pc_recall_for_GT(E, tracks, th)
    d = eo.dists_for_each_point(cloud, lines)
    assert same(pr["point_recall"], [100 * (d < t).sum() / len(d) for t in th])
    print("e2e: %d tracks, %d GT points; recall %s, precision %s, point recall %s" % (
        len(lines), len(cloud), np.round(rep["recall"], 3).tolist(), np.round(rep["precision"], 2).tolist(),
        np.round(pr["point_recall"], 2).tolist()))
