"""limap_amd.structures on the device, zero tolerance throughout: against the goldens the reference's own code wrote
(tests/golden/bpt), against the NumPy restatement (tests/bpt_oracle.py) on larger random scenes, batched against
per-image against class methods, and end to end into GlobalLineTriangulator.SetBipartites2d."""
import numpy as np
import pytest

import bpt_oracle as bo
from test_bpt_host import EXPECTED, bits, load

pytestmark = pytest.mark.gpu

W, H = 640.0, 480.0


def rand_lines(rng, n, lo=15.0, hi=160.0):
    c = rng.uniform([0, 0], [W, H], (n, 2))
    ang = rng.uniform(0, np.pi, n)
    h = 0.5 * rng.uniform(lo, hi, n)[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
    return np.concatenate([c - h, c + h], 1)


def rand_points(rng, n, lines=None):
    """uniform points, a third of them moved next to a line when there are lines"""
    p = rng.uniform([0, 0], [W, H], (n, 2))
    if lines is not None and lines.shape[0] and n:
        k = n // 3
        ln = lines[rng.integers(0, lines.shape[0], k)]
        t = rng.uniform(-0.05, 1.05, (k, 1))
        p[:k] = ln[:, :2] + t * (ln[:, 2:] - ln[:, :2]) + rng.normal(0, 1.4, (k, 2))
    return p


def csr_lists(off, flat):
    return [flat[off[k]:off[k + 1]].tolist() for k in range(len(off) - 1)]


def golden_bipartite(st, g):
    b = st.PL_Bipartite2d(g["cfg"])
    b.init_lines(g["lines"])
    return b


@pytest.mark.parametrize("name", EXPECTED)
def test_association_equals_reference(gpu_lib, name):
    from limap_amd import structures as st
    g = load(name)
    b = golden_bipartite(st, g)
    b.add_keypoints_with_point3D_ids(g["points"], g["point3D_ids"], g["point_ids"])
    assert b.get_point_ids() == g["out_assoc_point_ids"].tolist()
    want = csr_lists(g["out_assoc_off"], g["out_assoc_line_ids"])
    assert [b.neighbor_lines(p) for p in b.get_point_ids()] == want
    d = b.as_dict()
    nl2p = {l: set() for l in range(g["lines"].shape[0])}
    for p, ls in zip(b.get_point_ids(), want):
        for l in ls:
            nl2p[l].add(p)
    assert d["nl2p_"] == nl2p and d["np2l_"] == {p: set(ls) for p, ls in zip(b.get_point_ids(), want)}
    order = np.argsort(g["point_ids"], kind="stable")
    assert [b.point(p).point3D_id for p in b.get_point_ids()] == g["point3D_ids"][order].tolist()
    assert np.array_equal(bits(np.array([b.point(p).p for p in b.get_point_ids()]).reshape(-1, 2)),
                          bits(g["points"][order]))


@pytest.mark.parametrize("name", [n for n in EXPECTED if n != "no_lines"])
def test_junctions_equal_reference(gpu_lib, name):
    from limap_amd import structures as st
    g = load(name)
    b = golden_bipartite(st, g)
    b.compute_intersection_with_points(g["keypoints"])
    assert b.get_point_ids() == g["out_junc_point_ids"].tolist()
    xy = np.array([p.p for p in b.get_all_points()]).reshape(-1, 2)
    assert np.array_equal(bits(xy), bits(g["out_junc_xy"]))  # bit for bit
    assert [j.line_ids for j in b.get_all_junctions()] == csr_lists(g["out_junc_off"], g["out_junc_line_ids"])
    # the batched entry point, and the intermediate lists against the restatement
    res = st.compute_junctions({3: g["lines"]}, {3: g["keypoints"]}, g["cfg"])
    assert np.array_equal(bits(res[3]), bits(g["out_junc_xy"]))
    _, cands = st._junctions([g["lines"]], [g["keypoints"]], st.PL_Bipartite2dConfig(g["cfg"]), candidates=True)
    o = bo.junctions(g["lines"], g["keypoints"], g["cfg"])
    assert np.array_equal(bits(cands[0]["xy"]), bits(o["cand_xy"]))
    assert np.array_equal(cands[0]["lines"], o["cand_lines"])
    want_parents = [-1 if r == k else r for k, r in enumerate(o["roots"])]  # after the last root look-ups
    assert cands[0]["parents"].tolist() == want_parents


def test_no_lines_and_compute_intersection(gpu_lib):
    from limap_amd import structures as st
    b = st.PL_Bipartite2d()
    b.compute_intersection_with_points(np.array([[1.0, 1.0]]))  # defined here: no junction
    assert b.count_points() == 0
    b.add_keypoints_with_point3D_ids(np.array([[1.0, 1.0]]), [7])
    assert b.get_point_ids() == [0] and b.neighbor_lines(0) == []
    # compute_intersection(): the bipartite's own points are the keypoints
    g = load("one_line")
    b = golden_bipartite(st, g)
    b.add_keypoints_with_point3D_ids(g["keypoints"], [5, 6])
    b.compute_intersection()
    assert b.get_point_ids() == [0, 1, 2] and b.point(2).p.tolist() == [0.0, 0.0] and b.neighbor_lines(2) == [0]
    assert b.point(2).point3D_id == -1
    b.add_keypoint(st.Point2d([50.0, 2.0], 9))
    b.add_keypoint([50.0, 2.5], 40)
    assert b.neighbor_lines(3) == [0] and b.neighbor_lines(40) == [] and b.point(3).point3D_id == 9


def test_native_errors(gpu_lib):
    import ctypes as C
    from limap_amd import _capi, structures as st
    ctx = st._context(0)
    cfg = _capi.LtBptConfig(2.0, 2.0, 2.0)
    off = np.array([0, 1], np.int64)
    pt = np.zeros((1, 2))

    def call(fn, lines, cfg=cfg, loff=off):
        out = np.zeros(4, np.int64)
        return fn(ctx.h, 1, st._p(loff, C.c_int64), st._p(lines), st._p(off, C.c_int64), st._p(pt), C.byref(cfg),
                  st._p(out, C.c_int64))
    for fn in (ctx.L.lt_bpt_associate, ctx.L.lt_bpt_junctions):
        assert call(fn, np.array([[0.0, 0.0, np.nan, 1.0]])) == -2  # rejected before any launch
        assert b"non-finite" in ctx.L.lt_last_error(ctx.h)
        assert call(fn, np.zeros((1, 4)), cfg=_capi.LtBptConfig(2.0, float("nan"), 2.0)) == -2
        assert call(fn, np.zeros((1, 4)), loff=np.array([1, 1], np.int64)) == -2
        assert call(fn, np.array([[0.0, 0.0, 3.0, 4.0]])) == 0
    d = _capi.LtBptConfig()
    ctx.L.lt_bpt_config_default(C.byref(d))
    assert (d.threshold_keypoints, d.threshold_intersection, d.threshold_merge_junctions) == (2.0, 2.0, 2.0)


def _ragged_scene(seed, n_lines, n_pts):
    rng = np.random.default_rng(seed)
    lines = [rand_lines(rng, m) for m in n_lines]
    pts = [rand_points(rng, p, l) for p, l in zip(n_pts, lines)]
    return lines, pts


def test_association_large_batch_equals_oracle(gpu_lib):
    """50 images, ragged counts around 500 lines x 3000 keypoints, images without lines / without keypoints in the
    middle, one image beyond the LDS tile of lines (512)"""
    from limap_amd import structures as st
    rng = np.random.default_rng(77)
    n_lines = rng.integers(300, 512, 50).tolist()
    n_pts = rng.integers(2000, 3500, 50).tolist()
    n_lines[7], n_pts[8], n_lines[20], n_pts[20] = 0, 0, 0, 0
    n_lines[13], n_lines[14], n_pts[15] = 1300, 513, 257
    lines, pts = _ragged_scene(78, n_lines, n_pts)
    cfg = st.PL_Bipartite2dConfig()
    res = st._associate(lines, pts, cfg)
    n_edges = 0
    for m in range(50):
        want = bo.associate(lines[m], pts[m], 2.0)
        assert csr_lists(*res[m]) == [w.tolist() for w in want], m
        n_edges += sum(w.size for w in want)
    assert n_edges > 20000
    # batched == per image == class methods
    for m in (0, 7, 8, 13):
        (one,) = st._associate([lines[m]], [pts[m]], cfg)
        assert np.array_equal(one[0], res[m][0]) and np.array_equal(one[1], res[m][1])
    def p3d_of(n):  # every fifth keypoint observes no 3D point
        return np.arange(n) - (np.arange(n) % 5 == 0) * 10**6
    kp = {m: (pts[m], p3d_of(pts[m].shape[0]), None) for m in (3, 7, 8, 14)}
    bp = st.compute_2d_bipartites({m: lines[m] for m in kp}, kp, cfg)
    for m, b in bp.items():
        keep = np.flatnonzero(kp[m][1] >= 0)  # rows without a 3D point are dropped, ids are the row numbers
        assert b.get_point_ids() == keep.tolist()
        c = st.PL_Bipartite2d(cfg)
        c.init_lines(lines[m])
        c.add_keypoints_with_point3D_ids(pts[m][keep], kp[m][1][keep], keep)
        assert c.as_dict()["np2l_"] == b.as_dict()["np2l_"] and c.as_dict()["nl2p_"] == b.as_dict()["nl2p_"]
        batch = csr_lists(*res[m])
        assert [b.neighbor_lines(int(k)) for k in keep] == [batch[int(k)] for k in keep]


def test_junctions_batch_equals_oracle(gpu_lib):
    """ragged images, one without lines and one without keypoints in the middle, a single line, other thresholds"""
    from limap_amd import structures as st
    n_lines = [150, 0, 90, 1, 260, 2, 120]
    n_kps = [800, 50, 0, 3, 1500, 0, 400]
    lines, kps = _ragged_scene(91, n_lines, n_kps)
    for cfg in (None, dict(threshold_intersection=3.0, threshold_merge_junctions=1.25)):
        c = st.PL_Bipartite2dConfig(cfg)
        res, cands = st._junctions(lines, kps, c, candidates=True)
        total = 0
        for m in range(len(lines)):
            o = bo.junctions(lines[m], kps[m], cfg)
            assert np.array_equal(bits(cands[m]["xy"]), bits(o["cand_xy"])), m
            assert np.array_equal(cands[m]["lines"], o["cand_lines"].reshape(-1, 2)), m
            assert np.array_equal(bits(res[m][0]), bits(o["xy"])), m
            assert csr_lists(res[m][1], res[m][2]) == o["line_ids"], m
            total += o["xy"].shape[0]
            (one,) = st._junctions([lines[m]], [kps[m]], c)  # batched == per image
            assert np.array_equal(bits(one[0]), bits(res[m][0])) and np.array_equal(one[2], res[m][2])
        assert total > 500
        out = st.compute_junctions(dict(enumerate(lines)), dict(enumerate(kps)), cfg)
        assert all(np.array_equal(bits(out[m]), bits(res[m][0])) for m in range(len(lines)))
    # class methods, with sparse line ids
    b = st.PL_Bipartite2d()
    ids = np.arange(n_lines[2]) * 3 + 2
    b.init_lines(lines[2], ids)
    b.compute_intersection_with_points(kps[2])
    o = bo.junctions(lines[2], kps[2], None)
    assert [j.line_ids for j in b.get_all_junctions()] == [ids[l].tolist() for l in o["line_ids"]]
    assert np.array_equal(bits(np.array([p.p for p in b.get_all_points()])), bits(o["xy"]))


def test_bipartites_feed_the_triangulator(gpu_lib, oracle):
    """compute_2d_bipartites from keypoints (the synthetic associations' points plus off-line clutter) into
    GlobalLineTriangulator.SetBipartites2d, against the restatement's bipartites in the oracle triangulator"""
    from helpers import restated_one_point
    from limap_amd import structures as st, synthetic as syn
    from limap_amd.triangulation import _bipartite_as_arrays
    from test_gpu_points import _compare
    sc = syn.make_scene(n_views=10, n_segs=70, n_neighbors=4, seed=71)
    truth, sfm = syn.make_bipartites(sc, seed=2)
    rng = np.random.default_rng(3)
    lines2d, keypoints, want = {}, {}, {}
    n_edges = 0
    for n, i in enumerate(int(x) for x in sc.img_ids):
        segs = np.asarray(sc.segs_of(n), np.float64).reshape(-1, 4)
        xy = np.concatenate([truth[i]["xy"], rng.uniform([0, 0], [syn.W_IMG, syn.H_IMG], (150, 2))], 0)
        p3d = np.concatenate([truth[i]["point3D_ids"], np.full(150, -1)]).astype(np.int64)
        p3d[-150::3] = 10**6 + np.arange(50)  # clutter that claims a 3D point the SfM model does not hold stays in
        ids = np.arange(xy.shape[0])
        lines2d[i], keypoints[i] = segs, (xy, p3d, ids)
        keep = p3d >= 0
        d = bo.bipartite_dict(segs, xy[keep], p3d[keep], ids[keep])
        want[i] = _bipartite_as_arrays(d, segs.shape[0])
        n_edges += sum(len(v) for v in d["nl2p_"].values())
    assert n_edges > 300
    got = st.compute_2d_bipartites(lines2d, keypoints)
    for i in got:
        a = _bipartite_as_arrays(got[i], lines2d[i].shape[0])
        assert np.array_equal(a["point_ids"], want[i]["point_ids"]) and a["line_points"] == want[i]["line_points"]
        assert np.array_equal(bits(a["xy"]), bits(want[i]["xy"]))
    sfm = dict(sfm)
    for k in range(50):
        sfm[10**6 + k] = rng.uniform(-1, 1, 3)
    cfg = syn.default_triangulation_cfg(debug_mode=True)
    from limap_amd import triangulation as tri
    with restated_one_point(oracle):
        T = tri.GlobalLineTriangulator(cfg)
        O = oracle.OracleTriangulator(cfg, faithful=False)
        T.SetRanges(sc.ranges); O.SetRanges(sc.ranges)
        T.InitArrays(sc.img_ids, sc.kvec, sc.qvec, sc.tvec, [sc.segs_of(k) for k in range(sc.n_images)])
        O.Init(sc.img_ids, sc.kvec, sc.qvec, sc.tvec, sc.seg_off, sc.segs)
        T.SetBipartites2d(got); O.SetBipartites2d(want)  # the product gets the objects, the oracle the restatement
        T.SetSfMPoints(sfm); O.SetSfMPoints(sfm)
        for i in sc.img_ids:
            m = sc.matches_of(int(i))
            T.TriangulateImage(int(i), m)
            O.TriangulateImage(int(i), m)
        g = _compare(T, O)
    assert g["off"][-1] > 0
