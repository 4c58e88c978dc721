"""limap_amd.structures without a GPU: the NumPy restatement (tests/bpt_oracle.py) against the goldens the reference's own
code wrote (tests/golden/bpt, make_bpt_golden.py), the sparse union-find replay against the full O(J^2) loop, and the
host side of the module (config parsing, containers, dict round trip, id assignment, error cases)."""
import glob
import os

import numpy as np
import pytest

import bpt_oracle as bo

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bpt")
NAMES = sorted(os.path.basename(p)[4:-4] for p in glob.glob(os.path.join(GOLD, "bpt_*.npz")))
EXPECTED = ["chain", "chain2", "clutter", "edges", "intersect", "no_keypoints", "no_lines", "one_line",
            "one_line_short", "thresholds"]


def load(name):
    z = np.load(os.path.join(GOLD, f"bpt_{name}.npz"))
    d = {k: z[k] for k in z.files}
    d["cfg"] = {k[4:]: float(d[k]) for k in z.files if k.startswith("cfg_")}
    return d


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def test_fixture_set():
    assert NAMES == EXPECTED


@pytest.mark.parametrize("name", EXPECTED)
def test_oracle_association_equals_reference(name):
    g = load(name)
    order = np.argsort(g["point_ids"], kind="stable")
    nb = bo.associate(g["lines"], g["points"], g["cfg"]["threshold_keypoints"])
    assert np.array_equal(g["out_assoc_point_ids"], g["point_ids"][order])
    off = g["out_assoc_off"]
    for n, k in enumerate(order.tolist()):
        assert np.array_equal(nb[k], g["out_assoc_line_ids"][off[n]:off[n + 1]]), (name, k)


@pytest.mark.parametrize("name", [n for n in EXPECTED if n != "no_lines"])
def test_oracle_junctions_equal_reference(name):
    g = load(name)
    o = bo.junctions(g["lines"], g["keypoints"], g["cfg"])
    assert np.array_equal(bits(o["xy"]), bits(g["out_junc_xy"]))  # bit for bit
    off = g["out_junc_off"]
    assert [list(map(int, g["out_junc_line_ids"][off[k]:off[k + 1]])) for k in range(len(off) - 1)] == o["line_ids"]
    assert np.array_equal(g["out_junc_point_ids"], np.arange(o["xy"].shape[0]))  # ids 0, 1, ... in that order


def test_exact_threshold_cases():
    g = load("edges")
    nb = bo.associate(g["lines"], g["points"], 2.0)
    assert nb[0].tolist() == [0] and nb[1].tolist() == [0]  # distance exactly 2.0 connects
    assert nb[2].size == 0 and nb[3].size == 0              # one ulp beyond does not
    assert nb[4].tolist() == [1] and nb[5].tolist() == [1]
    assert nb[8].tolist() == [0] and nb[9].size == 0        # clamped to the start
    assert nb[20].tolist() == [2] and nb[21].tolist() == [2] and nb[23].size == 0  # a zero-length line is its start
    o = bo.junctions(load("one_line")["lines"], load("one_line")["keypoints"], None)
    assert o["xy"].tolist() == [[0.0, 0.0]]  # exactly at the threshold: kept; 1.5 away: dropped


@pytest.mark.parametrize("name", [n for n in EXPECTED if n not in ("no_lines", "clutter")])
def test_sparse_replay_equals_full_loop_on_goldens(name):
    g = load(name)
    xy, _ = bo.candidates(g["lines"], g["cfg"]["threshold_intersection"])
    th = g["cfg"]["threshold_merge_junctions"]
    assert bo.roots(bo.merge_sparse(xy, th)) == bo.roots(bo.merge_full(xy, th))


def test_chain_fixture_reparents():
    """the fixture built for it: a candidate that joined an earlier cluster is re-parented to a later candidate"""
    g = load("chain2")
    xy, _ = bo.candidates(g["lines"], 2.0)
    parents = [-1] * xy.shape[0]
    moved = 0
    for i, j in bo.close_pairs(xy, 2.0).tolist():
        if bo.find_root(parents, i) != bo.find_root(parents, j):
            moved += parents[j] != -1
            parents[j] = i
    assert moved > 0


def test_sparse_replay_equals_full_loop_random():
    rng = np.random.default_rng(5)
    for t in range(300):
        n = int(rng.integers(2, 60))
        if t % 3 == 0:  # a chain in scrambled order
            xy = np.stack([1.5 * rng.permutation(n) + rng.normal(0, 0.2, n), rng.normal(0, 0.3, n)], 1)
        elif t % 3 == 1:
            xy = rng.uniform(0, 12, (n, 2))
        else:  # clumps
            xy = rng.integers(0, 4, (n, 2)) * 2.5 + rng.normal(0, 0.8, (n, 2))
        assert bo.roots(bo.merge_sparse(xy, 2.0)) == bo.roots(bo.merge_full(xy, 2.0)), t


def test_oracle_full_loop_junctions_small_scenes():
    rng = np.random.default_rng(6)
    for t in range(40):
        lines = rng.uniform(0, 40, (int(rng.integers(1, 9)), 4))
        kps = rng.uniform(0, 40, (int(rng.integers(0, 6)), 2))
        a, b = bo.junctions(lines, kps, None, full=False), bo.junctions(lines, kps, None, full=True)
        assert np.array_equal(bits(a["xy"]), bits(b["xy"])) and a["line_ids"] == b["line_ids"] and a["roots"] == b["roots"]


# ---- limap_amd.structures: host side ----------------------------------------------------------------------------------
def test_config_parsing():
    from limap_amd import structures as st
    c = st.PL_Bipartite2dConfig()
    assert (c.threshold_keypoints, c.threshold_intersection, c.threshold_merge_junctions) == (2.0, 2.0, 2.0)
    c = st.PL_Bipartite2dConfig({"threshold_intersection": 3, "no_such_key": 7})
    assert c.as_dict() == dict(threshold_keypoints=2.0, threshold_intersection=3.0, threshold_merge_junctions=2.0)
    assert st.PL_Bipartite2d({"threshold_keypoints": 0.5}).config_.threshold_keypoints == 0.5
    assert st.PL_Bipartite2d(c).config_.threshold_intersection == 3.0


def test_containers_ids_and_dict_round_trip():
    from limap_amd import structures as st
    from limap_amd.base import Line2d
    b = st.PL_Bipartite2d()
    b.init_lines(np.array([[0, 0, 1, 1, 0.9], [2, 2, 3, 3, 0.8]]), ids=[4, 9])  # a score column is ignored
    assert b.get_line_ids() == [4, 9] and b.count_lines() == 2
    assert b.add_line(Line2d(np.array([5.0, 5.0]), np.array([6.0, 6.0]))) == 10  # largest id + 1
    assert b.add_point(st.Point2d([1.0, 2.0], 77)) == 0
    assert b.add_point([3.0, 4.0], 5, neighbors=[4, 9]) == 5
    assert b.add_point([0.0, 0.0]) == 6
    b.add_edge(0, 9)
    assert b.count_points() == 3 and b.count_edges() == 3 and b.get_point_ids() == [0, 5, 6]
    assert b.neighbor_lines(5) == [4, 9] and b.neighbor_points(9) == [0, 5] and b.pdegree(6) == 0 and b.ldegree(9) == 2
    assert b.point(0).point3D_id == 77 and np.array_equal(b.line(9).start, [2.0, 2.0])
    j = b.junc(5)
    assert j.line_ids == [4, 9] and j.degree() == 2 and len(b.get_all_junctions()) == 3
    b.add_junction(st.Junction(st.Point2d([9.0, 9.0]), [10]))
    assert b.get_point_ids() == [0, 5, 6, 7] and b.neighbor_points(10) == [7]
    d = b.as_dict()
    assert sorted(d) == ["lines_", "nl2p_", "np2l_", "points_"]
    assert d["nl2p_"][9] == {0, 5} and d["points_"][0]["point3D_id"] == 77 and d["lines_"][4].shape == (2, 2)
    c = st.PL_Bipartite2d(d)
    d2 = c.as_dict()
    assert d2["np2l_"] == d["np2l_"] and d2["nl2p_"] == d["nl2p_"] and sorted(d2["points_"]) == sorted(d["points_"])
    assert all(np.array_equal(d2["lines_"][k], d["lines_"][k]) for k in d["lines_"])
    assert all(np.array_equal(d2["points_"][k]["p"], d["points_"][k]["p"]) for k in d["points_"])
    # the triangulator's reader (triangulation.py) takes the object as it is
    from limap_amd.triangulation import _bipartite_as_arrays
    a = _bipartite_as_arrays(c, 0)
    assert a["point_ids"].tolist() == [0, 5, 6, 7] and a["line_points"][9] == [0, 5] and a["point3D_ids"][0] == 77
    b.delete_edge(0, 9)
    b.delete_point(5)
    assert b.neighbor_points(9) == [] and not b.exist_point(5)
    b.delete_line(4)
    assert b.get_line_ids() == [9, 10]
    b.update_point(0, [8.0, 8.0])
    b.update_line(9, [0, 0, 9, 9])
    assert b.point(0).p.tolist() == [8.0, 8.0] and b.line(9).end.tolist() == [9.0, 9.0]
    b.clear_edges()
    assert b.count_edges() == 0
    b.clear_points()
    assert b.count_points() == 0 and b.count_lines() == 2
    b.reset()
    assert b.count_lines() == 0 and b.as_dict() == dict(points_={}, lines_={}, np2l_={}, nl2p_={})


def test_error_cases():
    from limap_amd import structures as st
    b = st.PL_Bipartite2d()
    b.init_lines(np.array([[0.0, 0, 1, 1]]))
    with pytest.raises(ValueError):
        b.add_line([0, 0, 1, 1], 0)  # the id exists
    with pytest.raises(ValueError):
        b.add_point([0, 0], neighbors=[3])  # no such line (the point itself is in by then, as in the reference)
    assert b.exist_point(0)
    with pytest.raises(ValueError):
        b.add_edge(5, 0)  # no such point
    with pytest.raises(ValueError):
        b.point(1)
    with pytest.raises(ValueError):
        b.init_lines(np.zeros((2, 4)), ids=[1])
    with pytest.raises(ValueError):
        st.lines2d_array(np.array([[0.0, 0, np.nan, 1]]))
    with pytest.raises(ValueError):
        st.lines2d_array(np.zeros((3, 3)))
    with pytest.raises(ValueError):
        b.add_keypoints_with_point3D_ids(np.zeros((2, 2)), [1])  # lengths differ: raised before any device work
    with pytest.raises(ValueError):
        b.add_keypoints_with_point3D_ids(np.array([[np.inf, 0.0]]), [1])
    with pytest.raises(RuntimeError):
        st.PL_Bipartite2d({"points_": {}})


# ---- the grid prefilter of k_bpt_close_pairs through its host twins (lt_bpt.h, compiled for the host) ------------------
import ctypes as C  # noqa: E402

import bpt_cases as bc  # noqa: E402

MASK = (1 << 20) - 1


def grid_keys(lib, lines, th, xy, img=0):
    """lt_fn_bpt_grid_keys: (lo x, lo y, cell), keys (n,) uint64"""
    lines = np.ascontiguousarray(lines, np.float64).reshape(-1, 4)
    xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
    grid, keys = np.zeros(3), np.zeros(max(xy.shape[0], 1), np.uint64)
    dp = C.POINTER(C.c_double)
    rc = lib.lt_fn_bpt_grid_keys(img, lines.shape[0], lines.ctypes.data_as(dp), float(th), xy.shape[0],
                                 xy.ctypes.data_as(dp), grid.ctypes.data_as(dp), keys.ctypes.data_as(C.POINTER(C.c_uint64)))
    assert rc == 0
    return grid, keys[:xy.shape[0]]


def host_pairs(lib, keys, xy, th):
    """lt_fn_bpt_close_pairs_host: (P, 2) int64, lexicographic"""
    xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
    keys = np.ascontiguousarray(keys, np.uint64)
    n, u64p = C.c_int64(0), C.POINTER(C.c_uint64)
    out = np.zeros(1, np.uint64)
    for _ in range(2):  # the count, then the pairs
        rc = lib.lt_fn_bpt_close_pairs_host(xy.shape[0], keys.ctypes.data_as(u64p), xy.ctypes.data_as(C.POINTER(C.c_double)),
                                            float(th), out.shape[0], out.ctypes.data_as(u64p), C.byref(n))
        assert rc == 0
        if n.value <= out.shape[0]:
            break
        out = np.zeros(n.value, np.uint64)
    out = out[:n.value]
    return np.stack([out >> np.uint64(32), out & np.uint64(0xffffffff)], 1).astype(np.int64)


def check_prefilter(lib, lines, th, xy, pairs=None, img=0):
    """every close pair of the restatement lies in the same or adjacent cells, every key inside the image's bit
    field, and the scan over the 3 x 3 cells finds exactly the restatement's pairs.  Returns the cells."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    grid, keys = grid_keys(lib, lines, th, xy, img)
    assert grid[2] > 0.0 and np.isfinite(grid[:2]).all()
    assert (keys >> np.uint64(40) == np.uint64(img)).all()
    cx, cy = (keys & np.uint64(MASK)).astype(np.int64), ((keys >> np.uint64(20)) & np.uint64(MASK)).astype(np.int64)
    pairs = bo.close_pairs(xy, th) if pairs is None else pairs
    i, j = pairs[:, 0], pairs[:, 1]
    assert (np.abs(cx[i] - cx[j]) <= 1).all() and (np.abs(cy[i] - cy[j]) <= 1).all()
    assert np.array_equal(host_pairs(lib, keys, xy, th), pairs.reshape(-1, 2))
    return grid, cx, cy


@pytest.mark.parametrize("name", list(bc.FAMILIES))
def test_case_generators_hold_their_properties(name):
    cases = bc.family(name)  # the generators assert
    assert cases and all(bc.reference(c)["cand_xy"].shape[0] <= bc.MAX_CANDIDATES for c in cases)


def test_batch_generators():
    lines, kps = bc.many_images()
    assert len(lines) == len(kps) == 3000 and all(lines[m].size == kps[m].size == 0 for m in (0, 1, 2, -3, -2, -1))
    assert [c[1].shape[0] for c in bc.sandwich()] == [1, 769, 1, 40, 1]


@pytest.mark.parametrize("name", list(bc.FAMILIES))
def test_close_pairs_share_adjacent_cells_on_case_families(gpu_lib, name):
    for k, c in enumerate(bc.family(name)):
        o = bc.reference(c)
        th = bo.config(c[3])["threshold_merge_junctions"]
        grid, cx, cy = check_prefilter(gpu_lib, c[1], th, o["cand_xy"], o["pairs"], img=(1 << 23) - 1 - k)
        a = c[1].reshape(-1, 2)
        assert grid[:2].tolist() == a.min(0).tolist()
        assert cx.min() == 0 and cy.min() == 0  # the endpoints at lo
        if bc.extent_branch(c[1], th):          # the whole grid is in use
            assert max(cx.max(), cy.max()) >= (1 << 20) - 3


def _adversarial():
    """(tag, lines, th, points): pairs exactly th apart astride cell boundaries, points at and beyond the box, a huge
    lo, no extent at all, and the thresholds 0, negative, +inf, subnormal"""
    out = []
    frame = np.array([[0.0, 0.0, 640.0, 480.0]])
    for th in (2.0, 0.7, 1e-4, 500.0):
        grid = max(1.25 * th, 640.0 / ((1 << 20) - 2))
        k = np.arange(1, 40, dtype=np.float64)
        b = k * grid  # cell boundaries
        pts = [np.stack([b - th / 2, 7 + 0 * k], 1), np.stack([b + th / 2, 7 + 0 * k], 1),
               np.stack([9 + 0 * k, b - th / 2], 1), np.stack([9 + 0 * k, b + th / 2], 1),
               np.stack([b, b], 1), np.stack([b + th, b], 1), np.stack([b, b - th], 1),
               np.stack([np.nextafter(b, 0), b], 1), np.stack([np.nextafter(b, 0) + th, b], 1)]
        out.append((f"boundary_th{th}", frame, th, np.concatenate(pts, 0)))
    for th, thi in ((2.0, 40.0), (0.5, 40.0), (1e-4, 2.0)):
        xs = [0.0, -th, th, -thi, -thi + th, -thi - th, 640.0, 640.0 + th, 640.0 - th, 640.0 + thi, 640.0 + thi - th,
              640.0 + thi + th, 1e7, 1e7 + th, -1e7, -1e7 - th, 1e150, -1e150]
        ys = [0.0, -th, 480.0, 480.0 + th, 480.0 + thi, -thi]
        pts = np.array([[x, y] for x in xs for y in ys])
        out.append((f"box_th{th}", frame, th, np.concatenate([pts, pts[:, ::-1]], 0)))
    for lo in (1e15, -1e15):
        k = np.arange(0, 60, dtype=np.float64)
        x = lo + 0.5 * k
        pts = np.concatenate([np.stack([x, -lo + 0 * k], 1), np.stack([x + 2.0, -lo + 0 * k], 1),
                              np.stack([lo + 0 * k, -lo + 0.5 * k + 2.0], 1)], 0)
        out.append((f"lo_{lo}", frame + np.array([lo, -lo, lo, -lo]), 2.0, pts))
    dot = np.array([[5.0, 5.0, 5.0, 5.0]] * 3)
    k = np.arange(-20, 21, dtype=np.float64)
    ring = np.concatenate([np.stack([5 + 2.0 * k, 5 + 0 * k], 1), np.stack([5 + 0 * k, 5 + 2.0 * k], 1),
                           np.stack([5 + 2.0 * k, 5 + 2.0 * k], 1)], 0)
    out.append(("extent0", dot, 2.0, ring))
    rng = np.random.default_rng(8)
    cloud = rng.uniform(0, 30, (150, 2))
    cloud[100:] = cloud[:50]  # coincident points, for the threshold 0
    tiny = 5e-324
    for th in (0.0, -1.0, float("inf"), tiny, 1e-310, 1e-160):
        out.append((f"frame_th{th}", frame, th, cloud))
        out.append((f"extent0_th{th}", dot, th, np.concatenate([ring, ring[:9]], 0)))
        # everything within a few thousand thresholds of the origin: the squares of the differences underflow, and the
        # reference's norm is 0 for all of them
        step = th if 0 < th < 1 else tiny
        m = np.arange(0, 3000, 7, dtype=np.float64)[:, None] * step
        out.append((f"origin_th{th}", np.zeros((2, 4)), th, np.concatenate([m * [1, 0], m * [0, 1], m * [1, 1]], 0)))
        out.append((f"small_extent_th{th}", np.array([[0.0, 0.0, 3000 * step, 0.0]]), th,
                    np.concatenate([m * [1, 0], m * [1, 0] + [0, step]], 0)))
    return out


@pytest.mark.parametrize("case", _adversarial(), ids=lambda c: c[0])
def test_close_pairs_share_adjacent_cells_on_adversarial_points(gpu_lib, case):
    _, lines, th, pts = case
    check_prefilter(gpu_lib, lines, th, pts, img=5)


def test_grid_keys_reject_what_the_device_call_rejects(gpu_lib):
    dp, u64p = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    lines, xy, keys = np.zeros((1, 4)), np.zeros((1, 2)), np.zeros(1, np.uint64)

    def call(lines=lines, xy=xy, th=2.0, img=0):
        return gpu_lib.lt_fn_bpt_grid_keys(img, 1, lines.ctypes.data_as(dp), th, 1, xy.ctypes.data_as(dp), None,
                                           keys.ctypes.data_as(u64p))
    assert call() == 0
    assert call(th=float("nan")) == -2 and call(img=1 << 23) == -2 and call(img=-1) == -2
    assert call(lines=np.array([[0.0, np.inf, 0.0, 0.0]])) == -2 and call(xy=np.array([[np.nan, 0.0]])) == -2


def test_sparse_replay_equals_full_loop_on_case_families():
    """DESIGN section 16's claim on structured clusters: stars, chains, polygons with shared vertices"""
    moved = 0
    for c in bc.reduced_cases():
        o = bc.reference(c)
        th = bo.config(c[3])["threshold_merge_junctions"]
        assert o["roots"] == bo.roots(bo.merge_full(o["cand_xy"], th)), c[0]
        moved += bc.count_reparents(o["cand_xy"], th, o["pairs"])
    assert moved >= 10
