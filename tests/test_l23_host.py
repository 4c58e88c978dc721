"""2D-3D line matching for localization (limap_amd.localization) on the host, without a GPU: the
host twin (lt_fn_l23_host) against the restatement of tests/l23_oracle.py on the edge scenes of tests/l23_scenes.py --
identical rows in identical order, winning losses bit for bit --, the upstream-named one-pair functions, the refusals
by their text, the runner on a planted scene, and the twin under AddressSanitizer."""
import numpy as np
import pytest

import est_oracle as eo
import est_scenes as es
import helpers
import l23_oracle as lo
import l23_scenes as S
from limap_amd import base
from limap_amd import estimators as est
from limap_amd import hybrid_localization as hl
from limap_amd import localization as loc

CASES = S.cases()


def rows_of(ref, q=0):
    return ref[1][ref[0][q]:ref[0][q + 1]].tolist()


# ---- 1. the twin equals the restatement ----
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_twin_equals_restatement(oracle, case):
    q_off, rows, loss = S.reference(oracle, case)
    res = S.product(loc, case, host=True)
    print(f"{case['name']}: {len(rows)} rows, per query {np.diff(q_off).tolist()}")
    assert np.array_equal(res["q_off"], q_off)
    assert np.array_equal(res["rows"], rows)
    assert np.array_equal(res["loss"].view(np.int64), loss.view(np.int64))


def test_thread_count_does_not_change_the_result():
    case = CASES[0]
    a, b = S.product(loc, case, host_threads=1), S.product(loc, case, host_threads=5)
    assert np.array_equal(a["rows"], b["rows"]) and np.array_equal(a["q_off"], b["q_off"])


def case_named(name):
    return next(c for c in CASES if c["name"] == name)


def test_the_cases_show_what_they_are_there_for(oracle):
    """on the restatement, so that no case passes vacuously"""
    # order: line 1's rows come before line 0's
    for name in ("order-all_pairs-None", "order-listed-None", "order-listed_filtered-None"):
        assert rows_of(S.reference(oracle, case_named(name))) == [[1, 1], [0, 0]], name
    # sizes: every query shape is there, a track reached through the image listed twice is kept twice, one row with a filter
    ref = S.reference(oracle, case_named("sizes-all_pairs-None"))
    n = np.diff(ref[0])
    assert n[0] > 0 and n[1] == 0 and n[3] == 0 and n[4] > 0
    r0 = rows_of(ref, 0)
    assert any(r0.count(r) >= 2 for r in r0)
    rf = rows_of(S.reference(oracle, case_named("sizes-all_pairs-Midpoint_Perpendicular")), 0)
    assert len(rf) == len({r[0] for r in rf}) and len(rf) > 0
    assert len(S.reference(oracle, case_named("all-fail-all_pairs-None-thr2.0"))[1]) == 0
    assert len(S.reference(oracle, case_named("degenerate-all_pairs-None"))[1]) > 0
    # filter: the twin tracks tie and the smaller id wins; the far line is dropped; the turned and the hidden track lose
    for name in ("Perpendicular", "Midpoint"):
        w = dict(rows_of(S.reference(oracle, case_named(f"filter-listed-{name}-dist_thres10.0"))))
        assert w[1] == S.T_TWIN_LO and 5 not in w and w[6] == 5 and 7 in w, (name, w)
        w2 = dict(rows_of(S.reference(oracle, case_named(f"filter-listed-{name}-dist_thres2.0"))))
        assert 7 not in w2 and w2[1] == S.T_TWIN_LO
    sc = S.filter_scene()
    ref6 = tuple(float(v) for v in sc["q_segs"][0][6])
    assert lo.candidate(oracle, "Midpoint", ref6, sc["q_cams"][0], sc["tracks6"][S.T_TURNED], 10.0, 0.4, 1.0)[1] is False
    assert lo.candidate(oracle, "Midpoint", ref6, sc["q_cams"][0], sc["tracks6"][S.T_TURNED], 10.0, 0.8, 1.0)[1] is True
    # no cheirality test: the track behind the camera is measured like any other
    assert np.isfinite(lo.candidate(oracle, "Perpendicular", ref6, sc["q_cams"][0], sc["tracks6"][S.T_BEHIND], 10.0, 0.4, 1.0)[0])
    a = lo.candidate(oracle, "Perpendicular", tuple(sc["q_segs"][0][1]), sc["q_cams"][0], sc["tracks6"][S.T_TWIN_LO], 10, 0.4, 1)
    b = lo.candidate(oracle, "Perpendicular", tuple(sc["q_segs"][0][1]), sc["q_cams"][0], sc["tracks6"][S.T_TWIN_HI], 10, 0.4, 1)
    assert a == b and a[1]
    counts = [sum(1 for i, _ in np.unique(sc["pairs"][0][0], axis=0) if i == k) for k in range(5)]
    assert tuple(counts) == S.FILTER_COUNTS


# ---- 2. upstream's functions ----
def _views(sc, q=0, d=0):
    qc, dc = sc["q_cams"][q], sc["db_cams"][d]
    return base.CameraView(qc[:4], qc[4:8], qc[8:]), base.CameraView(dc[:4], dc[4:8], dc[8:])


def test_one_pair_functions_equal_the_restatement(oracle):
    sc = S.sizes_scene()
    q, d = 4, 4
    qv, dv = _views(sc, q, d)
    q_lines = base.get_all_lines_2d({0: sc["q_segs"][q]})[0]
    d_lines = base.get_all_lines_2d({0: sc["db_segs"][d]})[0]
    want = lo.match_2to2(oracle, sc["q_segs"][q], sc["q_cams"][q], sc["db_segs"][d], sc["db_cams"][d], 0.2)
    got = loc.match_line_2to2_epipolarIoU(q_lines, d_lines, qv, None, dv, None, 0.2, host=True)
    assert got == want and len(want) > 0
    # (camera, pose) as upstream passes them
    got2 = loc.match_line_2to2_epipolarIoU(q_lines, d_lines, qv.kvec, (qv._qvec_given, qv.tvec), dv.K(), hl.CameraPose(dv.qvec, dv.tvec),
                                           0.2, host=True)
    assert got2 == want
    pairs = [(4, 3), (0, 1), (4, 3), (2, 9), (1, 64), (3, 0)]
    want_f = lo.filter_2to2(oracle, pairs, sc["q_segs"][q], sc["q_cams"][q], sc["db_segs"][d], sc["db_cams"][d], 0.2)
    assert loc.filter_line_2to2_epipolarIoU(pairs, q_lines, d_lines, qv, None, dv, None, 0.2, host=True) == want_f
    assert 0 < len(want_f) < len(pairs) or len(want_f) in (0, len(pairs))
    line2track = {7: list(sc["db_tracks"][d])}
    want3 = [(i, sc["db_tracks"][d][j]) for i, j in want if sc["db_tracks"][d][j] != -1]
    assert loc.match_line_2to3(want, line2track, 7) == want3 and 0 < len(want3) < len(want)
    assert hl.match_line_2to3 is loc.match_line_2to3 and hl.midpoint_dist is loc.midpoint_dist
    for n in hl._FUNCTIONS:
        assert n in hl.__all__ and callable(getattr(hl, n))


def test_distance_functions_and_the_filter_equal_the_restatement(oracle):
    sc = S.filter_scene()
    segs, cam, t6 = sc["q_segs"][0], sc["q_cams"][0], sc["tracks6"]
    lines = base.get_all_lines_2d({0: segs})[0]
    for name, fn in (("Perpendicular", loc.perpendicular_dist), ("Midpoint", loc.midpoint_dist),
                     ("Midpoint_Perpendicular", loc.midpoint_perpendicular_dist)):
        assert loc.get_reprojection_dist_func(name) is fn
        for a in range(3):
            for b in range(3):
                assert fn(lines[a], lines[b]) == lo.DIST[name](tuple(segs[a]), tuple(segs[b]))
    lists = {}
    for i, t in sc["pairs"][0][0]:
        lists.setdefault(int(i), []).append(int(t))
    view = base.CameraView(cam[:4], cam[4:8], cam[8:])
    tracks = [base.LineTrack(base.Line3d(l[:3], l[3:])) for l in t6]
    for name in ("Perpendicular", "Midpoint", "Midpoint_Perpendicular"):
        for kw in (dict(), dict(dist_thres=2)):
            want = [(i, t) for i, t, _ in lo.reprojection_filter(oracle, name, segs, cam, lists, t6, **{k: float(v) for k, v in kw.items()})]
            assert loc.reprojection_filter_matches_2to3(lines, view, lists, tracks, dist_func=loc.get_reprojection_dist_func(name),
                                                        host=True, **kw) == want
            assert loc.reprojection_filter_matches_2to3(lines, view, lists, tracks, dist_func=name, host=True, **kw) == want
    # the function's own default is the midpoint distance at dist_thres 10
    want = [(i, t) for i, t, _ in lo.reprojection_filter(oracle, "Midpoint", segs, cam, lists, t6)]
    assert loc.reprojection_filter_matches_2to3(lines, view, lists, tracks, host=True) == want


def test_invert_idmap_overwrites():
    tracks = [base.LineTrack(None, [3, 4], [0, 2]), base.LineTrack(None, [4, 3], [2, 1]), base.LineTrack(None, [], [])]
    got = base.get_invert_idmap_from_linetracks({3: [None] * 3, 4: [None] * 4, 9: []}, tracks)
    assert got == lo.get_invert_idmap({3: 3, 4: 4, 9: 0}, [([3, 4], [0, 2]), ([4, 3], [2, 1]), ([], [])])
    assert got == {3: [0, 1, -1], 4: [-1, -1, 1, -1], 9: []}


# ---- 3. refusals ----
def _refused(sc, match, mode="all_pairs", **kw):
    with pytest.raises(ValueError, match=match) as e:
        loc.match_lines_arrays(sc if "db_cam" in sc else loc.scene_arrays(*S.args(sc)), mode, host=True, **kw)
    assert str(e.value).startswith("limap_amd.localization: ") or str(e.value).startswith("[Error]")


def test_refusals():
    base_sc = S.with_pairs(S.sizes_scene())
    plain = {k: v for k, v in base_sc.items() if k != "pairs"}

    def edit(sc, fn):
        A = loc.scene_arrays(*S.args(sc))
        fn(A)
        return A

    _refused(edit(plain, lambda A: A["db_cam"].__setitem__((2, 5), np.nan)), "non-finite camera of database image 2")
    _refused(edit(plain, lambda A: A["q_cam"].__setitem__((3, 0), np.inf)), "non-finite camera of query 3")
    _refused(edit(plain, lambda A: A["db_seg"].__setitem__((70, 1), np.nan)), "non-finite database segment 70")
    _refused(edit(plain, lambda A: A["q_seg"].__setitem__((6, 3), -np.inf)), "non-finite query segment 6")
    _refused(edit(plain, lambda A: A["track6"].__setitem__((9, 0), np.nan)), "non-finite track 9", dist_func="Midpoint")
    _refused(edit(plain, lambda A: A["db_seg_off"].__setitem__(3, 0)), "database segment offsets decrease")
    _refused(edit(plain, lambda A: A["q_seg_off"].__setitem__(0, 1)), "query segment offsets must start at 0")
    _refused(edit(plain, lambda A: A["task_off"].__setitem__(1, 9)), "task offsets decrease")
    _refused(edit(base_sc, lambda A: A["pair_off"].__setitem__(3, 1)), "pair offsets decrease", mode="listed")
    _refused(edit(plain, lambda A: A["task_db"].__setitem__(4, 6)), "task 4 names database image row 6 of 6")
    _refused(edit(plain, lambda A: A["task_db"].__setitem__(0, -1)), "task 0 names database image row -1")
    _refused(edit(base_sc, lambda A: A["pairs"].__setitem__((5, 0), 5)), r"listed pair 5 \(5, \d+\) is outside the 5 x 130 lines of task 0",
             mode="listed")
    _refused(edit(base_sc, lambda A: A["pairs"].__setitem__((5, 1), 130)), "listed pair 5", mode="listed_filtered")
    _refused(edit(plain, lambda A: A["db_track"].__setitem__(10, 130)), r"database segment 10 has track id 130 \(tracks: 130\)")
    _refused(edit(plain, lambda A: A["db_track"].__setitem__(11, -2)), "database segment 11 has track id -2")
    with pytest.raises(ValueError, match=r"^\[Error\] Unknown dist function: Nearest$"):
        loc.match_lines_arrays(loc.scene_arrays(*S.args(plain)), dist_func="Nearest", host=True)
    with pytest.raises(ValueError, match=r"^\[Error\] Unknown dist function: None$"):
        loc.get_reprojection_dist_func(None)
    with pytest.raises(ValueError, match="dist_func must be perpendicular_dist, midpoint_dist or midpoint_perpendicular_dist"):
        loc.reprojection_filter_matches_2to3([], None, {0: [0]}, [], dist_func=lambda a, b: 0.0)
    with pytest.raises(ValueError, match="unknown mode"):
        loc.match_lines_arrays(loc.scene_arrays(*S.args(plain)), "some", host=True)
    with pytest.raises(ValueError, match="needs the listed pairs"):
        loc.match_lines_arrays(loc.scene_arrays(*S.args(plain)), "listed", host=True)
    with pytest.raises(ValueError, match="Unknown 2d line matcher: nearest"):
        loc.match_lines_2to3_scene({"2d_matcher": "nearest"}, None, None, {}, {}, [], {})
    _refused(plain, "non-finite threshold", IoU_threshold=float("nan"))


def test_the_unit_limit_is_refused_before_any_work():
    """all_pairs keeps one counter per (task, query line): above 2^31 - 1 of them the call is refused"""
    n_lines, n_tasks = 70000, 31000
    cam = S.cam11([1.0, 0, 0, 0], [0, 0, 0])
    sc = loc.scene_arrays([cam], [np.zeros((0, 4))], [[]], [cam], [np.zeros((n_lines, 4))], [[0] * n_tasks], None, np.zeros((0, 6)))
    with pytest.raises(ValueError, match=r"limap_amd.localization: more than 2\^31 - 1 \(task, query line\) units in one call \(2170000000\)"):
        loc.match_lines_arrays(sc, host=True)


# ---- 4. the runner ----
_RUN = {}


def runner_result(oracle, tmp_path_factory):
    if not _RUN:
        sc = S.loc_scene()
        db, qr, db_segs, q_segs, linemap, retrieval, corresp = S.collections(sc)
        out = tmp_path_factory.mktemp("l23") / "results.txt"
        poses = loc.hybrid_localization(S.cfg(skip=True), db, qr, corresp, linemap, retrieval, out, all_db_segs=db_segs,
                                        all_query_segs=q_segs, host=True, seed=3)
        _RUN.update(sc=sc, poses=poses, out=out, cols=(db, qr, db_segs, q_segs, linemap, retrieval, corresp),
                    ref=lo.match_scene(oracle, sc, "all_pairs", None))
    return _RUN


def test_runner_matches_and_poses(oracle, tmp_path_factory):
    run = runner_result(oracle, tmp_path_factory)
    sc, (db, qr, db_segs, q_segs, linemap, retrieval, corresp) = run["sc"], run["cols"]
    q_off, rows, _ = run["ref"]
    retrieved = {100 + q: [10 + d for d in sc["tasks"][q]] for q in range(len(sc["q_cams"]))}
    got = loc.match_lines_2to3_scene(S.cfg()["localization"], db, qr, db_segs, q_segs, linemap, retrieved, host=True)
    for q in range(len(sc["q_cams"])):
        assert np.array_equal(got[100 + q], rows[q_off[q]:q_off[q + 1]]) and len(got[100 + q]) > 0
    # the poses are the batch estimator's on the restatement's correspondences, bit for bit
    matches = {100 + q: rows[q_off[q]:q_off[q + 1]] for q in range(len(sc["q_cams"]))}
    t6 = np.asarray(sc["tracks6"], float)
    full = loc.estimator_queries(qr, q_segs, t6, matches, corresp, [100, 101], compact=False)
    want = est.pl_estimate_absolute_pose_batch(S.cfg()["localization"], full, host=True, seed=3)
    for n, qid in enumerate((100, 101)):
        pose = run["poses"][qid]
        assert np.array_equal(pose.qvec, want[n][0].qvec) and np.array_equal(pose.tvec, want[n][0].tvec)
        true = sc["truth"][n]
        err = eo.pose_error(pose.qvec, pose.tvec, eo.rotation(true[4:8]), true[8:11])
        print(f"query {qid}: {len(matches[qid])} line matches, pose error {err:.4f}")
        assert err < 0.05
    # handing over only the tracks a query's matches name changes neither poses nor statistics
    small = loc.estimator_queries(qr, q_segs, t6, matches, corresp, [100, 101], compact=True)
    assert all(len(a["l3ds"]) <= len(b["l3ds"]) for a, b in zip(small, full))
    got_small = est.pl_estimate_absolute_pose_batch(S.cfg()["localization"], small, host=True, seed=3)
    for (pa, sa), (pb, sb) in zip(got_small, want):
        assert np.array_equal(pa.qvec, pb.qvec) and np.array_equal(pa.tvec, pb.tvec)
        assert sa.best_model_score == sb.best_model_score and sa.inlier_ratios == sb.inlier_ratios
        assert sa.num_iterations_total == sb.num_iterations_total and sa.inlier_indices == sb.inlier_indices
        assert sa.num_iterations_per_solver == sb.num_iterations_per_solver and sa.best_num_inliers == sb.best_num_inliers


def test_runner_files(oracle, tmp_path_factory):
    run = runner_result(oracle, tmp_path_factory)
    db, qr, db_segs, q_segs, linemap, retrieval, corresp = run["cols"]
    lines = run["out"].read_text().splitlines()
    assert [l.split()[0] for l in lines] == ["query/0.png", "query/1.png"]
    for l, qid in zip(lines, (100, 101)):
        v = np.array(l.split()[1:], float)
        assert np.array_equal(v[:4], run["poses"][qid].qvec) and np.array_equal(v[4:], run["poses"][qid].tvec)
    pose_dir = run["out"].parent / "poses_epipolar"
    assert sorted(p.name for p in pose_dir.iterdir()) == ["100.txt", "101.txt"]
    # a second run takes the poses from the files: it needs neither segments nor correspondences
    (pose_dir / "100.txt").write_text("query/0.png 1.0 0.0 0.0 0.0 0.5 0.25 0.125\n")
    again = loc.hybrid_localization(S.cfg(skip=True), db, qr, {}, linemap, {}, run["out"], all_db_segs=db_segs, all_query_segs={},
                                    host=True, seed=3)
    assert np.array_equal(again[100].qvec, [1, 0, 0, 0]) and np.array_equal(again[100].tvec, [0.5, 0.25, 0.125])
    assert np.array_equal(again[101].qvec, run["poses"][101].qvec) and np.array_equal(again[101].tvec, run["poses"][101].tvec)
    assert run["out"].read_text().splitlines()[0].split()[1:] == ["1.0", "0.0", "0.0", "0.0", "0.5", "0.25", "0.125"]


def test_runner_listed_matcher_and_refinement_only(oracle, tmp_path_factory):
    """any matcher but "epipolar" reads its pairs (a dict or a directory of matches_{qid}.npy); ransac.method None refines the coarse pose"""
    run = runner_result(oracle, tmp_path_factory)
    sc, (db, qr, db_segs, q_segs, linemap, retrieval, corresp) = run["sc"], run["cols"]
    listed = S.with_pairs(sc, per_task=30)
    folder = tmp_path_factory.mktemp("l23m")
    as_dict = {}
    for q in range(len(sc["q_cams"])):
        as_dict[100 + q] = {10 + d: listed["pairs"][q][k] for k, d in enumerate(sc["tasks"][q])}
        np.save(folder / f"matches_{100 + q}.npy", as_dict[100 + q], allow_pickle=True)
    retrieved = {100 + q: [10 + d for d in sc["tasks"][q]] for q in range(len(sc["q_cams"]))}
    block = dict(S.cfg("gluestick")["localization"], epipolar_filter=True, reprojection_filter="Midpoint_Perpendicular")
    q_off, rows, _ = lo.match_scene(oracle, listed, "listed_filtered", "Midpoint_Perpendicular", dist_thres=2.0)
    for source in (as_dict, str(folder)):
        got = loc.match_lines_2to3_scene(block, db, qr, db_segs, q_segs, linemap, retrieved, line_matches_2to2=source, host=True)
        for q in range(len(sc["q_cams"])):
            assert np.array_equal(got[100 + q], rows[q_off[q]:q_off[q + 1]])
    out = folder / "refined.txt"
    poses = loc.hybrid_localization(S.cfg(method=None), db, qr, corresp, linemap, retrieval, out, all_db_segs=db_segs,
                                    all_query_segs=q_segs, host=True)
    assert sorted(poses) == [100, 101] and all(np.isfinite(p.qvec).all() and np.isfinite(p.tvec).all() for p in poses.values())
    assert len(out.read_text().splitlines()) == 2


def test_hloc_keypoints_from_log():
    class P:
        def __init__(self, xyz):
            self.xyz = np.array(xyz, float)

    class Sfm:
        points3D = {4: P([1, 2, 3]), 9: P([4, 5, 6])}

    logs = {"loc": {"a.png": {"keypoints_query": [[1.0, 2.0], [3.0, 4.0]], "3d_points": [[0, 0, 1], [0, 1, 0]], "points3D_ids": [9, 4],
                              "PnP_ret": {"inlier_mask": [True, False]}}}}
    p2, p3, inl = loc.get_hloc_keypoints_from_log(logs, "a.png")
    assert p2.tolist() == [[1, 2], [3, 4]] and p3.tolist() == [[0, 0, 1], [0, 1, 0]] and inl == [True, False]
    p2, p3, _ = loc.get_hloc_keypoints_from_log(logs, "a.png", Sfm(), {"a.png": 2.0})
    assert p2.tolist() == [[2.5, 4.5], [6.5, 8.5]] and p3.tolist() == [[4, 5, 6], [1, 2, 3]]


# ---- 5. the twin under the sanitizers ----
def test_twin_under_asan():
    helpers.run_host_asan("l23_asan", "l23_host_asan")
