"""Mirror of `limap.optimize.hybrid_localization.functions` and of `limap.runners.hybrid_localization`: the 2D-3D line
matching in front of the pose estimation, and the runner around both.

    matches = localization.match_lines_2to3_scene(cfg["localization"], imagecols_db, imagecols_query, all_db_segs,
                                                  all_query_segs, linemap_db, retrieved)        # qid -> (M, 2)
    poses = localization.hybrid_localization(cfg, imagecols_db, imagecols_query, point_corresp, linemap_db, retrieval,
                                             results_path, all_db_segs=all_db_segs, all_query_segs=all_query_segs)

A pair (query line i, database line j) of a task (query, retrieved database image) survives if
`compute_epipolar_IoU(l_i, view_q, l_j, view_d) > IoU_threshold` and the database line belongs to a track.  Upstream tests
every pair of every task in nested Python loops; here all queries go through one set of launches of lt_kernels_l23.hip,
and the rows come back in upstream's order (the estimator's sampler draws correspondences by index).  The reprojection
filter (`reprojection_filter_matches_2to3`) runs on the device too.

The upstream-named functions are one-task calls of the same native path.  `match_line_2to3` alone is a plain lookup in
Python: its result keeps the order of the pair list, which the grouped rows of the native call do not carry.

`host=True` (or `host_threads=N`) runs the documented host twin (lt_fn_l23_host) instead of the device; it is a request,
never a fallback.  Line detection, extractors, learned matchers and HLoc's readers are not part of this module.
"""
import ctypes as C
import math
import os
from pathlib import Path

import numpy as np

from . import _capi, _native, base
from . import hybrid_localization as _hl

__all__ = ["match_line_2to2_epipolarIoU", "filter_line_2to2_epipolarIoU", "match_line_2to3", "midpoint_dist",
           "midpoint_perpendicular_dist", "perpendicular_dist", "get_reprojection_dist_func",
           "reprojection_filter_matches_2to3", "match_lines_2to3_scene", "hybrid_localization", "get_hloc_keypoints_from_log",
           "scene_arrays", "match_lines_arrays", "estimator_queries", "MODES", "FILTERS", "MATCHERS"]

WHO = "limap_amd.localization"
MODES = {"all_pairs": 0, "listed": 1, "listed_filtered": 2}
FILTERS = {None: 0, "Perpendicular": 1, "Midpoint": 2, "Midpoint_Perpendicular": 3}
MATCHERS = ("epipolar", "sold2", "superglue_endpoints", "gluestick", "linetr", "lbd", "l2d2")  # runners/hybrid_localization.py:142-150

_context = _capi.per_device_contexts()


# ---- the three distances in plain Python (functions.py:66-83) with the definition's scalar arithmetic ----
def _ends(line):
    if hasattr(line, "start"):
        s, e = line.start, line.end
    else:
        a = np.asarray(line, float).reshape(4)
        s, e = a[:2], a[2:]
    return (float(s[0]), float(s[1])), (float(e[0]), float(e[1]))


def _direction(s, e):
    x, y = e[0] - s[0], e[1] - s[1]
    z = x * x + y * y
    if z > 0.0:
        n = math.sqrt(z)
        return x / n, y / n
    return x, y


def _length(s, e):
    x, y = s[0] - e[0], s[1] - e[1]
    return math.sqrt(x * x + y * y)


def _mid(s, e):
    return (s[0] + e[0]) * 0.5, (s[1] + e[1]) * 0.5


def _cross(a, b):
    return a[0] * b[1] - a[1] * b[0]


def _div(a, b):
    a, b = np.float64(a), np.float64(b)
    with np.errstate(all="ignore"):
        return float(a / b)


def midpoint_dist(ref_line, tgt_line):
    mr, mt = _mid(*_ends(ref_line)), _mid(*_ends(tgt_line))
    x, y = mr[0] - mt[0], mr[1] - mt[1]
    return math.sqrt(x * x + y * y)


def midpoint_perpendicular_dist(ref_line, tgt_line):
    rs, re = _ends(ref_line)
    ts, te = _ends(tgt_line)
    m, d = _mid(rs, re), _direction(ts, te)
    return _div(abs(_cross(d, (ts[0] - m[0], ts[1] - m[1]))), _length(rs, re))  # divided by the query line's length


def perpendicular_dist(ref_line, tgt_line):
    rs, re = _ends(ref_line)
    ts, te = _ends(tgt_line)
    d = _direction(ts, te)
    return 0.5 * (abs(_cross(d, (ts[0] - rs[0], ts[1] - rs[1]))) + abs(_cross(d, (ts[0] - re[0], ts[1] - re[1]))))


def get_reprojection_dist_func(func_name):
    if func_name == "Perpendicular":
        return perpendicular_dist
    if func_name == "Midpoint":
        return midpoint_dist
    if func_name == "Midpoint_Perpendicular":
        return midpoint_perpendicular_dist
    raise ValueError(f"[Error] Unknown dist function: {func_name}")


def _filter_kind(dist_func):
    """0 for None; a name or one of the three functions -> 1..3"""
    if dist_func is None:
        return 0
    if isinstance(dist_func, str):
        dist_func = get_reprojection_dist_func(dist_func)
    for name, fn in (("Perpendicular", perpendicular_dist), ("Midpoint", midpoint_dist),
                     ("Midpoint_Perpendicular", midpoint_perpendicular_dist)):
        if dist_func is fn:
            return FILTERS[name]
    raise ValueError(f"{WHO}: dist_func must be perpendicular_dist, midpoint_dist or midpoint_perpendicular_dist (or "
                     f"\"Perpendicular\", \"Midpoint\", \"Midpoint_Perpendicular\"), not {dist_func!r}")


# ---- arrays ----
def _f64(x, width, what):
    """(n, width) float64, contiguous, on the host (arrays and tensors enter through _native.operand)"""
    op = _native.operand(x, host=True, device=None, who=WHO, what=what)
    a = np.asarray(op.astype("float64").contiguous().keep)
    if a.size == 0:
        return np.zeros((0, width))
    if a.ndim == 3 and a.shape[1:] == (2, width // 2):
        a = a.reshape(-1, width)
    if a.ndim != 2 or a.shape[1] < width:
        raise ValueError(f"{WHO}: {what} must have shape (n, {width}), not {a.shape}")
    return np.ascontiguousarray(a[:, :width])


def _lines4(lines, what="segments"):
    """a list of Line2d or an (n, 4+) array -> (n, 4)"""
    if isinstance(lines, (list, tuple)) and len(lines) and hasattr(lines[0], "start"):
        return np.array([[l.start[0], l.start[1], l.end[0], l.end[1]] for l in lines], float).reshape(-1, 4)
    if isinstance(lines, (list, tuple)) and not len(lines):
        return np.zeros((0, 4))
    return _f64(lines, 4, what)


def _cam11(cam, pose=None):
    """a CameraView (kvec, qvec, tvec), or upstream's (camera, pose) with pose a CameraPose or (qvec | R, tvec)"""
    if pose is None:
        if isinstance(cam, (tuple, list)) and len(cam) == 2:
            cam, pose = cam
        elif hasattr(cam, "tvec"):
            pose = cam
            cam = cam.kvec
        else:
            a = np.asarray(cam, float).reshape(-1)
            if a.size != 11:
                raise ValueError(f"{WHO}: a camera is a CameraView, (camera, pose) or 11 numbers (kvec, qvec, tvec)")
            return a
    kvec = _hl._kvec(cam)
    if hasattr(pose, "tvec"):
        q, t = getattr(pose, "_qvec_given", pose.qvec), pose.tvec
    else:
        q, t = np.asarray(pose[0], float).reshape(-1), pose[1]
        if q.size == 9:
            q = _hl._qvec_from_R(q)
    return np.concatenate([kvec, np.asarray(q, float).reshape(4), np.asarray(t, float).reshape(3)])


def scene_arrays(db_cams, db_segs, db_tracks, q_cams, q_segs, tasks, pairs=None, tracks6=None):
    """The flat arrays of lt_l23_match.  db_cams / q_cams: (n, 11) rows or sequences `_cam11` reads; db_segs / q_segs: per
    image its (n, 4) segments; db_tracks: per database image the track id of each segment (-1: none); tasks: per query
    the database image rows in retrieval order; pairs (listed modes): per query, per task its (m, 2+) pairs; tracks6:
    (T, 6) or (T, 2, 3)."""
    cams = lambda v: (np.ascontiguousarray(np.array([_cam11(c) for c in v], float).reshape(-1, 11)) if len(v)  # noqa: E731
                      else np.zeros((0, 11)))
    sc = dict(db_cam=cams(db_cams), q_cam=cams(q_cams))
    if len(db_segs) != len(sc["db_cam"]) or len(db_tracks) != len(db_segs) or len(q_segs) != len(sc["q_cam"]) or len(tasks) != len(q_segs):
        raise ValueError(f"{WHO}: cameras, segments, track ids or tasks differ in length")
    dsegs = [_lines4(s, "database segments") for s in db_segs]
    qsegs = [_lines4(s, "query segments") for s in q_segs]
    sc["db_seg_off"], sc["db_seg"] = _native.csr(dsegs, 4) if dsegs else (np.zeros(1, np.int64), np.zeros((1, 4)))
    sc["q_seg_off"], sc["q_seg"] = _native.csr(qsegs, 4) if qsegs else (np.zeros(1, np.int64), np.zeros((1, 4)))
    trk = [np.asarray(t, np.int64).reshape(-1) for t in db_tracks]
    for k, (t, s) in enumerate(zip(trk, dsegs)):
        if len(t) != len(s):
            raise ValueError(f"{WHO}: database image {k} has {len(s)} segments and {len(t)} track ids")
    flat = np.concatenate(trk) if trk else np.zeros(0, np.int64)
    if len(flat) and (flat.min() < -(1 << 31) or flat.max() >= (1 << 31)):
        raise ValueError(f"{WHO}: a track id does not fit 32 bits")
    sc["db_track"] = np.ascontiguousarray(flat.astype(np.int32)) if len(flat) else np.zeros(1, np.int32)
    sc["task_off"] = np.zeros(len(tasks) + 1, np.int64)
    for q, t in enumerate(tasks):
        sc["task_off"][q + 1] = sc["task_off"][q] + len(t)
    rows = [int(r) for t in tasks for r in t]
    sc["task_db"] = np.ascontiguousarray(np.array(rows if rows else [0], np.int32))
    sc["pair_off"] = sc["pairs"] = None
    if pairs is not None:
        if len(pairs) != len(tasks) or any(len(p) != len(t) for p, t in zip(pairs, tasks)):
            raise ValueError(f"{WHO}: the listed pairs do not follow the tasks")
        per_task = [np.asarray(m).reshape(-1, np.asarray(m).shape[-1] if np.asarray(m).ndim == 2 else 2)[:, :2] if np.asarray(m).size
                    else np.zeros((0, 2)) for p in pairs for m in p]
        sc["pair_off"] = np.zeros(len(per_task) + 1, np.int64)
        for k, m in enumerate(per_task):
            sc["pair_off"][k + 1] = sc["pair_off"][k] + len(m)
        allp = np.concatenate(per_task) if per_task and sc["pair_off"][-1] else np.zeros((0, 2))
        if len(allp) and (np.abs(allp) >= (1 << 31)).any():
            raise ValueError(f"{WHO}: a listed line index does not fit 32 bits")
        sc["pairs"] = np.ascontiguousarray(allp.astype(np.int32)) if len(allp) else np.zeros((1, 2), np.int32)
    t6 = np.zeros((0, 6)) if tracks6 is None else _f64(tracks6, 6, "tracks")
    sc["n_tracks"] = len(t6)
    sc["track6"] = t6 if len(t6) else np.zeros((1, 6))
    return sc


def _config(mode, dist_func, IoU_threshold, dist_thres, sine_thres, angle_scale):
    c = _capi.LtL23Config()
    _capi.load_library().lt_l23_config_default(C.byref(c))
    if mode not in MODES:
        raise ValueError(f"{WHO}: unknown mode {mode!r} (one of {', '.join(MODES)})")
    c.mode, c.filter = MODES[mode], _filter_kind(dist_func)
    c.IoU_threshold, c.dist_thres = float(IoU_threshold), float(dist_thres)
    c.sine_thres, c.angle_scale = float(sine_thres), float(angle_scale)
    return c


def match_lines_arrays(sc, mode="all_pairs", dist_func=None, IoU_threshold=0.2, dist_thres=10.0, sine_thres=0.4,
                       angle_scale=1.0, host=False, host_threads=None, ctx=None):
    """One call of lt_l23_match (device) or lt_fn_l23_host on the arrays of `scene_arrays` -> dict with q_off (Q + 1),
    rows (M, 2) = (query line, track id) in upstream's order, loss (M,) (the winning loss with a filter) and timers"""
    cfg = _config(mode, dist_func, IoU_threshold, dist_thres, sine_thres, angle_scale)
    if (cfg.mode != 0) != (sc["pairs"] is not None):
        raise ValueError(f"{WHO}: mode {mode!r} " + ("needs the listed pairs" if cfg.mode else "takes no listed pairs"))
    L = _capi.load_library()
    p = _capi.ptr
    inp = _capi.LtL23Input()
    inp.n_db, inp.n_query, inp.n_tracks = len(sc["db_cam"]), len(sc["q_cam"]), int(sc["n_tracks"])
    pad = lambda a, w: a if len(a) else np.zeros((1, w))  # noqa: E731
    keep = [pad(sc["db_cam"], 11), pad(sc["q_cam"], 11)]
    inp.db_cam11, inp.q_cam11 = p(keep[0]), p(keep[1])
    inp.db_seg_off, inp.db_seg4, inp.db_track = p(sc["db_seg_off"], C.c_int64), p(sc["db_seg"]), p(sc["db_track"], C.c_int32)
    inp.q_seg_off, inp.q_seg4 = p(sc["q_seg_off"], C.c_int64), p(sc["q_seg"])
    inp.task_off, inp.task_db = p(sc["task_off"], C.c_int64), p(sc["task_db"], C.c_int32)
    if sc["pairs"] is not None:
        inp.pair_off, inp.pairs2 = p(sc["pair_off"], C.c_int64), p(sc["pairs"], C.c_int32)
    inp.track6 = p(sc["track6"])
    Q = inp.n_query
    ht = _native.host_threads(host, host_threads)
    q_off = np.zeros(Q + 1, np.int64)
    timers = None
    if ht is not None:
        n = C.c_int64(0)
        if L.lt_fn_l23_host(C.byref(inp), C.byref(cfg), int(ht), C.byref(n)) != 0:
            _native.raise_host_error(L, "lt_fn_l23_host_error")
        M = int(n.value)
        rows, loss = np.zeros((max(M, 1), 2), np.int32), np.zeros(max(M, 1))
        L.lt_fn_l23_host_get(p(q_off, C.c_int64), p(rows, C.c_int32), p(loss))
    else:
        ctx = ctx if ctx is not None else _context()
        ctx.chk(L.lt_l23_match(ctx.h, C.byref(inp), C.byref(cfg)))
        M = int(L.lt_l23_num(ctx.h))
        rows, loss = np.zeros((max(M, 1), 2), np.int32), np.zeros(max(M, 1))
        ctx.chk(L.lt_l23_get(ctx.h, p(q_off, C.c_int64), p(rows, C.c_int32), p(loss)))
        tm = ctx.module_timers("lt_l23_get_timers", 8)
        timers = dict(prepare_ms=float(tm[0]), launches_ms=float(tm[1]), download_ms=float(tm[2]), build_device_ms=float(tm[3]),
                      count_device_ms=float(tm[4]), scan_device_ms=float(tm[5]), fill_device_ms=float(tm[6]),
                      filter_device_ms=float(tm[7]))
    return dict(q_off=q_off, rows=rows[:M], loss=loss[:M], timers=timers)


# ---- upstream's one-task functions ----
def _one_task(ref_lines, tgt_lines, ref_cam, ref_pose, tgt_cam, tgt_pose, pairs):
    tgt = _lines4(tgt_lines)
    return scene_arrays([_cam11(tgt_cam, tgt_pose)], [tgt], [np.arange(len(tgt))], [_cam11(ref_cam, ref_pose)],
                        [_lines4(ref_lines)], [[0]], None if pairs is None else [[pairs]], np.zeros((len(tgt), 6)))


def match_line_2to2_epipolarIoU(ref_lines, tgt_lines, ref_cam, ref_pose, tgt_cam, tgt_pose, IoU_threshold, host=False):
    """functions.py:6-23 -> the (ref line, tgt line) pairs above the threshold, ref-major.  One all_pairs task in which
    every target line is its own track."""
    sc = _one_task(ref_lines, tgt_lines, ref_cam, ref_pose, tgt_cam, tgt_pose, None)
    rows = match_lines_arrays(sc, "all_pairs", IoU_threshold=IoU_threshold, host=host)["rows"]
    return [(int(i), int(j)) for i, j in rows]


def filter_line_2to2_epipolarIoU(pairs, ref_lines, tgt_lines, ref_cam, ref_pose, tgt_cam, tgt_pose, IoU_threshold, host=False):
    """functions.py:26-51 -> the pairs of the list that pass, in the list's order.  One listed_filtered task; the test is a
    function of the pair alone, so the kept set decides every occurrence."""
    plist = [(int(p[0]), int(p[1])) for p in pairs]
    if not plist:
        return []
    sc = _one_task(ref_lines, tgt_lines, ref_cam, ref_pose, tgt_cam, tgt_pose, np.array(plist, np.int64).reshape(-1, 2))
    kept = {(int(i), int(j)) for i, j in match_lines_arrays(sc, "listed_filtered", IoU_threshold=IoU_threshold, host=host)["rows"]}
    return [p for p in plist if p in kept]


def match_line_2to3(pairs_2to2, line2track, tgt_img_id):
    """functions.py:54-63: a lookup, kept in Python (the list's order is the result's)"""
    track_ids = line2track[tgt_img_id]
    out = []
    for pair in pairs_2to2:
        i, j = int(pair[0]), int(pair[1])
        if track_ids[j] != -1:
            out.append((i, track_ids[j]))
    return out


def _track6(linetracks):
    if isinstance(linetracks, np.ndarray):
        return _f64(linetracks, 6, "tracks")
    return (np.array([_hl._l3(t.line if hasattr(t, "line") else t) for t in linetracks], float).reshape(-1, 6)
            if len(linetracks) else np.zeros((0, 6)))


def reprojection_filter_matches_2to3(ref_lines, ref_camview, all_pairs_2to3, linetracks, dist_thres=10, sine_thres=0.4,
                                     angle_scale=1.0, dist_func=midpoint_dist, host=False):
    """functions.py:96-140 -> at most one (ref line, best track) per key of all_pairs_2to3, in the dict's order.  One
    listed task over a stand-in image whose line t belongs to track t."""
    kind = _filter_kind(dist_func)
    if kind == 0:
        raise ValueError(f"{WHO}: the reprojection filter needs a dist_func")
    t6 = _track6(linetracks)
    plist = [(int(i), int(t)) for i, ts in all_pairs_2to3.items() for t in ts]
    if not plist:
        return []
    cam = _cam11(ref_camview)
    sc = scene_arrays([cam], [np.zeros((len(t6), 4))], [np.arange(len(t6))], [cam], [_lines4(ref_lines)], [[0]],
                      [[np.array(plist, np.int64).reshape(-1, 2)]], t6)
    rows = match_lines_arrays(sc, "listed", dist_func=dist_func, dist_thres=dist_thres, sine_thres=sine_thres,
                              angle_scale=angle_scale, host=host)["rows"]
    return [(int(i), int(t)) for i, t in rows]


# ---- the batch call ----
def _load_matches(line_matches_2to2, qid):
    if isinstance(line_matches_2to2, (str, os.PathLike)):
        return np.load(os.path.join(line_matches_2to2, f"matches_{qid}.npy"), allow_pickle=True).item()
    return line_matches_2to2[qid]


def _mode_of(cfg_loc):
    if cfg_loc["2d_matcher"] not in MATCHERS:
        raise ValueError("Unknown 2d line matcher: {}".format(cfg_loc["2d_matcher"]))
    if cfg_loc["2d_matcher"] == "epipolar":
        return "all_pairs"
    return "listed_filtered" if cfg_loc.get("epipolar_filter") else "listed"


def match_lines_2to3_scene(cfg_loc, imagecols_db, imagecols_query, all_db_segs, all_query_segs, linemap_db, retrieved,
                           line_matches_2to2=None, host=False, host_threads=None, dist_thres=2, return_arrays=False):
    """runners/hybrid_localization.py:277-340 for all queries in one set of launches -> dict qid -> (M, 2) int array of
    (query line, track id) in upstream's order.  cfg_loc: the `localization` block (2d_matcher, epipolar_filter,
    IoU_threshold, reprojection_filter); retrieved: qid -> [db ids]; line_matches_2to2 (any matcher but "epipolar"):
    qid -> {db id -> (M, 2+) array}, or a directory of matches_{qid}.npy.  dist_thres is the runner's 2."""
    mode = _mode_of(cfg_loc)
    name = cfg_loc.get("reprojection_filter")
    dist_func = None if name is None else get_reprojection_dist_func(name)
    db_ids = list(imagecols_db.get_img_ids())
    row_of = {i: k for k, i in enumerate(db_ids)}
    qids = list(retrieved.keys())
    line2track = base.get_invert_idmap_from_linetracks({i: all_db_segs[i] for i in db_ids}, linemap_db)
    tasks = []
    for qid in qids:
        for d in retrieved[qid]:
            if d not in row_of:
                raise ValueError(f"{WHO}: query {qid} retrieves image {d}, which the database does not hold")
        tasks.append([row_of[d] for d in retrieved[qid]])
    pairs = None
    if mode != "all_pairs":
        if line_matches_2to2 is None:
            raise ValueError(f"{WHO}: the {cfg_loc['2d_matcher']!r} matcher needs line_matches_2to2")
        pairs = []
        for qid in qids:
            m = _load_matches(line_matches_2to2, qid)
            pairs.append([np.asarray(m[d]) for d in retrieved[qid]])
    sc = scene_arrays([imagecols_db.camview(i) for i in db_ids], [all_db_segs[i] for i in db_ids],
                      [line2track[i] for i in db_ids], [imagecols_query.camview(q) for q in qids],
                      [all_query_segs[q] for q in qids], tasks, pairs, _track6(linemap_db))
    res = match_lines_arrays(sc, mode, dist_func=dist_func, IoU_threshold=cfg_loc["IoU_threshold"], dist_thres=dist_thres,
                             host=host, host_threads=host_threads)
    out = {qid: res["rows"][res["q_off"][n]:res["q_off"][n + 1]].astype(np.int64) for n, qid in enumerate(qids)}
    return (out, sc, res) if return_arrays else out


# ---- the runner ----
class _Pose:
    """a query's coarse pose with the quaternion as given (the native code normalises it as CameraPose does)"""

    def __init__(self, qvec, tvec):
        self.qvec, self.tvec = np.asarray(qvec, float).reshape(4), np.asarray(tvec, float).reshape(3)

    def R(self):
        return _hl._rotation(self.qvec)

    def T(self):
        return self.tvec


def estimator_queries(imagecols_query, all_query_segs, tracks6, matches, point_corresp, qids, compact=True):
    """The estimator's query dicts.  compact: a query hands over only the tracks its matches name, ids remapped (the
    ingest of the estimator is per element, so all tracks for every query would scale with tracks x queries); the 3D
    line behind every correspondence is the same either way."""
    out = []
    for qid in qids:
        view = imagecols_query.camview(qid)
        m = np.asarray(matches[qid], np.int64).reshape(-1, 2)
        segs = _lines4(all_query_segs[qid])
        ids = m[:, 1]
        if compact:
            used, ids = np.unique(ids, return_inverse=True) if len(ids) else (np.zeros(0, np.int64), ids)
            l3ds = tracks6[used]
        else:
            l3ds = tracks6
        pc = point_corresp[qid]
        out.append(dict(l3ds=l3ds.reshape(-1, 2, 3), l3d_ids=np.asarray(ids, np.int64).reshape(-1), l2ds=segs[m[:, 0]].reshape(-1, 2, 2),
                        p3ds=pc["p3ds"], p2ds=pc["p2ds"], camera=np.asarray(view.kvec, float),
                        campose=_Pose(getattr(view, "_qvec_given", view.qvec), view.tvec), inliers_point=pc.get("inliers")))
    return out


def _pose_line(name, pose):
    return " ".join([name] + [str(x) for x in pose.qvec] + [str(x) for x in pose.tvec]) + "\n"


def hybrid_localization(cfg, imagecols_db, imagecols_query, point_corresp, linemap_db, retrieval, results_path,
                        img_name_dict=None, logger=None, *, all_db_segs, all_query_segs, line_matches_2to2=None, host=False,
                        seed=None):
    """runners/hybrid_localization.py:142-398: 2D-3D line matches for every query, one pose per query from points and
    lines, the results file -> {qid: CameraPose}.  `retrieval` maps a query's image name to the names of its retrieved
    database images.  all_db_segs / all_query_segs (img id -> (n, 4+) segments) stand where upstream detects lines.
    ransac.method "hybrid" estimates all queries that were not skipped in one batch; None goes query by query."""
    from . import estimators
    loc = cfg["localization"]
    _mode_of(loc)
    train_ids, query_ids = list(imagecols_db.get_img_ids()), list(imagecols_query.get_img_ids())
    if img_name_dict is None:
        img_name_dict = {i: imagecols_db.image_name(i) for i in train_ids}
        img_name_dict.update({i: imagecols_query.image_name(i) for i in query_ids})
    id_to_name = img_name_dict
    name_to_id = {img_name_dict[i]: i for i in train_ids + query_ids}
    results_path = Path(results_path)
    pose_dir = results_path.parent / "poses_{}".format(loc["2d_matcher"])
    final_poses, todo = {}, []
    for qid in query_ids:
        if loc["skip_exists"]:
            os.makedirs(pose_dir, exist_ok=True)
            f = pose_dir / f"{qid}.txt"
            if f.exists():
                data = f.read_text().rstrip().split("\n")[0].split()
                final_poses[qid] = _hl.CameraPose(np.array(data[1:5], float), np.array(data[5:8], float))
                continue
        todo.append(qid)
    retrieved = {qid: [name_to_id[n] for n in retrieval[id_to_name[qid]]] for qid in todo}
    matches = match_lines_2to3_scene(loc, imagecols_db, imagecols_query, all_db_segs, all_query_segs, linemap_db, retrieved,
                                     line_matches_2to2=line_matches_2to2, host=host)
    if logger:
        for qid in todo:
            logger.info(f"Query Image ID: {qid}: {len(matches[qid])} line matches found for {len(all_query_segs[qid])} 2D lines")
    queries = estimator_queries(imagecols_query, all_query_segs, _track6(linemap_db), matches, point_corresp, todo)
    if estimators._method(loc) is None:
        poses = [estimators.pl_estimate_absolute_pose(loc, q["l3ds"], q["l3d_ids"], q["l2ds"], q["p3ds"], q["p2ds"], q["camera"],
                                                      q["campose"], inliers_point=q["inliers_point"], logger=logger, host=host)[0]
                 for q in queries]
    else:
        poses = [p for p, _ in estimators.pl_estimate_absolute_pose_batch(loc, queries, host=host, seed=seed)] if queries else []
    for qid, pose in zip(todo, poses):
        if loc["skip_exists"]:
            (pose_dir / f"{qid}.txt").write_text(_pose_line(id_to_name[qid], pose))
        final_poses[qid] = pose
    with open(results_path, "w") as f:
        f.writelines([_pose_line(id_to_name[qid], final_poses[qid]) for qid in query_ids])
    return final_poses


def get_hloc_keypoints_from_log(logs, query_img_name, ref_sfm=None, resize_scales=None):
    """runners/hybrid_localization.py:74-91 -> (p2ds, p3ds, inliers) of a query from HLoc's localization log.  Without
    ref_sfm (InLoc) the log carries the 3D points; with it, their ids in the reconstruction.  resize_scales maps a query
    name to the factor its keypoints are scaled back by (pixel centres at +0.5)."""
    entry = logs["loc"][query_img_name]
    p2ds = np.array(entry["keypoints_query"])
    if ref_sfm is None:
        p3ds = np.array(entry["3d_points"])
    else:
        p3ds = np.array([ref_sfm.points3D[j].xyz for j in entry["points3D_ids"]])
    if resize_scales is not None and query_img_name in resize_scales:
        p2ds = (p2ds + 0.5) * resize_scales[query_img_name] - 0.5
    return p2ds, p3ds, entry["PnP_ret"]["inlier_mask"]
