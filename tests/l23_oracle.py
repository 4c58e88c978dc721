"""Restatement of the 2D-3D line matching of limap's localization runner in plain Python with
scalar arithmetic: the loops of runners/hybrid_localization.py:277-340 over the functions of
optimize/hybrid_localization/functions.py, written from the definition.  Test infrastructure: imports nothing from the
product.  The epipolar IoU and the projection are the C checker's (`ora`: compute_epipolar_IoU, cam_project), which is
pinned to the reference's sources; everything else is scalar float arithmetic in the definition's order.

A scene is a dict: db_cams (n, 11), db_segs (per image (n, 4)), db_tracks (per image the track id per segment, -1:
none), q_cams, q_segs, tasks (per query the database image rows in retrieval order), pairs (per query, per task, (m, 2)
or None), tracks6 (T, 6)."""
import math

import numpy as np

INF = float("inf")


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _sqrt(x):
    return math.sqrt(x) if x >= 0.0 else float("nan")


def length(l):  # Line2d::length: |start - end|
    x, y = l[0] - l[2], l[1] - l[3]
    return _sqrt(x * x + y * y)


def direction(l):  # Line2d::direction: (end - start).normalized(), unchanged where the squared norm is not > 0
    x, y = l[2] - l[0], l[3] - l[1]
    z = x * x + y * y
    if z > 0.0:
        n = _sqrt(z)
        return _div(x, n), _div(y, n)
    return x, y


def midpoint(l):
    return (l[0] + l[2]) * 0.5, (l[1] + l[3]) * 0.5


def cross(a, b):
    return a[0] * b[1] - a[1] * b[0]


def midpoint_dist(ref, tgt):
    a, b = midpoint(ref), midpoint(tgt)
    x, y = a[0] - b[0], a[1] - b[1]
    return _sqrt(x * x + y * y)


def midpoint_perpendicular_dist(ref, tgt):
    m, d = midpoint(ref), direction(tgt)
    return _div(abs(cross(d, (tgt[0] - m[0], tgt[1] - m[1]))), length(ref))


def perpendicular_dist(ref, tgt):
    d = direction(tgt)
    return 0.5 * (abs(cross(d, (tgt[0] - ref[0], tgt[1] - ref[1]))) + abs(cross(d, (tgt[0] - ref[2], tgt[1] - ref[3]))))


DIST = {"Perpendicular": perpendicular_dist, "Midpoint": midpoint_dist, "Midpoint_Perpendicular": midpoint_perpendicular_dist}


def get_invert_idmap(n_lines, tracks):
    """n_lines: img id -> number of 2D lines; tracks: list of (image ids, line ids); later tracks overwrite earlier ones"""
    out = {i: [-1] * n for i, n in n_lines.items()}
    for t, (imgs, lines) in enumerate(tracks):
        for i, l in zip(imgs, lines):
            out[i][l] = t
    return out


def match_2to2(ora, q_segs, q_cam, d_segs, d_cam, thr):
    return [(i, j) for i in range(len(q_segs)) for j in range(len(d_segs))
            if ora.compute_epipolar_IoU(q_segs[i], q_cam, d_segs[j], d_cam) > thr]


def filter_2to2(ora, pairs, q_segs, q_cam, d_segs, d_cam, thr):
    return [(int(i), int(j)) for i, j in pairs if ora.compute_epipolar_IoU(q_segs[int(i)], q_cam, d_segs[int(j)], d_cam) > thr]


def candidate(ora, name, ref, cam, t6, dist_thres, sine_thres, angle_scale):
    """(loss, kept) of one candidate track of a query line"""
    a, b = ora.cam_project(cam, t6[:3]), ora.cam_project(cam, t6[3:])
    l2d = (float(a[0]), float(a[1]), float(b[0]), float(b[1]))
    dist = DIST[name](ref, l2d)
    loss = dist
    if name == "Midpoint":
        dr, dd = direction(ref), direction(l2d)
        cosine = dr[0] * dd[0] + dr[1] * dd[1]
        cosine = -1.0 if cosine < -1.0 else (1.0 if cosine > 1.0 else cosine)
        sine = _sqrt(1.0 - cosine * cosine)
        loss = loss + angle_scale * length(l2d) * sine
        if sine > sine_thres:
            return loss, False
    if dist > dist_thres:
        return loss, False
    return loss, True


def reprojection_filter(ora, name, q_segs, q_cam, lists, tracks6, dist_thres=10.0, sine_thres=0.4, angle_scale=1.0):
    """lists: dict line -> track ids, in insertion order -> [(line, best track, loss)]"""
    out = []
    for i, ids in lists.items():
        ref = tuple(float(v) for v in q_segs[i])
        best, best_loss = None, INF
        for t in sorted(set(int(v) for v in ids)):
            loss, kept = candidate(ora, name, ref, q_cam, tracks6[t], dist_thres, sine_thres, angle_scale)
            if kept and loss < best_loss:
                best, best_loss = t, loss
        if best is not None:
            out.append((i, best, best_loss))
    return out


def match_scene(ora, sc, mode="all_pairs", filt=None, thr=0.2, dist_thres=10.0, sine_thres=0.4, angle_scale=1.0):
    """-> q_off (Q + 1), rows [(line, track)], loss (zeros without a filter)"""
    q_off, rows, losses = [0], [], []
    for q in range(len(sc["q_cams"])):
        q_segs, q_cam = np.asarray(sc["q_segs"][q], float).reshape(-1, 4), sc["q_cams"][q]
        lists = {}
        for k, img in enumerate(sc["tasks"][q]):
            d_segs, d_cam = np.asarray(sc["db_segs"][img], float).reshape(-1, 4), sc["db_cams"][img]
            if mode == "all_pairs":
                pairs = match_2to2(ora, q_segs, q_cam, d_segs, d_cam, thr)
            elif mode == "listed":
                pairs = [(int(i), int(j)) for i, j in np.asarray(sc["pairs"][q][k]).reshape(-1, 2)]
            else:
                pairs = filter_2to2(ora, np.asarray(sc["pairs"][q][k]).reshape(-1, 2), q_segs, q_cam, d_segs, d_cam, thr)
            for i, j in pairs:
                t = int(sc["db_tracks"][img][j])
                if t != -1:
                    lists.setdefault(i, []).append(t)
        if filt is None:
            new = [(i, t, 0.0) for i in lists for t in lists[i]]
        else:
            new = reprojection_filter(ora, filt, q_segs, q_cam, lists, np.asarray(sc["tracks6"], float).reshape(-1, 6), dist_thres,
                                      sine_thres, angle_scale)
        rows += [(i, t) for i, t, _ in new]
        losses += [l for _, _, l in new]
        q_off.append(len(rows))
    return np.array(q_off, np.int64), np.array(rows, np.int64).reshape(-1, 2), np.array(losses, float)
