"""A literal NumPy / Python restatement of limap's PL_Bipartite2d (structures/pl_bipartite.cc, base/linebase.cc,
base/graph.cc:157-166, util/kd_tree.h:96-98): slow, in the reference's operation order, IEEE double without
contraction.  tests/test_bpt_host.py holds it to the goldens the reference's own code wrote; tests/test_gpu_bpt.py holds
the device to it on larger scenes.  Lines are named by their index in the (M, 4) array, which is their id order."""
import math

import numpy as np

EPS = 1e-12  # util/types.h:35
DEFAULT_CFG = dict(threshold_keypoints=2.0, threshold_intersection=2.0, threshold_merge_junctions=2.0)


def config(d=None):
    """ASSIGN_PYDICT_ITEM: present keys overwrite, unknown keys are ignored"""
    c = dict(DEFAULT_CFG)
    for k in c:
        if d and k in d:
            c[k] = float(d[k])
    return c


def prep(lines):
    """Line2d::direction(), length(), coords() per line: dict of (M,) arrays"""
    a = np.asarray(lines, np.float64).reshape(-1, 4)
    sx, sy, ex, ey = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    vx, vy = ex - sx, ey - sy
    z = vx * vx + vy * vy
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.sqrt(z)
        dx = np.where(z > 0, vx / n, vx)  # normalized(): unchanged unless the squared norm is > 0
        dy = np.where(z > 0, vy / n, vy)
    wx, wy = sx - ex, sy - ey
    length = np.sqrt(wx * wx + wy * wy)
    # homogeneous(start).cross(homogeneous(end)).normalized()
    c0, c1, c2 = sy * 1.0 - 1.0 * ey, 1.0 * ex - sx * 1.0, sx * ey - sy * ex
    zc = (c0 * c0 + c1 * c1) + c2 * c2
    with np.errstate(invalid="ignore", divide="ignore"):
        nc = np.sqrt(zc)
        c0, c1, c2 = (np.where(zc > 0, c / nc, c) for c in (c0, c1, c2))
    return dict(sx=sx, sy=sy, ex=ex, ey=ey, dx=dx, dy=dy, len=length, c0=c0, c1=c1, c2=c2)


def point_line_dists(lines, pts):
    """Line2d::point_distance of every point (rows) to every line (columns)"""
    L = prep(lines)
    p = np.asarray(pts, np.float64).reshape(-1, 2)
    px, py = p[:, 0:1], p[:, 1:2]
    proj = (px - L["sx"]) * L["dx"] + (py - L["sy"]) * L["dy"]
    qx = np.where(proj < 0, L["sx"], np.where(proj > L["len"], L["ex"], L["sx"] + proj * L["dx"]))
    qy = np.where(proj < 0, L["sy"], np.where(proj > L["len"], L["ey"], L["sy"] + proj * L["dy"]))
    ux, uy = px - qx, py - qy
    return np.sqrt(ux * ux + uy * uy)


def associate(lines, pts, th):
    """add_keypoint: per point the ascending indices of the lines with !(dist > th)"""
    if np.asarray(lines).size == 0:
        return [np.zeros(0, np.int64) for _ in range(np.asarray(pts).reshape(-1, 2).shape[0])]
    d = point_line_dists(lines, pts)
    return [np.flatnonzero(~(row > th)) for row in d]


def intersect_row(L, i, th):
    """intersect(line i, line j) for every j > i: (hit mask, x, y) over j = i + 1 .."""
    j = slice(i + 1, None)
    s1x, s1y, e1x, e1y = L["sx"][i], L["sy"][i], L["ex"][i], L["ey"][i]
    s2x, s2y, e2x, e2y = L["sx"][j], L["sy"][j], L["ex"][j], L["ey"][j]

    def norm(x, y):
        return np.sqrt(x * x + y * y)
    t = [norm(s1x - s2x, s1y - s2y) <= th, norm(e1x - s2x, e1y - s2y) <= th,
         norm(s1x - e2x, s1y - e2y) <= th, norm(e1x - e2x, e1y - e2y) <= th]
    mids = [((s1x + s2x) / 2.0, (s1y + s2y) / 2.0), ((e1x + s2x) / 2.0, (e1y + s2y) / 2.0),
            ((s1x + e2x) / 2.0, (s1y + e2y) / 2.0), ((e1x + e2x) / 2.0, (e1y + e2y) / 2.0)]
    a0, a1, a2 = L["c0"][i], L["c1"][i], L["c2"][i]
    b0, b1, b2 = L["c0"][j], L["c1"][j], L["c2"][j]
    h0, h1, h2 = a1 * b2 - a2 * b1, a2 * b0 - a0 * b2, a0 * b1 - a1 * b0
    z = (h0 * h0 + h1 * h1) + h2 * h2
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        n = np.sqrt(z)
        h0, h1, h2 = (np.where(z > 0, h / n, h) for h in (h0, h1, h2))
        px, py = h0 / (h2 + EPS), h1 / (h2 + EPS)
        proj1 = (px - s1x) * L["dx"][i] + (py - s1y) * L["dy"][i]
        err1 = np.where(proj1 < 0.0, -proj1, 0.0)
        err1 = np.where(proj1 > L["len"][i], proj1 - L["len"][i], err1)
        proj2 = (px - s2x) * L["dx"][j] + (py - s2y) * L["dy"][j]
        err2 = np.where(proj2 < 0.0, -proj2, 0.0)
        err2 = np.where(proj2 > L["len"][j], proj2 - L["len"][j], err2)
        hit, x, y = ~(err1 + err2 > th), px, py
    for k in (3, 2, 1, 0):  # the first test that holds wins
        hit = np.where(t[k], True, hit)
        x = np.where(t[k], mids[k][0], x)
        y = np.where(t[k], mids[k][1], y)
    return hit, x, y


def intersections(lines, th):
    """the accepted intersections in the order of pl_bipartite.cc:112-124: (K, 2) line indices, (K, 2) points"""
    L = prep(lines)
    M = L["sx"].shape[0]
    ij, xy = [], []
    for i in range(M - 1):
        hit, x, y = intersect_row(L, i, th)
        js = np.flatnonzero(hit)
        ij.append(np.stack([np.full(js.shape, i), js + i + 1], 1))
        xy.append(np.stack([x[js], y[js]], 1))
    if not ij:
        return np.zeros((0, 2), np.int64), np.zeros((0, 2))
    return np.concatenate(ij, 0).astype(np.int64), np.concatenate(xy, 0)


def candidates(lines, th):
    """the junction candidates: both endpoints per line, then the intersections: xy (J, 2), lines (J, 2; -1: none)"""
    a = np.asarray(lines, np.float64).reshape(-1, 4)
    M = a.shape[0]
    ij, ixy = intersections(a, th)
    xy = np.concatenate([a.reshape(-1, 2), ixy], 0)
    ln = np.concatenate([np.stack([np.repeat(np.arange(M), 2), np.full(2 * M, -1)], 1), ij], 0).astype(np.int64)
    return xy, ln


def find_root(parents, k):
    """union_find_get_root with its path compression (the recursion unrolled: same final array)"""
    r = k
    while parents[r] != -1:
        r = parents[r]
    while parents[k] != -1:
        parents[k], k = r, parents[k]
    return r


def merge_full(xy, th):
    """pl_bipartite.cc:128-143 literally: every pair i < j, two root look-ups each.  O(J^2)."""
    J = xy.shape[0]
    parents = [-1] * J
    X, Y = xy[:, 0].tolist(), xy[:, 1].tolist()
    for i in range(J - 1):
        for j in range(i + 1, J):
            ri, rj = find_root(parents, i), find_root(parents, j)
            if ri == rj:
                continue
            dx, dy = X[i] - X[j], Y[i] - Y[j]
            if math.sqrt(dx * dx + dy * dy) > th:
                continue
            parents[j] = i
    return parents


def close_pairs(xy, th):
    """the pairs i < j with !(dist > th), lexicographic"""
    out = []
    for i in range(xy.shape[0] - 1):
        dx, dy = xy[i, 0] - xy[i + 1:, 0], xy[i, 1] - xy[i + 1:, 1]
        js = np.flatnonzero(~(np.sqrt(dx * dx + dy * dy) > th))
        out.append(np.stack([np.full(js.shape, i), js + i + 1], 1))
    return np.concatenate(out, 0) if out else np.zeros((0, 2), np.int64)


def merge_sparse(xy, th, pairs=None):
    """the same loop over the close pairs only (DESIGN section 16 argues, and test_bpt_host.py checks, that the roots
    are those of merge_full)"""
    parents = [-1] * xy.shape[0]
    for i, j in (close_pairs(xy, th) if pairs is None else pairs).tolist():
        if find_root(parents, i) != find_root(parents, j):
            parents[j] = i
    return parents


def roots(parents):
    p = list(parents)
    return [find_root(p, k) for k in range(len(p))]


def nearest_dists(kps, q):
    """KDTree::point_distance as the exact minimum: sqrt of the smallest (dx*dx + dy*dy) + dz*dz, dz = 0"""
    k = np.asarray(kps, np.float64).reshape(-1, 2)
    out = np.zeros(q.shape[0])
    for n in range(q.shape[0]):
        ux, uy = q[n, 0] - k[:, 0], q[n, 1] - k[:, 1]
        out[n] = math.sqrt(((ux * ux + uy * uy) + 0.0 * 0.0).min())
    return out


def junctions(lines, kps, cfg=None, full=False):
    """compute_intersection_with_points on a bipartite of the lines alone: dict(xy (J, 2), line_ids list of lists,
    cand_xy, cand_lines, parents (after the last root look-ups), roots, merged_xy, pairs (the close pairs; None with
    full=True))"""
    c = config(cfg)
    a = np.asarray(lines, np.float64).reshape(-1, 4)
    kps = np.asarray(kps, np.float64).reshape(-1, 2)
    if a.shape[0] == 0:  # the reference's loop bounds wrap around: defined here as no junction
        return dict(xy=np.zeros((0, 2)), line_ids=[], cand_xy=np.zeros((0, 2)), cand_lines=np.zeros((0, 2), np.int64),
                    parents=[], roots=[], merged_xy=np.zeros((0, 2)), pairs=np.zeros((0, 2), np.int64))
    xy, ln = candidates(a, c["threshold_intersection"])
    th = c["threshold_merge_junctions"]
    pairs = None if full else close_pairs(xy, th)
    parents = merge_full(xy, th) if full else merge_sparse(xy, th, pairs)
    rt = [find_root(parents, k) for k in range(len(parents))]  # pl_bipartite.cc:145-146
    groups = {}
    for k, r in enumerate(rt):
        groups.setdefault(r, []).append(k)
    mxy, mids = [], []
    for r in sorted(groups):  # std::map order
        px = py = 0.0
        ids = set()
        for k in groups[r]:  # merge_junctions
            px += float(xy[k, 0])
            py += float(xy[k, 1])
            ids.update(int(x) for x in ln[k] if x >= 0)
        n = len(groups[r])
        mxy.append((px / n, py / n))
        mids.append(sorted(ids))
    mxy = np.array(mxy, np.float64).reshape(-1, 2)
    keep = np.ones(mxy.shape[0], bool)
    if kps.shape[0]:  # `if (!tree.empty())`
        keep = ~(nearest_dists(kps, mxy) < th)
    return dict(xy=mxy[keep], line_ids=[m for m, k in zip(mids, keep) if k], cand_xy=xy, cand_lines=ln,
                parents=parents, roots=rt, merged_xy=mxy, pairs=pairs)


def bipartite_dict(lines, xy, point3D_ids, ids, cfg=None, line_ids=None):
    """init_lines + add_keypoints_with_point3D_ids as the as_dict() of the result"""
    c = config(cfg)
    a = np.asarray(lines, np.float64).reshape(-1, 4)
    lids = list(range(a.shape[0])) if line_ids is None else [int(x) for x in line_ids]
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    nb = associate(a, xy, c["threshold_keypoints"])
    d = dict(points_={}, lines_={l: a[k].reshape(2, 2) for k, l in enumerate(lids)}, np2l_={},
             nl2p_={l: set() for l in lids})
    for k in range(xy.shape[0]):
        pid = int(ids[k])
        d["points_"][pid] = dict(p=xy[k].copy(), point3D_id=int(point3D_ids[k]))
        d["np2l_"][pid] = {lids[x] for x in nb[k].tolist()}
        for x in nb[k].tolist():
            d["nl2p_"][lids[x]].add(pid)
    return d
