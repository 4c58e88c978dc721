"""limap.structures on the GPU: the 2D point-line bipartite ``PL_Bipartite2d`` with its config (structures/bindings.cc,
pl_bipartite{,_base}.{h,cc} of limap; method names and defaults follow the bindings), plus the two batched forms of
runners/functions_structures.py -- one set of launches for a whole scene instead of one serial pass per image:

    from limap_amd import structures
    bpts = structures.compute_2d_bipartites(all_2d_lines, keypoints, cfg)      # img_id -> PL_Bipartite2d
    triangulator.SetBipartites2d(bpts)                                         # use_pointsfm without limap
    juncs = structures.compute_junctions(all_2d_lines, all_keypoints, cfg)     # img_id -> (J, 2)

Keypoint-line association (``add_keypoint``) and the junctions of ``compute_intersection_with_points`` are computed by
the HIP kernels of lt_kernels_bpt.hip, bit for bit the reference's expressions; the container
methods are plain host bookkeeping.  ``PL_Bipartite3d`` and the VP-line bipartites are out of scope.
"""
import ctypes as C

import numpy as np

from . import _capi, _native

__all__ = ["VP2d", "VPLine_Bipartite2d", "VPLine_Bipartite3d", "PL_Bipartite3d", "GetAllBipartites_VPLine2d",
           "Point2d", "Junction", "PL_Bipartite2dConfig", "PL_Bipartite2d", "compute_2d_bipartites",
           "compute_junctions", "lines2d_array", "timers"]

_context = _capi.per_device_contexts()
_p = _capi.ptr


def timers(device=0):
    """lt_bpt_get_timers of the last native call: host ms of upload, kernels, sorts, download + host replay"""
    return _context(device).module_timers("lt_bpt_get_timers", 4)


class Point2d:
    """base/pointtrack.h: a 2D point and the id of the 3D point it observes (-1: none)"""

    def __init__(self, p=None, point3D_id=-1):
        if isinstance(p, dict):
            p, point3D_id = p["p"], p.get("point3D_id", -1)
        self.p = np.zeros(2) if p is None else np.array(p, np.float64).reshape(2)
        self.point3D_id = int(point3D_id)

    def as_dict(self):
        return {"p": self.p.copy(), "point3D_id": self.point3D_id}


class Junction:
    """structures/pl_bipartite_base.h:19-29: a point and the ids of the lines that meet in it"""

    def __init__(self, p, line_ids=()):
        self.p = p
        self.line_ids = [int(x) for x in line_ids]

    def degree(self):
        return len(self.line_ids)


class PL_Bipartite2dConfig:
    """structures/pl_bipartite.h:22-33: keys that are present overwrite the defaults, unknown keys are ignored"""

    KEYS = ("threshold_keypoints", "threshold_intersection", "threshold_merge_junctions")

    def __init__(self, d=None):
        self.threshold_keypoints = 2.0
        self.threshold_intersection = 2.0
        self.threshold_merge_junctions = 2.0
        if isinstance(d, PL_Bipartite2dConfig):
            d = d.as_dict()
        for k in self.KEYS:
            if d and k in d:
                setattr(self, k, float(d[k]))

    def as_dict(self):
        return {k: getattr(self, k) for k in self.KEYS}

    def _struct(self):
        return _capi.LtBptConfig(self.threshold_keypoints, self.threshold_intersection, self.threshold_merge_junctions)


def lines2d_array(lines):
    """(M, 4 | 5) array (a fifth column is a score), (M, 2, 2) array, list of Line2d or of anything with .start / .end
    -> contiguous (M, 4)"""
    if isinstance(lines, np.ndarray) or (hasattr(lines, "shape") and not isinstance(lines, (list, tuple))):
        a = np.asarray(lines, np.float64)
        if a.ndim == 3 and a.shape[1:] == (2, 2):
            a = a.reshape(-1, 4)
        if a.size == 0:
            a = np.zeros((0, 4))
        if a.ndim != 2 or a.shape[1] not in (4, 5):
            raise ValueError(f"2D lines must be (M, 4), (M, 5) or (M, 2, 2), got shape {a.shape}")
        a = a[:, :4]
    else:
        rows = []
        for ln in lines:
            if hasattr(ln, "start") and hasattr(ln, "end"):
                rows.append(np.concatenate([np.asarray(ln.start, np.float64).reshape(2),
                                            np.asarray(ln.end, np.float64).reshape(2)]))
            else:
                rows.append(np.asarray(ln, np.float64).reshape(-1)[:4])
        a = np.stack(rows, 0) if rows else np.zeros((0, 4))
    a = np.ascontiguousarray(a, np.float64)
    if not np.isfinite(a).all():
        raise ValueError("2D lines: non-finite coordinate")
    return a


def _points2(p, what="points"):
    q = np.asarray(p, np.float64)
    q = np.ascontiguousarray(q.reshape(-1, 2)) if q.size else np.zeros((0, 2))
    if not np.isfinite(q).all():
        raise ValueError(f"{what}: non-finite coordinate")
    return q


def _associate(lines_list, points_list, cfg, device=0):
    """per image the (edge_off, edge_line) CSR of its points: one native call for the batch"""
    ctx = _context(device)
    loff, lflat = _native.csr(lines_list, 4)
    poff, pflat = _native.csr(points_list, 2)
    st = cfg._struct()
    n_edges = C.c_int64(0)
    ctx.chk(ctx.L.lt_bpt_associate(ctx.h, len(lines_list), _p(loff, C.c_int64), _p(lflat), _p(poff, C.c_int64),
                                   _p(pflat), C.byref(st), C.byref(n_edges)))
    eoff = np.zeros(int(poff[-1]) + 1, np.int64)
    edge = np.zeros(max(n_edges.value, 1), np.int32)
    ctx.chk(ctx.L.lt_bpt_associate_get(ctx.h, _p(eoff, C.c_int64), _p(edge, C.c_int32)))
    out = []
    for m in range(len(lines_list)):
        o = eoff[poff[m]:poff[m + 1] + 1]
        out.append((o - o[0], edge[o[0]:o[-1]]))
    return out


def _junctions(lines_list, kps_list, cfg, device=0, candidates=False, sizes=False):
    """per image (xy (J, 2), id_off (J + 1), line indices): one native call for the batch.  candidates: also the
    per-image candidate lists; sizes: also lt_bpt_junctions' sizes[4] (junctions, line indices, candidates, close
    pairs of the whole call)"""
    ctx = _context(device)
    loff, lflat = _native.csr(lines_list, 4)
    koff, kflat = _native.csr(kps_list, 2)
    st = cfg._struct()
    want_sizes, sizes = sizes, np.zeros(4, np.int64)
    n = len(lines_list)
    ctx.chk(ctx.L.lt_bpt_junctions(ctx.h, n, _p(loff, C.c_int64), _p(lflat), _p(koff, C.c_int64), _p(kflat),
                                   C.byref(st), _p(sizes, C.c_int64)))
    joff = np.zeros(n + 1, np.int64)
    xy = np.zeros((max(int(sizes[0]), 1), 2))
    ioff = np.zeros(int(sizes[0]) + 1, np.int64)
    idx = np.zeros(max(int(sizes[1]), 1), np.int32)
    ctx.chk(ctx.L.lt_bpt_junctions_get(ctx.h, _p(joff, C.c_int64), _p(xy), _p(ioff, C.c_int64), _p(idx, C.c_int32)))
    out = []
    for m in range(n):
        o = ioff[joff[m]:joff[m + 1] + 1]
        out.append((xy[joff[m]:joff[m + 1]].copy(), o - o[0], idx[o[0]:o[-1]].copy()))
    if not candidates:
        return (out, sizes) if want_sizes else out
    coff = np.zeros(n + 1, np.int64)
    cxy = np.zeros((max(int(sizes[2]), 1), 2))
    cl = np.zeros((max(int(sizes[2]), 1), 2), np.int32)
    par = np.zeros(max(int(sizes[2]), 1), np.int32)
    ctx.chk(ctx.L.lt_bpt_junctions_get_candidates(ctx.h, _p(coff, C.c_int64), _p(cxy), _p(cl, C.c_int32),
                                                  _p(par, C.c_int32)))
    cands = [dict(xy=cxy[coff[m]:coff[m + 1]].copy(), lines=cl[coff[m]:coff[m + 1]].copy(),
                  parents=par[coff[m]:coff[m + 1]].copy()) for m in range(n)]
    return (out, cands, sizes) if want_sizes else (out, cands)


class _Graph:
    """pl_bipartite_base.h: the bipartite graph over `points_` and `lines_` keyed by id, with the two adjacency maps.  The
    node types, their insertion and their dict form are the subclasses'"""

    def _check(self, cond, msg):
        if not cond:
            raise ValueError("Check failed: " + msg)

    def _new_point_id(self):
        return max(self.points_) + 1 if self.points_ else 0

    def _new_line_id(self):
        return max(self.lines_) + 1 if self.lines_ else 0

    def add_edge(self, point_id, line_id):
        self._check(self.exist_point(point_id), "exist_point(point_id)")
        self._check(self.exist_line(line_id), "exist_line(line_id)")
        self.np2l_[int(point_id)].add(int(line_id))
        self.nl2p_[int(line_id)].add(int(point_id))

    def delete_edge(self, point_id, line_id):
        self._check(self.exist_point(point_id), "exist_point(point_id)")
        self._check(self.exist_line(line_id), "exist_line(line_id)")
        self.np2l_[int(point_id)].discard(int(line_id))
        self.nl2p_[int(line_id)].discard(int(point_id))

    def clear_edges(self):
        for s in self.np2l_.values():
            s.clear()
        for s in self.nl2p_.values():
            s.clear()

    def delete_point(self, point_id):
        self._check(self.exist_point(point_id), "exist_point(point_id)")
        for line_id in self.np2l_.pop(int(point_id)):
            self.nl2p_[line_id].discard(int(point_id))
        del self.points_[int(point_id)]

    def delete_line(self, line_id):
        self._check(self.exist_line(line_id), "exist_line(line_id)")
        for point_id in self.nl2p_.pop(int(line_id)):
            self.np2l_[point_id].discard(int(line_id))
        del self.lines_[int(line_id)]

    def clear_points(self):
        self.points_.clear()
        self.clear_edges()
        self.np2l_.clear()

    def clear_lines(self):
        self.lines_.clear()
        self.clear_edges()
        self.nl2p_.clear()

    def reset(self):
        self.points_.clear()
        self.lines_.clear()
        self.np2l_.clear()
        self.nl2p_.clear()

    def count_lines(self):
        return len(self.lines_)

    def count_points(self):
        return len(self.points_)

    def count_edges(self):
        return sum(len(s) for s in self.nl2p_.values())

    def exist_point(self, point_id):
        return int(point_id) in self.points_

    def exist_line(self, line_id):
        return int(line_id) in self.lines_

    def get_dict_points(self):
        return {k: self.points_[k] for k in sorted(self.points_)}

    def get_all_points(self):
        return [self.points_[k] for k in sorted(self.points_)]

    def get_point_ids(self):
        return sorted(self.points_)

    def get_line_ids(self):
        return sorted(self.lines_)

    def pdegree(self, point_id):
        self._check(self.exist_point(point_id), "exist_point(point_id)")
        return len(self.np2l_[int(point_id)])

    def ldegree(self, line_id):
        self._check(self.exist_line(line_id), "exist_line(line_id)")
        return len(self.nl2p_[int(line_id)])

    def neighbor_lines(self, point_id):
        self._check(self.exist_point(point_id), "exist_point(point_id)")
        return sorted(self.np2l_[int(point_id)])

    def neighbor_points(self, line_id):
        self._check(self.exist_line(line_id), "exist_line(line_id)")
        return sorted(self.nl2p_[int(line_id)])

    def point(self, point_id):
        self._check(self.exist_point(point_id), "exist_point(point_id)")
        return self.points_[int(point_id)]


class PL_Bipartite2d(_Graph):
    """structures/pl_bipartite.h:35-60 over pl_bipartite_base.h: points, lines and their edges, keyed by id"""

    def __init__(self, cfg=None, device=0):
        self.device = int(device)
        self.points_, self.lines_, self.np2l_, self.nl2p_ = {}, {}, {}, {}
        if isinstance(cfg, PL_Bipartite2d):  # the copy constructor keeps the content and takes a default config
            self.config_ = PL_Bipartite2dConfig()
            self._load(cfg.as_dict())
        elif isinstance(cfg, dict) and ("points_" in cfg or "lines_" in cfg):
            self.config_ = PL_Bipartite2dConfig()
            self._load(cfg)
        else:
            self.config_ = PL_Bipartite2dConfig(cfg)

    # ---- dict form (pl_bipartite.cc:11-54) --------------------------------------------------------------------------
    def _load(self, d):
        for key in ("points_", "lines_"):
            if key not in d:
                raise RuntimeError(f'Error! Key "{key}" does not exist!')
        self.points_ = {int(k): Point2d(v) if isinstance(v, dict) else Point2d(v.p, v.point3D_id)
                        for k, v in d["points_"].items()}
        self.lines_ = {int(k): np.array(v, np.float64).reshape(2, 2) for k, v in d["lines_"].items()}
        self.np2l_ = {int(k): {int(x) for x in v} for k, v in d.get("np2l_", {}).items()}
        self.nl2p_ = {int(k): {int(x) for x in v} for k, v in d.get("nl2p_", {}).items()}

    def as_dict(self):
        return {"points_": {k: self.points_[k].as_dict() for k in sorted(self.points_)},
                "lines_": {k: self.lines_[k].copy() for k in sorted(self.lines_)},
                "np2l_": {k: set(self.np2l_[k]) for k in sorted(self.np2l_)},
                "nl2p_": {k: set(self.nl2p_[k]) for k in sorted(self.nl2p_)}}

    # ---- insertion and deletion (pl_bipartite_base.cc:37-209) ---------------------------------------------------------
    def add_point(self, p, point_id=-1, neighbors=()):
        point_id = int(point_id)
        if point_id == -1:
            point_id = self._new_point_id()
        self._check(not self.exist_point(point_id), "!exist_point(point_id)")
        self.points_[point_id] = p if isinstance(p, Point2d) else Point2d(p)
        self.np2l_[point_id] = set()
        for line_id in neighbors:
            self._check(self.exist_line(line_id), "exist_line(line_id)")
            self.np2l_[point_id].add(int(line_id))
            self.nl2p_[int(line_id)].add(point_id)
        return point_id

    def add_line(self, line, line_id=-1, neighbors=()):
        line_id = int(line_id)
        if line_id == -1:
            line_id = self._new_line_id()
        self._check(not self.exist_line(line_id), "!exist_line(line_id)")
        self.lines_[line_id] = lines2d_array([line]).reshape(2, 2)
        self.nl2p_[line_id] = set()
        for point_id in neighbors:
            self._check(self.exist_point(point_id), "exist_point(point_id)")
            self.nl2p_[line_id].add(int(point_id))
            self.np2l_[int(point_id)].add(line_id)
        return line_id

    def update_point(self, point_id, p):
        self._check(self.exist_point(point_id), "exist_point(point_id)")
        self.points_[int(point_id)] = p if isinstance(p, Point2d) else Point2d(p)

    def update_line(self, line_id, line):
        self._check(self.exist_line(line_id), "exist_line(line_id)")
        self.lines_[int(line_id)] = lines2d_array([line]).reshape(2, 2)

    def init_points(self, points, ids=None):
        ids = list(range(len(points))) if ids is None or len(ids) == 0 else list(ids)
        self._check(len(ids) == len(points), "points.size() == ids.size()")
        for p, i in zip(points, ids):
            self.add_point(p, i)

    def init_lines(self, lines, ids=None):
        a = lines2d_array(lines)
        ids = list(range(a.shape[0])) if ids is None or len(ids) == 0 else [int(i) for i in ids]
        self._check(len(ids) == a.shape[0], "lines.size() == ids.size()")
        for row, i in zip(a, ids):
            self._check(not self.exist_line(i), "!exist_line(line_id)")
            self.lines_[i] = row.reshape(2, 2).copy()
            self.nl2p_[i] = set()

    # ---- const operations (pl_bipartite_base.h:61-87) -------------------------------------------------------------------
    def get_dict_lines(self):
        return {k: self.line(k) for k in sorted(self.lines_)}

    def get_all_lines(self):
        return [self.line(k) for k in sorted(self.lines_)]

    def line(self, line_id):
        from .base import Line2d
        self._check(self.exist_line(line_id), "exist_line(line_id)")
        a = self.lines_[int(line_id)]
        return Line2d(a[0].copy(), a[1].copy())

    def junc(self, point_id):
        return Junction(self.point(point_id), self.neighbor_lines(point_id))

    def get_all_junctions(self):
        return [self.junc(k) for k in sorted(self.points_)]

    def add_junction(self, junction, point_id=-1):
        self.add_point(junction.p, point_id, junction.line_ids)

    # ---- the device paths (pl_bipartite.cc:56-164) ------------------------------------------------------------------------
    def _line_table(self):
        ids = self.get_line_ids()
        a = np.stack([self.lines_[i].reshape(4) for i in ids], 0) if ids else np.zeros((0, 4))
        return np.asarray(ids, np.int64), np.ascontiguousarray(a)

    def _add_associated(self, xy, p3d, ids, line_ids, eoff, edge):
        """add_point for every keypoint, with the lines the device connected it to"""
        for k in range(xy.shape[0]):
            pid = self._new_point_id() if ids is None or int(ids[k]) == -1 else int(ids[k])
            self.add_point(Point2d(xy[k], p3d[k]), pid, line_ids[edge[eoff[k]:eoff[k + 1]]].tolist())

    def add_keypoint(self, p, point_id=-1):
        p = p if isinstance(p, Point2d) else Point2d(p)
        self.add_keypoints_with_point3D_ids([p.p], [p.point3D_id], [point_id])

    def add_keypoints_with_point3D_ids(self, points, point3D_ids, ids=None):
        xy = _points2(points, "keypoints")
        p3d = np.asarray(point3D_ids, np.int64).reshape(-1)
        self._check(xy.shape[0] == p3d.shape[0], "points.size() == point3D_ids.size()")
        if ids is not None and len(ids) == 0:
            ids = None
        if ids is not None:
            self._check(len(ids) == xy.shape[0], "points.size() == ids.size()")
        line_ids, a = self._line_table()
        (eoff, edge), = _associate([a], [xy], self.config_, self.device)
        self._add_associated(xy, p3d, ids, line_ids, eoff, edge)

    def _add_junctions(self, line_ids, res):
        xy, ioff, idx = res
        for k in range(xy.shape[0]):
            self.add_junction(Junction(Point2d(xy[k]), line_ids[idx[ioff[k]:ioff[k + 1]]].tolist()))

    def compute_intersection_with_points(self, points):
        kps = _points2(points, "keypoints")
        line_ids, a = self._line_table()
        res, = _junctions([a], [kps], self.config_, self.device)
        self._add_junctions(line_ids, res)

    def compute_intersection(self):
        pts = [self.points_[k].p for k in sorted(self.points_)]
        self.compute_intersection_with_points(np.array(pts, np.float64).reshape(-1, 2))


def _cfg(cfg):
    return cfg if isinstance(cfg, PL_Bipartite2dConfig) else PL_Bipartite2dConfig(cfg)


def compute_2d_bipartites(all_2d_lines, keypoints, cfg=None, device=0):
    """compute_2d_bipartites_from_colmap (runners/functions_structures.py:81-119) without the COLMAP reading: per image
    init_lines(all_2d_lines[img_id]) and add_keypoints_with_point3D_ids over the keypoints that observe a 3D point.
    keypoints[img_id] = (xy (P, 2), point3D_ids (P,), ids (P,) | None); rows with point3D_id < 0 are dropped first, the
    point ids default to the row numbers before that.  The association of all images is one native call.
    Returns dict img_id -> PL_Bipartite2d."""
    cfg = _cfg(cfg)
    img_ids = sorted(int(k) for k in keypoints)
    bpts, lines, pts, meta = {}, [], [], []
    for i in img_ids:
        kp = keypoints[i]
        xy = _points2(kp[0], "keypoints")
        p3d = np.asarray(kp[1], np.int64).reshape(-1)
        ids = np.arange(xy.shape[0], dtype=np.int64) if len(kp) < 3 or kp[2] is None else \
            np.asarray(kp[2], np.int64).reshape(-1)
        if not (xy.shape[0] == p3d.shape[0] == ids.shape[0]):
            raise ValueError(f"image {i}: keypoints, point3D_ids and ids differ in length")
        mask = p3d >= 0
        b = PL_Bipartite2d(cfg, device=device)
        b.init_lines(all_2d_lines[i])
        bpts[i] = b
        lines.append(b._line_table())
        pts.append(np.ascontiguousarray(xy[mask]))
        meta.append((p3d[mask], ids[mask]))
    if img_ids:
        res = _associate([a for _, a in lines], pts, cfg, device)
        for i, (line_ids, _), xy, (p3d, ids), (eoff, edge) in zip(img_ids, lines, pts, meta, res):
            bpts[i]._add_associated(xy, p3d, ids, line_ids, eoff, edge)
    return bpts


def compute_junctions(all_2d_lines, all_keypoints, cfg=None, device=0):
    """the middle loop of compute_colmap_model_with_junctions (runners/functions_structures.py:62-69): per image the
    junctions compute_intersection_with_points(keypoints) adds to a bipartite that holds the lines only, in ascending
    point-id order.  One native call for all images.  Returns dict img_id -> (J, 2) float64."""
    cfg = _cfg(cfg)
    img_ids = sorted(int(k) for k in all_2d_lines)
    lines = [lines2d_array(all_2d_lines[i]) for i in img_ids]
    kps = [_points2(all_keypoints[i], "keypoints") if i in all_keypoints else np.zeros((0, 2)) for i in img_ids]
    if not img_ids:
        return {}
    res = _junctions(lines, kps, cfg, device)
    return {i: r[0] for i, r in zip(img_ids, res)}


# ---- the containers of limap.runners.pointline_association (structures/vpline_bipartite.h, pl_bipartite.h:62-75): the
# same graph over other node types.  Host containers: nothing here runs on the device ----
class VP2d:
    """vplib/vptrack.h:19: Feature2dWith3dIndex<V3D> -- a homogeneous 2D vanishing point and the id of its 3D track"""

    def __init__(self, p=None, point3D_id=-1):
        if isinstance(p, dict):
            p, point3D_id = p.get("p"), p.get("point3D_id", -1)
        elif isinstance(p, VP2d):
            p, point3D_id = p.p, p.point3D_id
        self.p = np.zeros(3) if p is None else np.array(p, np.float64).reshape(3)
        self.point3D_id = int(point3D_id)

    def as_dict(self):
        return {"p": self.p.copy(), "point3D_id": self.point3D_id}


class _Bipartite(_Graph):
    """pl_bipartite_base.h over other node types: `_point(v)` / `_line(v)` build a node from an object or its dict"""

    def __init__(self, d=None):
        self.points_, self.lines_, self.np2l_, self.nl2p_ = {}, {}, {}, {}
        if isinstance(d, _Bipartite):
            d = d.as_dict()
        if d is not None:
            self._load(d)

    def _load(self, d):
        for key in ("points_", "lines_"):
            if key not in d:
                raise RuntimeError(f'Error! Key "{key}" does not exist!')
        self.points_ = {int(k): self._point(v) for k, v in d["points_"].items()}
        self.lines_ = {int(k): self._line(v) for k, v in d["lines_"].items()}
        self.np2l_ = {int(k): {int(x) for x in v} for k, v in d.get("np2l_", {}).items()}
        self.nl2p_ = {int(k): {int(x) for x in v} for k, v in d.get("nl2p_", {}).items()}
        for k in self.points_:
            self.np2l_.setdefault(k, set())
        for k in self.lines_:
            self.nl2p_.setdefault(k, set())

    def as_dict(self):
        return {"points_": {k: self.points_[k].as_dict() for k in sorted(self.points_)},
                "lines_": {k: self._line_dict(self.lines_[k]) for k in sorted(self.lines_)},
                "np2l_": {k: set(self.np2l_[k]) for k in sorted(self.np2l_)},
                "nl2p_": {k: set(self.nl2p_[k]) for k in sorted(self.nl2p_)}}

    def _line_dict(self, v):
        return v.as_dict()

    def add_point(self, p, point_id=-1, neighbors=()):
        point_id = int(point_id)
        if point_id == -1:
            point_id = self._new_point_id()
        self._check(not self.exist_point(point_id), "!exist_point(point_id)")
        self.points_[point_id] = self._point(p)
        self.np2l_[point_id] = set()
        for line_id in neighbors:
            self.add_edge(point_id, line_id)
        return point_id

    def add_line(self, line, line_id=-1, neighbors=()):
        line_id = int(line_id)
        if line_id == -1:
            line_id = self._new_line_id()
        self._check(not self.exist_line(line_id), "!exist_line(line_id)")
        self.lines_[line_id] = self._line(line)
        self.nl2p_[line_id] = set()
        for point_id in neighbors:
            self.add_edge(point_id, line_id)
        return line_id

    def update_point(self, point_id, p):
        self._check(self.exist_point(point_id), "exist_point(point_id)")
        self.points_[int(point_id)] = self._point(p)

    def update_line(self, line_id, line):
        self._check(self.exist_line(line_id), "exist_line(line_id)")
        self.lines_[int(line_id)] = self._line(line)

    def init_lines(self, lines, ids=None):
        ids = list(range(len(lines))) if ids is None or len(ids) == 0 else [int(i) for i in ids]
        self._check(len(ids) == len(lines), "lines.size() == ids.size()")
        for ln, i in zip(lines, ids):
            self.add_line(ln, i)

    def line(self, line_id):
        self._check(self.exist_line(line_id), "exist_line(line_id)")
        return self.lines_[int(line_id)]

    def get_dict_lines(self):
        return {k: self.lines_[k] for k in sorted(self.lines_)}

    def get_all_lines(self):
        return [self.lines_[k] for k in sorted(self.lines_)]


def _line2d(v):
    from .base import Line2d
    if isinstance(v, Line2d):
        return Line2d(v.start, v.end)
    a = np.array(v, np.float64).reshape(2, 2)
    return Line2d(a[0], a[1])


def _track(cls, v):
    """a copy of a track object, or the track of its dict"""
    if isinstance(v, dict):
        if cls.__name__ == "LineTrack":
            from .base import Line3d, Line2d
            ln = v["line"]
            ln = Line3d(ln["start"], ln["end"]) if isinstance(ln, dict) else Line3d(np.asarray(ln)[0], np.asarray(ln)[1])
            t = cls(ln, v["image_id_list"], v["line_id_list"], [_line2d(x if not isinstance(x, dict) else
                                                                         np.array([x["start"], x["end"]])) for x in v["line2d_list"]])
            for k in ("node_id_list", "score_list"):
                if k in v:
                    setattr(t, k, list(v[k]))
            if "line3d_list" in v:
                t.line3d_list = [Line3d(x["start"], x["end"]) if isinstance(x, dict) else Line3d(np.asarray(x)[0], np.asarray(x)[1])
                                 for x in v["line3d_list"]]
            return t
        if cls.__name__ == "PointTrack":
            return cls(v["p"], v["image_id_list"], v["p2d_id_list"], v["p2d_list"])
        return cls(v)
    return v


class VPLine_Bipartite2d(_Bipartite):
    """structures/vpline_bipartite.h:20-27: VP2d nodes and Line2d nodes"""
    _point = staticmethod(VP2d)
    _line = staticmethod(_line2d)

    def _line_dict(self, v):
        return np.array([v.start, v.end])


class PL_Bipartite3d(_Bipartite):
    """structures/pl_bipartite.h:62-75: PointTrack nodes and LineTrack nodes"""

    @staticmethod
    def _point(v):
        from .base import PointTrack
        return _track(PointTrack, v)

    @staticmethod
    def _line(v):
        from .base import LineTrack
        return _track(LineTrack, v)

    def get_point_cloud(self):
        return [np.asarray(self.points_[k].p, float).copy() for k in sorted(self.points_)]

    def get_line_cloud(self):
        return [self.lines_[k].line for k in sorted(self.lines_)]


class VPLine_Bipartite3d(_Bipartite):
    """structures/vpline_bipartite.h:29-36: VPTrack nodes and LineTrack nodes"""

    @staticmethod
    def _point(v):
        from .vplib import VPTrack
        return VPTrack(v)

    _line = staticmethod(PL_Bipartite3d._line)


def GetAllBipartites_VPLine2d(all_2d_lines, vpresults, vptracks):
    """vpline_bipartite.cc:97-158: per image the 2D lines, the 2D VPs that belong to a 3D track (VP2d with the track's
    index) and an edge from every line with such a VP"""
    if len(all_2d_lines) != len(vpresults):
        raise ValueError("Check failed: all_2d_lines.size() == vpresults.size()")
    m = {int(i): [-1] * r.count_vps() for i, r in vpresults.items()}
    for track_id, t in enumerate(vptracks):
        for img_id, vp2d_id in t.supports:
            m[int(img_id)][int(vp2d_id)] = track_id
    out = {}
    for img_id in sorted(all_2d_lines):
        bpt = VPLine_Bipartite2d()
        lines = all_2d_lines[img_id]
        bpt.init_lines([_line2d(x) for x in lines2d_array(lines).reshape(-1, 2, 2)])
        res = vpresults[img_id]
        for vp2d_id in range(res.count_vps()):
            if m[int(img_id)][vp2d_id] >= 0:
                bpt.add_point(VP2d(res.vps[vp2d_id], m[int(img_id)][vp2d_id]), vp2d_id)
        for line_id in range(bpt.count_lines()):
            if res.HasVP(line_id) and m[int(img_id)][res.GetVPLabel(line_id)] >= 0:
                bpt.add_edge(res.GetVPLabel(line_id), line_id)
        out[int(img_id)] = bpt
    return out
