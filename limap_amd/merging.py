"""Mirror of `limap.merging`: `merging` (MergeToLineTracks, merging/merging.py:6-21, merging/merging.cc:347-511), the
merge of `limap.runners.line_fitnmerge`, with its pair tests on the GPU; and the functions that follow
ComputeLineTracks inside `limap.runners.line_triangulation` (runners/line_triangulation.py:171-200; python wrappers
merging/merging.py:24-100, C++ merging/merging_utils.cc:27-155 and merging/merging.cc:513-644):

    filter_tracks_by_reprojection, remerge, filter_tracks_by_sensitivity, filter_tracks_by_overlap

Same names and argument meaning.  `TrackSet` is the efficient form: it stays bound to the
triangulator's context (cameras already resident) and keeps the tracks in the native container
between steps; the module-level functions take and return LineTrack lists like the reference.
"""
import ctypes as C

import numpy as np

from . import _capi, _native
from .base import Line2d, Line3d, LineTrack


def _linker_cfg(linker3d):
    """dict (cfg["triangulation"]["remerging"]["linker3d"]) or an object exposing the fields."""
    if isinstance(linker3d, dict):
        d = dict(linker3d)
    else:
        conf = getattr(linker3d, "config", linker3d)
        d = {k: getattr(conf, k) for k in _capi.L3_KEYS if hasattr(conf, k)}
    return _capi.config_from_dict({"linker3d_config": d})


def _conf_dict(obj, keys):
    """a linker config as a dict: a dict itself, a LineLinker2d/3d (`.config`) or a config object"""
    if isinstance(obj, dict):
        return dict(obj)
    conf = getattr(obj, "config", obj)
    if isinstance(conf, dict):
        return dict(conf)
    return {k: getattr(conf, k) for k in keys if hasattr(conf, k)}


def _merge_linker_cfg(linker):
    """LineLinker-like (`.linker_2d` / `.linker_3d`) or {"linker2d": ..., "linker3d": ...} (cfg["merging"])."""
    if isinstance(linker, dict):
        d2 = linker.get("linker2d", linker.get("linker2d_config")) or {}
        d3 = linker.get("linker3d", linker.get("linker3d_config")) or {}
    else:
        d2 = getattr(linker, "linker_2d", None)
        d3 = getattr(linker, "linker_3d", None)
        if d2 is None and hasattr(linker, "GetLinker2d"):
            d2, d3 = linker.GetLinker2d(), linker.GetLinker3d()
        d2, d3 = d2 if d2 is not None else {}, d3 if d3 is not None else {}
    return _capi.config_from_dict({"linker2d_config": _conf_dict(d2, _capi.L2_KEYS),
                                   "linker3d_config": _conf_dict(d3, _capi.L3_KEYS)})


def _seg3d_array(x):
    """_GetLine3dVectorFromArray input: (M, 2, 3), (M, 6) or a list of (2, 3) -> (M, 6)"""
    if isinstance(x, (list, tuple)) and len(x) == 0:
        return np.zeros((0, 6))
    a = np.asarray(x, dtype=np.float64)
    if a.size == 0:
        return np.zeros((0, 6))
    if (a.ndim == 3 and a.shape[1:] == (2, 3)) or (a.ndim == 2 and a.shape[1] == 6):
        return np.ascontiguousarray(a.reshape(-1, 6))
    raise ValueError(f"3D segments must be (M, 2, 3) or (M, 6), got shape {a.shape}")


def _merge_inputs(all_2d_segs, imagecols, seg3d_list, neighbors):
    """Arrays of the merge, with the checks of merging/merging.cc:353-368 and the std::map::at lookups made before
    any device work: the image counts of the three inputs, 2D against 3D segments per image, neighbour ids."""
    from .triangulation import _view_arrays
    ids = sorted(int(i) for i in imagecols.get_img_ids())
    if len(all_2d_segs) != len(seg3d_list) or len(all_2d_segs) != len(neighbors):
        raise ValueError(f"merging: {len(all_2d_segs)} images of 2D segments, {len(seg3d_list)} of 3D segments, "
                         f"{len(neighbors)} of neighbours")
    idset = set(ids)
    k = np.zeros((len(ids), 4)); q = np.zeros((len(ids), 4)); t = np.zeros((len(ids), 3))
    seg_off = np.zeros(len(ids) + 1, np.int64)
    segs2, segs3, nb_off, nb = [], [], np.zeros(len(ids) + 1, np.int64), []
    for n, i in enumerate(ids):
        k[n], q[n], t[n] = _view_arrays(imagecols.camview(i))
        s2 = np.asarray(all_2d_segs[i], dtype=np.float64)
        s2 = s2.reshape(0, 4) if s2.size == 0 else s2[:, :4]
        s3 = _seg3d_array(seg3d_list[i])
        if len(s2) != len(s3):
            raise ValueError(f"merging: image {i} has {len(s2)} 2D segments but {len(s3)} 3D segments")
        if i not in neighbors:
            raise IndexError(f"merging: no neighbour list for image {i}")
        ng = [int(j) for j in neighbors[i]]
        for j in ng:
            if j not in idset:
                raise IndexError(f"merging: neighbour {j} of image {i} is not an image")
        segs2.append(s2); segs3.append(s3); nb += ng
        seg_off[n + 1] = seg_off[n] + len(s2)
        nb_off[n + 1] = len(nb)
    cat = lambda L, w: np.ascontiguousarray(np.concatenate(L, 0)) if L else np.zeros((0, w))  # noqa: E731
    return dict(ids=ids, k=k, q=q, t=t, seg_off=seg_off, segs2=cat(segs2, 4), segs3=cat(segs3, 6), nb_off=nb_off,
                nb=np.asarray(nb, np.int32).reshape(-1))


class MergeGraph:
    """The graph MergeToLineTracks builds (base/graph.h): nodes in node order as (image id, line id), undirected
    edges (node_idx1, node_idx2, sim) in insertion order."""

    def __init__(self, node_image_ids, node_line_ids, edge_idx1, edge_idx2, edge_sim):
        self.node_image_ids, self.node_line_ids = node_image_ids, node_line_ids
        self.edge_idx1, self.edge_idx2, self.edge_sim = edge_idx1, edge_idx2, edge_sim

    @classmethod
    def from_ctx(cls, ctx):
        n, e = C.c_int64(), C.c_int64()
        ctx.chk(ctx.L.lt_merge_graph_size(ctx.h, C.byref(n), C.byref(e)))
        N, E = n.value, e.value
        ni, nl = np.zeros(max(N, 1), np.int32), np.zeros(max(N, 1), np.int32)
        e1, e2, sim = np.zeros(max(E, 1), np.int32), np.zeros(max(E, 1), np.int32), np.zeros(max(E, 1))
        p = _capi.ptr
        ctx.chk(ctx.L.lt_merge_graph_get(ctx.h, p(ni, C.c_int32), p(nl, C.c_int32), p(e1, C.c_int32),
                                         p(e2, C.c_int32), p(sim, C.c_double)))
        return cls(ni[:N], nl[:N], e1[:E], e2[:E], sim[:E])

    @property
    def nodes(self):
        return np.stack([self.node_image_ids, self.node_line_ids], 1)

    @property
    def edges(self):
        return np.stack([self.edge_idx1, self.edge_idx2], 1)

    def num_nodes(self):
        return len(self.node_image_ids)

    def num_edges(self):
        return len(self.edge_idx1)


class TrackSet:
    def __init__(self, ctx, handle):
        self.ctx = ctx
        self.L = ctx.L
        self.h = C.c_void_p(handle)

    @classmethod
    def from_triangulator(cls, tri):
        """Tracks of a GlobalLineTriangulator after ComputeLineTracks()."""
        ctx = tri.context()
        return cls(ctx, ctx.L.lt_ts_from_ctx(ctx.h))

    @classmethod
    def from_tracks(cls, ctx, tracks):
        T = len(tracks)
        off = np.zeros(T + 1, np.int64)
        off[1:] = np.cumsum([len(t.image_id_list) for t in tracks])
        M = int(off[-1])
        line7 = np.zeros((max(T, 1), 7)); active = np.ones(max(T, 1), np.uint8)
        img = np.zeros(max(M, 1), np.int32); lid = np.zeros(max(M, 1), np.int32); nid = np.zeros(max(M, 1), np.int32)
        sc = np.zeros(max(M, 1)); l2 = np.zeros((max(M, 1), 4)); l3 = np.zeros((max(M, 1), 10))
        for n, t in enumerate(tracks):
            line7[n, :3], line7[n, 3:6], line7[n, 6] = t.line.start, t.line.end, getattr(t.line, "uncertainty", -1.0)
            active[n] = 1 if getattr(t, "active", True) else 0
            a, b = int(off[n]), int(off[n + 1])
            img[a:b], lid[a:b] = t.image_id_list, t.line_id_list
            if len(t.node_id_list) == b - a:
                nid[a:b] = t.node_id_list
            if len(t.score_list) == b - a:
                sc[a:b] = t.score_list
            for k in range(b - a):
                l2[a + k, :2], l2[a + k, 2:] = t.line2d_list[k].start, t.line2d_list[k].end
                if k < len(t.line3d_list):
                    l = t.line3d_list[k]
                    l3[a + k, :3], l3[a + k, 3:6] = l.start, l.end
                    l3[a + k, 6:8] = getattr(l, "depths", (-1.0, -1.0))
                    l3[a + k, 8], l3[a + k, 9] = getattr(l, "uncertainty", -1.0), getattr(l, "score", -1.0)
        p = _capi.ptr
        h = ctx.L.lt_ts_create(T, p(line7, C.c_double), p(active, C.c_uint8), p(off, C.c_int64), p(img, C.c_int32),
                               p(lid, C.c_int32), p(nid, C.c_int32), p(sc, C.c_double), p(l2, C.c_double),
                               p(l3, C.c_double))
        return cls(ctx, h)

    @classmethod
    def from_merge(cls, linker, all_2d_segs, imagecols, seg3d_list, neighbors, var2d=5.0, device=0):
        """limap.merging.merging into a track set bound to a context with the cameras of `imagecols` (the later
        filter_by_reprojection / remerge run on it without a copy); the graph is in `.graph`, the merge's timers
        (lt_merge_get_timers) in `.merge_timers`."""
        a = _merge_inputs(all_2d_segs, imagecols, seg3d_list, neighbors)
        cfg = _merge_linker_cfg(linker)
        ctx = _capi.Context(device=device)
        ctx.init(a["ids"], a["k"], a["q"], a["t"], a["seg_off"], a["segs2"])
        seg3d_off = a["seg_off"].copy()
        out = C.c_void_p()
        p = _capi.ptr
        ctx.chk(ctx.L.lt_merge_to_tracks(ctx.h, p(seg3d_off, C.c_int64), p(a["segs3"], C.c_double),
                                         p(a["nb_off"], C.c_int64), p(a["nb"], C.c_int32), C.byref(cfg),
                                         float(var2d), C.byref(out)))
        ts = cls(ctx, out.value)
        ts.graph = MergeGraph.from_ctx(ctx)
        tm = ctx.module_timers("lt_merge_get_timers", 4)
        ts.merge_timers = dict(device_ms=float(tm[0]), host_ms=float(tm[1]), attempts=int(tm[2]), edges=int(tm[3]))
        return ts

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.L.lt_ts_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def __len__(self):
        return int(self.L.lt_ts_num_tracks(self.h))

    def filter_by_reprojection(self, th_angular2d, th_perp2d, num_outliers=2):
        self.ctx.chk(self.L.lt_ts_filter_by_reprojection(self.ctx.h, self.h, float(th_angular2d), float(th_perp2d),
                                                         int(num_outliers)))
        return self

    def filter_by_sensitivity(self, th_angular3d, min_num_supports):
        self.ctx.chk(self.L.lt_ts_filter_by_sensitivity(self.ctx.h, self.h, float(th_angular3d), int(min_num_supports)))
        return self

    def filter_by_overlap(self, th_overlap, min_num_supports):
        self.ctx.chk(self.L.lt_ts_filter_by_overlap(self.ctx.h, self.h, float(th_overlap), int(min_num_supports)))
        return self

    def remerge(self, linker3d, num_outliers=2):
        """merging.remerge (merging/merging.py:24-42): repeat until the number of tracks is stable."""
        cfg = _linker_cfg(linker3d)
        n = len(self)
        if n == 0:
            return self
        while True:
            self.ctx.chk(self.L.lt_ts_remerge_once(self.ctx.h, self.h, C.byref(cfg), int(num_outliers)))
            n_new = len(self)
            if n_new == n:
                break
            n = n_new
        return self

    def refine(self, cfg, max_num_iterations=200):
        """Step [E] of the runner (runners/line_triangulation.py:208-219) on the native container, cameras constant:
        every track's line becomes the re-cut segment of its refined infinite line (limap_amd.optimize, DESIGN.md
        section 19).  cfg: cfg["refinement"] or an optimize.HybridBAConfig.  The per-track results (parameters, costs,
        iterations, termination codes) are in `.refine_result` afterwards."""
        import copy
        from . import optimize
        ba = optimize.HybridBAConfig(cfg) if isinstance(cfg, dict) or cfg is None else copy.copy(cfg)
        if not isinstance(ba, optimize.HybridBAConfig):
            raise TypeError("TrackSet.refine: cfg must be a dict or an optimize.HybridBAConfig")
        ba._check()
        ba.max_num_iterations = int(max_num_iterations)
        T = len(self)
        if T == 0:
            self.refine_result = dict(params=np.zeros((0, 6)), segments=np.zeros((0, 6)), cost=np.zeros((0, 2)),
                                      iterations=np.zeros(0, np.int32), codes=np.zeros(0, np.int32))
            return self
        c = ba._struct(ba.num_outliers_aggregator, ba.constant_line)
        self.ctx.chk(self.L.lt_refine_tracks(self.ctx.h, self.h, C.byref(c)))
        P = np.zeros((T, 6)); seg = np.zeros((T, 6)); cost = np.zeros((T, 2))
        it = np.zeros(T, np.int32); code = np.zeros(T, np.int32)
        p = _capi.ptr
        self.ctx.chk(self.L.lt_refine_get(self.ctx.h, p(P, C.c_double), p(seg, C.c_double), p(cost, C.c_double),
                                          p(it, C.c_int32), p(code, C.c_int32)))
        self.refine_result = dict(params=P, segments=seg, cost=cost, iterations=it, codes=code)
        return self

    def arrays(self):
        T = len(self); M = int(self.L.lt_ts_num_members(self.h))
        line = np.zeros((max(T, 1), 7)); active = np.zeros(max(T, 1), np.uint8); off = np.zeros(T + 1, np.int64)
        img = np.zeros(max(M, 1), np.int32); lid = np.zeros(max(M, 1), np.int32); nid = np.zeros(max(M, 1), np.int32)
        sc = np.zeros(max(M, 1)); l2 = np.zeros((max(M, 1), 4)); l3 = np.zeros((max(M, 1), 10))
        p = _capi.ptr
        self.ctx.chk(self.L.lt_ts_get(self.h, p(line, C.c_double), p(active, C.c_uint8), p(off, C.c_int64),
                                      p(img, C.c_int32), p(lid, C.c_int32), p(nid, C.c_int32), p(sc, C.c_double),
                                      p(l2, C.c_double), p(l3, C.c_double)))
        return dict(line=line[:T], active=active[:T], off=off, image_ids=img[:M], line_ids=lid[:M], node_ids=nid[:M],
                    scores=sc[:M], line2d=l2[:M], line3d=l3[:M])

    def tracks(self):
        a = self.arrays()
        out = []
        for n in range(len(a["off"]) - 1):
            sl = slice(int(a["off"][n]), int(a["off"][n + 1]))
            t = LineTrack()
            t.line = Line3d(a["line"][n, :3], a["line"][n, 3:6], -1.0, -1.0, -1.0, a["line"][n, 6])
            t.image_id_list = a["image_ids"][sl].tolist(); t.line_id_list = a["line_ids"][sl].tolist()
            t.node_id_list = a["node_ids"][sl].tolist(); t.score_list = a["scores"][sl].tolist()
            t.line2d_list = [Line2d(s[:2], s[2:]) for s in a["line2d"][sl]]
            t.line3d_list = [Line3d.from10(s) for s in a["line3d"][sl]]
            t.active = bool(a["active"][n])
            out.append(t)
        return out


def track_connect_edges(ctx, line7, active, linker3d, capacity0=0):
    """The edge set of one remerge pass's device part (lt_fn_track_connect, k_track_connect) on plain arrays, for tests:
    line7 (T, 7) = start, end, uncertainty; active (T,).  -> dict(edges (E, 2) int64 as (min, max), sorted and unique;
    n_raw: the device's edge counter; attempts: launches).  capacity0: edge slots of the first launch (0 = default)."""
    line7 = np.ascontiguousarray(np.asarray(line7, np.float64).reshape(-1, 7))
    active = np.ascontiguousarray(np.asarray(active).reshape(-1) != 0, np.uint8)
    if len(active) != len(line7):
        raise ValueError(f"track_connect_edges: {len(line7)} lines, {len(active)} active flags")
    cfg = _linker_cfg(linker3d)
    T = len(line7)
    p = _capi.ptr
    n_unique, n_raw, attempts = C.c_int64(), C.c_int64(), C.c_int32()
    out = np.zeros(max(4 * T, 1), np.uint64)
    for _ in range(2):
        rc = ctx.L.lt_fn_track_connect(ctx.h, T, p(line7, C.c_double), p(active, C.c_uint8), C.byref(cfg), int(capacity0),
                                       p(out, C.c_uint64), len(out), C.byref(n_unique), C.byref(n_raw), C.byref(attempts))
        if rc == 0 or n_unique.value <= len(out):
            break
        out = np.zeros(n_unique.value, np.uint64)  # too small: the call said how many there are
    ctx.chk(rc)
    e = out[:n_unique.value]
    edges = np.stack([(e >> np.uint64(32)).astype(np.int64), (e & np.uint64(0xFFFFFFFF)).astype(np.int64)], 1)
    return dict(edges=edges, n_raw=int(n_raw.value), attempts=int(attempts.value))


# ---- module-level functions with the reference's signatures ------------------------------------
def merging(linker, all_2d_segs, imagecols, seg3d_list, neighbors, var2d=5.0):
    """limap.merging.merging (merging/merging.py:6-21): -> (graph, linetracks)."""
    ts = TrackSet.from_merge(linker, all_2d_segs, imagecols, seg3d_list, neighbors, var2d)
    return ts.graph, ts.tracks()


def _ctx_for(imagecols):
    from .triangulation import _view_arrays
    ids = [int(i) for i in imagecols.get_img_ids()]
    k = np.zeros((len(ids), 4)); q = np.zeros((len(ids), 4)); t = np.zeros((len(ids), 3))
    for n, i in enumerate(ids):
        k[n], q[n], t[n] = _view_arrays(imagecols.camview(i))
    ctx = _capi.Context()
    ctx.init(ids, k, q, t, np.zeros(len(ids) + 1, np.int64), np.zeros((0, 4)))
    return ctx


def filter_tracks_by_reprojection(linetracks, imagecols, th_angular2d, th_perp2d, num_outliers=2):
    ts = TrackSet.from_tracks(_ctx_for(imagecols), linetracks)
    return ts.filter_by_reprojection(th_angular2d, th_perp2d, num_outliers).tracks()


def remerge(linker3d, linetracks, num_outliers=2):
    if len(linetracks) == 0:
        return linetracks
    ctx = _capi.Context()
    ctx.init([0], np.array([[1.0, 1, 0, 0]]), np.array([[1.0, 0, 0, 0]]), np.zeros((1, 3)), np.zeros(2, np.int64),
             np.zeros((0, 4)))
    return TrackSet.from_tracks(ctx, linetracks).remerge(linker3d, num_outliers).tracks()


def filter_tracks_by_sensitivity(linetracks, imagecols, th_angular3d, min_num_supports):
    ts = TrackSet.from_tracks(_ctx_for(imagecols), linetracks)
    return ts.filter_by_sensitivity(th_angular3d, min_num_supports).tracks()


def filter_tracks_by_overlap(linetracks, imagecols, th_overlap, min_num_supports):
    ts = TrackSet.from_tracks(_ctx_for(imagecols), linetracks)
    return ts.filter_by_overlap(th_overlap, min_num_supports).tracks()
