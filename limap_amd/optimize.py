"""Mirror of the part of `limap.optimize` that `limap.runners.line_triangulation` runs as its step [E]
(runners/line_triangulation.py:208-219): the geometric refinement of line tracks with constant cameras.

    cfg_ba = optimize.HybridBAConfig(cfg["refinement"]); cfg_ba.set_constant_camera()
    ba_engine = optimize.solve_line_bundle_adjustment(cfg_ba, imagecols, linetracks, max_num_iterations=200)
    linetracks_map = ba_engine.GetOutputLineTracks(num_outliers=cfg["refinement"]["num_outliers_aggregator"])

and, per track, `solve_line_refinement` / `line_refinement` (optimize/line_refinement) with their geometric terms.  With
constant intrinsics and poses every track is its own 4-degree-of-freedom problem; all of them run in one launch of the
HIP kernels of lt_kernels_refine.hip.  limap's cost, parameterisation, weights, residual order and
segment cut are restated; **the minimiser is this project's deterministic Levenberg-Marquardt definition: refined lines
are minimisers of upstream's cost, not the iterates of a particular Ceres run.**

Not built, and rejected with a ValueError that names the key: constant_intrinsics=False, constant_pose=False, point
tracks, use_vp, use_heatmap, use_feature.

`host_threads=N` on the solve functions runs the documented host path (lt_fn_refine_host: the same inline functions in
plain C++, bit-identical results) on N OpenMP threads instead of the device; it is a request, never a fallback -- without
it a missing device is an error.
"""
import copy
import ctypes as C

import numpy as np

from . import _capi
from .base import Line3d, LineTrack

__all__ = ["HybridBAConfig", "RefinementConfig", "HybridBAEngine", "RefinementEngine", "solve_line_bundle_adjustment",
           "solve_line_refinement", "line_refinement", "TERMINATION"]

TERMINATION = {0: "max_num_iterations", 1: "radius", 2: "zero_gradient", 3: "pivot", 4: "model_decrease", 5: "constant"}
_UNSUPPORTED_TRUE = ("use_vp", "use_heatmap", "use_feature")


class RefinementConfig:
    """optimize/line_refinement/refinement_config.h:18-90 -- the keys the geometric terms read (ASSIGN_PYDICT_ITEM: a
    present key overrides, unknown keys are ignored)."""
    _KEYS = dict(use_geometric=bool, min_num_images=int, num_outliers_aggregate=int, geometric_alpha=float,
                 print_summary=bool)

    def __init__(self, cfg=None):
        self.use_geometric, self.min_num_images, self.num_outliers_aggregate = True, 4, 2
        self.geometric_alpha, self.print_summary = 10.0, True
        self.max_num_iterations = 100  # solver_options.max_num_iterations
        # not keys of upstream's C++ configuration: the python callers read them from the same dict
        self.num_outliers_aggregator = 2
        self.use_vp = self.use_heatmap = self.use_feature = False
        self._assign(cfg, dict(self._KEYS, num_outliers_aggregator=int, use_vp=bool, use_heatmap=bool, use_feature=bool))

    def _assign(self, cfg, keys):
        if cfg is None:
            return
        if not isinstance(cfg, dict):
            raise TypeError("the configuration must be a dict")
        for k, typ in keys.items():
            if k in cfg and cfg[k] is not None:
                setattr(self, k, typ(cfg[k]))

    def _check(self):
        for k in _UNSUPPORTED_TRUE:
            if getattr(self, k):
                raise ValueError(f"limap_amd.optimize: {k}=True is not built (geometric terms only)")
        if not self.use_geometric:
            raise ValueError("limap_amd.optimize: use_geometric=False leaves no residual (geometric terms only)")

    def _struct(self, num_outliers, constant_line=False):
        c = _capi.LtRefineConfig()
        _capi.load_library().lt_refine_config_default(C.byref(c))
        c.geometric_alpha, c.min_num_images = float(self.geometric_alpha), int(self.min_num_images)
        c.num_outliers_aggregator, c.num_outliers_aggregate = int(num_outliers), int(self.num_outliers_aggregate)
        c.max_num_iterations, c.constant_line = int(self.max_num_iterations), int(bool(constant_line))
        return c


class HybridBAConfig(RefinementConfig):
    """optimize/hybrid_bundle_adjustment/hybrid_bundle_adjustment_config.h:17-49"""
    _BA_KEYS = dict(constant_intrinsics=bool, constant_principal_point=bool, constant_pose=bool, constant_point=bool,
                    constant_line=bool, lw_point=float)

    def __init__(self, cfg=None):
        self.constant_intrinsics, self.constant_principal_point, self.constant_pose = False, True, False
        self.constant_point, self.constant_line, self.lw_point = False, False, 0.1
        super().__init__(cfg)
        self._assign(cfg, self._BA_KEYS)

    def set_constant_camera(self):
        self.constant_intrinsics = True
        self.constant_pose = True

    def _check(self):
        super()._check()
        for k in ("constant_intrinsics", "constant_pose"):
            if not getattr(self, k):
                raise ValueError(f"limap_amd.optimize: {k}=False is not built (cameras are constant: call "
                                 "set_constant_camera() or set the key)")


def _track_arrays(tracks):
    T = len(tracks)
    off = np.zeros(T + 1, np.int64)
    off[1:] = np.cumsum([len(t.image_id_list) for t in tracks])
    M = int(off[-1])
    line6 = np.zeros((max(T, 1), 6)); img = np.zeros(max(M, 1), np.int32)
    l2 = np.zeros((max(M, 1), 4)); l3 = np.zeros((max(M, 1), 6))
    for n, t in enumerate(tracks):
        a, b = int(off[n]), int(off[n + 1])
        if len(t.line2d_list) != b - a or len(t.line3d_list) != b - a:
            raise ValueError(f"track {n}: {b - a} image ids, {len(t.line2d_list)} 2D lines, {len(t.line3d_list)} 3D lines")
        line6[n, :3], line6[n, 3:] = t.line.start, t.line.end
        img[a:b] = t.image_id_list
        for k in range(b - a):
            l2[a + k, :2], l2[a + k, 2:] = t.line2d_list[k].start, t.line2d_list[k].end
            l3[a + k, :3], l3[a + k, 3:] = t.line3d_list[k].start, t.line3d_list[k].end
    return line6, off, img, l2, l3


def _camera_arrays(views):
    """{img_id: view} -> ids, k, q, t"""
    from .triangulation import _view_arrays
    ids = np.array(sorted(views), np.int32)
    k = np.zeros((max(len(ids), 1), 4)); q = np.zeros((max(len(ids), 1), 4)); t = np.zeros((max(len(ids), 1), 3))
    for n, i in enumerate(ids):
        k[n], q[n], t[n] = _view_arrays(views[int(i)])
    return ids, k, q, t


_context = _capi.per_device_contexts()  # lt_create once per device, buffers reused between calls


def cut_segment(params6, line3d6, num_outliers):
    """GetLineSegmentFromInfiniteLine3d alone: the segment of solved parameters for another num_outliers"""
    l3 = np.ascontiguousarray(line3d6, np.float64)
    pp = np.ascontiguousarray(params6, np.float64)
    seg = np.zeros(6)
    p = _capi.ptr
    if _capi.load_library().lt_fn_refine_cut(len(l3), p(l3, C.c_double), p(pp, C.c_double), int(num_outliers),
                                             p(seg, C.c_double)) != 0:
        raise ValueError(f"limap_amd.optimize: num_outliers {num_outliers} leaves the {2 * len(l3)} values of the track")
    return seg


def refine_arrays(cams, tracks_csr, cfg_struct, host_threads=None, ctx=None):
    """One call of lt_refine_arrays (device) or lt_fn_refine_host (host_threads given) -> dict of per-track results."""
    ids, k, q, t = cams
    line6, off, img, l2, l3 = tracks_csr
    T = len(off) - 1
    L = _capi.load_library()
    p = _capi.ptr
    P = np.zeros((max(T, 1), 6)); seg = np.zeros((max(T, 1), 6)); cost = np.zeros((max(T, 1), 2))
    it = np.zeros(max(T, 1), np.int32); code = np.zeros(max(T, 1), np.int32)
    args = (len(ids), p(ids, C.c_int32), p(k, C.c_double), p(q, C.c_double), p(t, C.c_double), T, p(line6, C.c_double),
            p(off, C.c_int64), p(img, C.c_int32), p(l2, C.c_double), p(l3, C.c_double), C.byref(cfg_struct))
    outs = (p(P, C.c_double), p(seg, C.c_double), p(cost, C.c_double), p(it, C.c_int32), p(code, C.c_int32))
    timers = None
    if host_threads is not None:
        if L.lt_fn_refine_host(*args, int(host_threads), *outs) != 0:
            raise ValueError("limap_amd.optimize: " + L.lt_fn_refine_host_error().decode(errors="replace"))
    else:
        ctx = ctx if ctx is not None else _context()
        ctx.chk(L.lt_refine_arrays(ctx.h, *args))
        ctx.chk(L.lt_refine_get(ctx.h, *outs))
        tm = np.zeros(4)
        ctx.chk(L.lt_refine_get_timers(ctx.h, p(tm, C.c_double)))
        timers = dict(prepare_ms=float(tm[0]), kernels_ms=float(tm[1]), download_ms=float(tm[2]), lm_device_ms=float(tm[3]))
    return dict(params=P[:T], segments=seg[:T], cost=cost[:T], iterations=it[:T], codes=code[:T], timers=timers)


def _copy_track(t, line):
    n = LineTrack(line, t.image_id_list, t.line_id_list, t.line2d_list)
    n.node_id_list, n.line3d_list, n.score_list = list(t.node_id_list), list(t.line3d_list), list(t.score_list)
    n.active = getattr(t, "active", True)
    return n


class HybridBAEngine:
    """HybridBAEngine restricted to line tracks with constant cameras.  The solve runs once, with the configuration's
    num_outliers_aggregator; GetOutputLineTracks with another num_outliers re-cuts the segments from the stored
    parameters (cut_segment), it does not solve again."""

    def __init__(self, cfg, imagecols, linetracks, host_threads=None):
        self.config, self.host_threads = cfg, host_threads
        self._tracks = dict(enumerate(linetracks)) if not isinstance(linetracks, dict) else dict(linetracks)
        self._keys = sorted(self._tracks)
        self._cams = _camera_arrays({int(i): imagecols.camview(int(i)) for i in imagecols.get_img_ids()})
        self._csr = _track_arrays([self._tracks[k] for k in self._keys])
        self._n_out = int(cfg.num_outliers_aggregator)
        c = cfg._struct(self._n_out, getattr(cfg, "constant_line", False))
        self._res = refine_arrays(self._cams, self._csr, c, host_threads)
        self._segs = {self._n_out: self._res["segments"]}

    def _segments(self, num_outliers):
        if num_outliers not in self._segs:
            off, l3 = self._csr[1], self._csr[4]
            self._segs[num_outliers] = np.array([cut_segment(self._res["params"][n], l3[off[n]:off[n + 1]], num_outliers)
                                                 for n in range(len(self._keys))]).reshape(-1, 6)
        return self._segs[num_outliers]

    def result(self, num_outliers=None):
        """per-track arrays: params (uvec, wvec), segments, cost (initial, final), iterations, codes (TERMINATION)"""
        n_out = self._n_out if num_outliers is None else int(num_outliers)
        return dict(self._res, segments=self._segments(n_out))

    def GetOutputLineTracks(self, num_outliers=2):
        seg = self._segments(int(num_outliers))
        return {k: _copy_track(self._tracks[k], Line3d(seg[n, :3], seg[n, 3:])) for n, k in enumerate(self._keys)}

    def GetOutputLines(self, num_outliers=2):
        return {k: t.line for k, t in self.GetOutputLineTracks(num_outliers).items()}


def solve_line_bundle_adjustment(cfg, imagecols, linetracks, max_num_iterations=100, host_threads=None):
    """optimize/hybrid_bundle_adjustment/solve.py:31-39"""
    ba = HybridBAConfig(cfg) if isinstance(cfg, dict) or cfg is None else cfg
    if not isinstance(ba, HybridBAConfig):
        raise TypeError("cfg must be a dict or a HybridBAConfig")
    ba._check()
    ba = copy.copy(ba)  # the caller's configuration is not changed
    ba.max_num_iterations = int(max_num_iterations)
    if len(linetracks) == 0:
        raise ValueError("limap_amd.optimize: no line tracks")
    return HybridBAEngine(ba, imagecols, linetracks, host_threads)


class RefinementEngine:
    def __init__(self, result):
        self._r = result

    def GetLine3d(self):
        s = self._r["segments"][0]
        return Line3d(s[:3], s[3:])

    def result(self):
        return self._r


def _refinement_cfg(cfg, kw):
    for k in ("p_vpresults", "p_heatmaps", "p_patches", "p_features"):
        if kw.get(k) is not None:
            raise ValueError(f"limap_amd.optimize: {k} is not built (geometric terms only)")
    rf = RefinementConfig(cfg) if isinstance(cfg, dict) or cfg is None else cfg
    rf._check()
    return rf


def solve_line_refinement(cfg, track, p_camviews, host_threads=None, **kw):
    """optimize/line_refinement/solve.py:4-48: p_camviews are the views of track.GetSortedImageIds(), in that order.
    None below min_num_images."""
    rf = _refinement_cfg(cfg, kw)
    if track.count_images() < rf.min_num_images:
        return None
    ids = track.GetSortedImageIds()
    if len(p_camviews) != len(ids):
        raise ValueError(f"{len(ids)} images support the track, {len(p_camviews)} views given")
    cams = _camera_arrays(dict(zip(ids, p_camviews)))
    r = refine_arrays(cams, _track_arrays([track]), rf._struct(rf.num_outliers_aggregate), host_threads)
    return RefinementEngine(r)


def line_refinement(cfg, tracks, imagecols, heatmap_dir=None, patch_dir=None, featuremap_dir=None, vpresults=None,
                    n_visible_views=4, host_threads=None):
    """optimize/line_refinement/line_refinement.py:15-136 with the geometric terms: the tracks seen in at least
    n_visible_views images and min_num_images images are refined -- all of them in one call -- the others pass through."""
    rf = _refinement_cfg(cfg, {})
    sel = [n for n, t in enumerate(tracks) if t.count_images() >= max(int(n_visible_views), rf.min_num_images)]
    out = list(tracks)
    if sel:
        cams = _camera_arrays({int(i): imagecols.camview(int(i)) for i in imagecols.get_img_ids()})
        r = refine_arrays(cams, _track_arrays([tracks[n] for n in sel]), rf._struct(rf.num_outliers_aggregate), host_threads)
        for m, n in enumerate(sel):
            out[n] = _copy_track(tracks[n], Line3d(r["segments"][m, :3], r["segments"][m, 3:]))
    return out
