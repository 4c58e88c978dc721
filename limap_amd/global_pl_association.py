"""Mirror of `limap.optimize.global_pl_association` -- the core of limap.runners.pointline_association: the joint
optimisation of point tracks, line tracks and vanishing points under soft association constraints.

    cfg_associator = optimize.GlobalAssociatorConfig(cfg["global_pl_association"])
    associator = optimize.GlobalAssociator(cfg_associator)
    associator.InitImagecols(imagecols); associator.InitPointTracks(pointtracks); associator.InitLineTracks(linetracks)
    associator.Init2DBipartites_PointLine(all_bpt2ds)
    associator.InitVPTracks(vptracks); associator.Init2DBipartites_VPLine(all_bpt2ds_vp)
    associator.SetUp(); associator.Solve()
    bpt3d = associator.GetBipartite3d_PointLine(); bpt3d_vp = associator.GetBipartite3d_VPLine()

Cameras are constant (upstream's default, constant_pose: True): the unknowns are the points (3 each), the lines (4) and
the vanishing points (2), coupled by the association edges.  SetUp restates upstream's switches, weights and edge
construction on the host; Solve runs the HIP kernels of lt_kernels_assoc.hip -- section 27's loop with its linear step by
preconditioned conjugate gradients on the block-sparse matrix -- or, with `host_threads=N`, the documented host path
(lt_fn_assoc_host: bit-identical results), a request, never a fallback.  **Points, lines and vanishing points are a
stationary point of upstream's cost under its weights and losses, not the iterates of a Ceres run.**

Rejected by name with a ValueError before any launch: constant_pose=False, constant_intrinsics=False, non-finite input,
ids missing from the collection, a vanishing point of zero length.  ReassociateJunctions raises NotImplementedError
(upstream's runner has it commented out).  Upstream's yaml key th_pixel_sigma is not read by upstream either: the key is
th_pixel.
"""
import copy
import ctypes as C

import numpy as np

from . import _capi, _native
from .base import Line3d, PointTrack
from .structures import PL_Bipartite3d, VPLine_Bipartite3d
from .vplib import VPTrack
# (limap_amd.optimize ends by importing this module, after the names below exist: either may load first)
from .optimize import HybridBAConfig, RefinementConfig

__all__ = ["GlobalAssociatorConfig", "GlobalAssociator", "solve_global_pl_association", "assoc_arrays"]

PL, VL, ORTH, COLL = 0, 1, 2, 3  # edge_kind of lt_assoc_input
_KERNELS = ("linearize", "diag", "diag_vp", "precond", "cg_begin", "matvec", "alpha", "update", "beta", "dir", "backsub",
            "cost", "decide")


class GlobalAssociatorConfig(HybridBAConfig):
    """optimize/global_pl_association/global_associator.h:19-74 on top of HybridBAConfig.  The four loss functions
    are fixed as upstream's InitConfig() fixes them."""
    _UNSUPPORTED_TRUE = ("use_vp", "use_heatmap", "use_feature", "use_ref_descriptor")
    _GA_KEYS = dict(constant_vp=bool, th_angle_lineline=float, th_count_lineline=int, lw_pointline_association=float,
                    th_pixel=float, th_weight_pointline=float, lw_vpline_association=float, th_count_vpline=int,
                    lw_vp_orthogonality=float, th_angle_orthogonality=float, lw_vp_collinearity=float,
                    th_angle_collinearity=float, th_hard_pl_dist3d=float, th_hard_vpline_angle3d=float)
    point_line_association_3d_loss_function = ("HuberLoss", 0.01)
    vp_line_association_3d_loss_function = ("HuberLoss", 0.01)
    vp_orthogonality_loss_function = ("TrivialLoss",)
    vp_collinearity_loss_function = ("TrivialLoss",)

    def __init__(self, cfg=None):
        self.th_count_lineline, self.th_angle_lineline = 3, 30.0
        self.lw_pointline_association, self.th_pixel, self.th_weight_pointline = 10.0, 2.0, 3.0
        self.lw_vpline_association, self.th_count_vpline = 1.0, 3
        self.lw_vp_orthogonality, self.th_angle_orthogonality = 1.0, 87.0
        self.lw_vp_collinearity, self.th_angle_collinearity = 0.0, 1.0
        self.th_hard_pl_dist3d, self.th_hard_vpline_angle3d = 2.0, 5.0
        self.constant_vp = False
        self.cg_eta, self.cg_max_iterations = 0.1, 500  # Ceres' eta and max_linear_solver_iterations
        super().__init__(cfg)
        self._assign(cfg, dict(self._GA_KEYS, cg_eta=float, cg_max_iterations=int, max_num_iterations=int))

    def _check_assoc(self):
        RefinementConfig._check(self)  # (HybridBAConfig's own check is solve_line_bundle_adjustment's)
        for k in ("constant_intrinsics", "constant_pose"):
            if not getattr(self, k):
                raise ValueError(f"limap_amd.optimize: {k}=False is not built in the global association (the cameras "
                                 "are constant: call set_constant_camera() or set the key)")

    def _assoc_struct(self, enable_pointline, enable_vpline, poll_interval=None, cg_batch=None, kernel_timers=False):
        c = _capi.LtAssocConfig()
        _capi.load_library().lt_assoc_config_default(C.byref(c))
        for k in ("geometric_alpha", "lw_point", "lw_pointline_association", "lw_vpline_association", "lw_vp_orthogonality",
                  "lw_vp_collinearity", "cg_eta"):
            setattr(c, k, float(getattr(self, k)))
        for k in ("cg_max_iterations", "min_num_images", "max_num_iterations", "constant_intrinsics", "constant_pose",
                  "constant_point", "constant_line", "constant_vp"):
            setattr(c, k, int(getattr(self, k)))
        c.enable_pointline, c.enable_vpline = int(bool(enable_pointline)), int(bool(enable_vpline))
        c.poll_interval, c.cg_batch, c.kernel_timers = int(poll_interval or 0), int(cg_batch or 0), int(bool(kernel_timers))
        return c


_context = _capi.per_device_contexts()


def assoc_arrays(cams, points_csr, lines_csr, vps, edges, cfg_struct, host_threads=None, ctx=None):
    """One call of lt_assoc_arrays (device) or lt_fn_assoc_host (host_threads given).  cams = (ids, k, q, t); points_csr =
    (p3, off, img, xy); lines_csr = (line6, off, img, l2d[, l3d]); vps (V, 3); edges = (kind, a, b, w) arrays -> dict:
    points, params (uvec, wvec), vps, cost (initial, final), iterations, cg_iterations, code, timers"""
    ids, k, q, t = cams
    p3, poff, pimg, pxy = points_csr
    line6, loff, limg, l2 = lines_csr[:4]
    f64, p = _capi.f64, _capi.ptr
    vps = f64(np.asarray(vps, float).reshape(-1, 3))
    ek, ea, eb = (np.ascontiguousarray(x, np.int32).reshape(-1) for x in edges[:3])
    ew = f64(np.asarray(edges[3], float).reshape(-1))
    NP, NL, NV, N = len(poff) - 1, len(loff) - 1, len(vps), len(ids)
    keep = [np.ascontiguousarray(ids, np.int32), f64(k), f64(q), f64(t), f64(p3), np.ascontiguousarray(poff, np.int64),
            np.ascontiguousarray(pimg, np.int32), f64(pxy), f64(line6), np.ascontiguousarray(loff, np.int64),
            np.ascontiguousarray(limg, np.int32), f64(l2), vps if NV else np.zeros((1, 3)), ek if len(ek) else np.zeros(1, np.int32),
            ea if len(ea) else np.zeros(1, np.int32), eb if len(eb) else np.zeros(1, np.int32), ew if len(ew) else np.zeros(1)]
    a = _capi.LtAssocInput()
    a.n_img, a.n_pt, a.n_ln, a.n_vp, a.n_edge = N, NP, NL, NV, len(ek)
    a.img_ids, a.kvec4, a.qvec4, a.tvec3 = p(keep[0], C.c_int32), p(keep[1]), p(keep[2]), p(keep[3])
    a.pt3, a.pt_off, a.pt_img, a.pt_xy2 = p(keep[4]), p(keep[5], C.c_int64), p(keep[6], C.c_int32), p(keep[7])
    a.line6, a.ln_off, a.ln_img, a.l2d4 = p(keep[8]), p(keep[9], C.c_int64), p(keep[10], C.c_int32), p(keep[11])
    a.vp3 = p(keep[12])
    a.edge_kind, a.edge_a, a.edge_b, a.edge_w = p(keep[13], C.c_int32), p(keep[14], C.c_int32), p(keep[15], C.c_int32), p(keep[16])
    po = np.zeros((max(NP, 1), 3)); P = np.zeros((max(NL, 1), 6)); vo = np.zeros((max(NV, 1), 3)); cost = np.zeros(2)
    it = np.zeros(1, np.int32); cg = np.zeros(1, np.int64); code = np.zeros(1, np.int32)
    outs = (p(po), p(P), p(vo), p(cost), p(it, C.c_int32), p(cg, C.c_int64), p(code, C.c_int32))
    L = _capi.load_library()
    timers = None
    if host_threads is not None:
        if L.lt_fn_assoc_host(C.byref(a), C.byref(cfg_struct), int(host_threads), *outs, 0, None, None, None) != 0:
            _native.raise_host_error(L, "lt_fn_assoc_host_error", "limap_amd.optimize: ")
    else:
        ctx = ctx if ctx is not None else _context()
        ctx.chk(L.lt_assoc_arrays(ctx.h, C.byref(a), C.byref(cfg_struct)))  # (a refusal raises ValueError)
        ctx.chk(L.lt_assoc_get(ctx.h, *outs))
        tm = ctx.module_timers("lt_assoc_get_timers", 20)
        timers = dict(prepare_ms=float(tm[0]), loop_ms=float(tm[1]), download_ms=float(tm[2]), batches_enqueued=int(tm[3]),
                      kernels_ms={"k_as_" + n: float(tm[4 + i]) for i, n in enumerate(_KERNELS)})
    return dict(points=po[:NP], params=P[:NL], vps=vo[:NV], cost=cost, iterations=int(it[0]), cg_iterations=int(cg[0]),
                code=int(code[0]), timers=timers)


def _as_dict(x):
    return dict(enumerate(x)) if not isinstance(x, dict) else {int(k): v for k, v in x.items()}


def _angle_deg(a, b):
    c = min(abs(float(np.dot(a, b))), 1.0)
    return float(np.degrees(np.arccos(c)))


def _point_line_distance_2d(line, p):
    """InfiniteLine2d(line).point_distance(p)"""
    s, e = np.asarray(line.start, float), np.asarray(line.end, float)
    d = (e - s) / np.linalg.norm(e - s)
    v = np.asarray(p, float) - s
    return abs(d[0] * v[1] - d[1] * v[0])


class GlobalAssociator:
    """optimize/global_pl_association/global_associator.h:76-155"""

    def __init__(self, cfg=None, host_threads=None, poll_interval=None, cg_batch=None, kernel_timers=False):
        self.config_ = cfg if isinstance(cfg, GlobalAssociatorConfig) else GlobalAssociatorConfig(cfg)
        self.host_threads, self._poll, self._batch, self._kt = host_threads, poll_interval, cg_batch, kernel_timers
        self.imagecols_ = None
        self.point_tracks_, self.line_tracks_, self.vp_tracks_ = {}, {}, {}
        self.points_, self.vps_ = {}, {}
        self.enable_pointline_ = self.enable_vpline_ = False
        self.all_bpt2ds_, self.all_bpt2ds_vp_ = {}, {}
        self._problem = self._res = None

    # ---- init ----
    def InitImagecols(self, imagecols):
        self.imagecols_ = imagecols

    def InitPointTracks(self, pointtracks):
        self.point_tracks_ = {k: (v if hasattr(v, "p2d_list") else PointTrack(v)) for k, v in _as_dict(pointtracks).items()}
        self.points_ = {k: np.array(v.p, np.float64).reshape(3) for k, v in self.point_tracks_.items()}

    def InitLineTracks(self, linetracks):
        self.line_tracks_ = _as_dict(linetracks)

    def InitVPTracks(self, vptracks):
        self.vp_tracks_ = {k: VPTrack(v) for k, v in _as_dict(vptracks).items()}
        self.vps_ = {k: v.direction.copy() for k, v in self.vp_tracks_.items()}

    def Init2DBipartites_PointLine(self, all_bpt2ds):
        self.enable_pointline_ = True
        self.all_bpt2ds_ = {int(k): v for k, v in all_bpt2ds.items()}

    def Init2DBipartites_VPLine(self, all_bpt2ds_vp):
        self.enable_vpline_ = True
        self.all_bpt2ds_vp_ = {int(k): v for k, v in all_bpt2ds_vp.items()}

    def ReassociateJunctions(self):
        raise NotImplementedError("limap_amd.optimize: ReassociateJunctions is not built (upstream's runner does not call it)")

    # ---- the soft associations (global_associator.cc:319-504): host work shared by both solve paths ----
    def construct_weights_pointline(self, th_weight):
        """{(point3d_id, line3d_id): weight}: the count of supports whose keypoint lies within th_pixel of the infinite
        2D line, kept when >= th_weight; in upstream's map order"""
        counts = {}
        for line3d_id in sorted(self.line_tracks_):
            track = self.line_tracks_[line3d_id]
            for img_id, line2d_id in zip(track.image_id_list, track.line_id_list):
                bpt = self._bpt(self.all_bpt2ds_, img_id)
                for point2d_id in bpt.neighbor_points(line2d_id):
                    pt = bpt.point(point2d_id)
                    if pt.point3D_id < 0:
                        continue
                    dist = _point_line_distance_2d(bpt.line(line2d_id), pt.p)
                    key = (int(pt.point3D_id), int(line3d_id))
                    counts[key] = counts.get(key, 0.0) + (1.0 if dist <= self.config_.th_pixel else 0.0)
        return {k: counts[k] for k in sorted(counts) if not counts[k] < th_weight}

    def construct_weights_vpline(self, th_count):
        """{(vp3d_id, line3d_id): count}: the best VP per line by count, ties to the smaller VP id"""
        out = {}
        for line3d_id in sorted(self.line_tracks_):
            track = self.line_tracks_[line3d_id]
            counter = {}
            for img_id, line2d_id in zip(track.image_id_list, track.line_id_list):
                bpt = self._bpt(self.all_bpt2ds_vp_, img_id)
                ids = bpt.neighbor_points(line2d_id)
                if not ids:
                    continue
                if len(ids) != 1:
                    raise ValueError("Check failed: vp2d_ids.size() == 1")
                vp3d_id = bpt.point(ids[0]).point3D_id
                if vp3d_id < 0:
                    continue
                counter[int(vp3d_id)] = counter.get(int(vp3d_id), 0) + 1
            best, best_count = -1, 0
            for vp3d_id in sorted(counter):
                if counter[vp3d_id] > best_count:
                    best, best_count = vp3d_id, counter[vp3d_id]
            if counter and not best_count < th_count:
                out[(best, int(line3d_id))] = best_count
        return {k: out[k] for k in sorted(out)}

    def _vp_pairs(self, keep):
        ids = sorted(self.vps_)
        return [(a, b) for i, a in enumerate(ids) for b in ids[i + 1:] if keep(_angle_deg(self.vps_[a], self.vps_[b]))]

    def construct_pairs_vp_orthogonality(self, th_angle_orthogonality):
        """pairs at least th_angle apart; zero VPs give no pairs (upstream's n_vps - 1 wraps around in size_t)"""
        return self._vp_pairs(lambda ang: not ang < th_angle_orthogonality)

    def construct_pairs_vp_collinearity(self, th_angle_collinearity):
        return self._vp_pairs(lambda ang: not ang > th_angle_collinearity)

    @staticmethod
    def _bpt(table, img_id):
        if int(img_id) not in table:
            raise ValueError(f"limap_amd.optimize: image id {int(img_id)} is not in the 2D bipartites")
        return table[int(img_id)]

    # ---- set-up and solve ----
    def SetUp(self):
        """global_associator.cc:176-220.  The switches that decide which residuals exist are applied by the native plan
        (lt_assoc_config): every edge upstream's construct_* would hand to an Add*Residuals goes in"""
        from .optimize import _camera_arrays, _point_arrays, _track_arrays
        cfg = self.config_
        cfg._check_assoc()
        if self.imagecols_ is None:
            raise ValueError("limap_amd.optimize: InitImagecols was not called")
        pk, lk, vk = sorted(self.point_tracks_), sorted(self.line_tracks_), sorted(self.vp_tracks_)
        pi, li, vi = ({k: n for n, k in enumerate(ks)} for ks in (pk, lk, vk))
        for k in vk:
            v = self.vps_[k]
            if not np.all(np.isfinite(v)):
                raise ValueError(f"limap_amd.optimize: vanishing point {k} is not finite")
            if not np.linalg.norm(v) > 0:
                raise ValueError(f"limap_amd.optimize: vanishing point {k} has zero length")
        edges = []
        if self.enable_pointline_:
            for (p3, l3), w in self.construct_weights_pointline(cfg.th_weight_pointline).items():
                if p3 not in pi:
                    raise ValueError(f"limap_amd.optimize: point3D id {p3} of a 2D bipartite is not in the point tracks")
                edges.append((PL, pi[p3], li[l3], w))
        if self.enable_vpline_:
            for (v3, l3), w in self.construct_weights_vpline(cfg.th_count_vpline).items():
                if v3 not in vi:
                    raise ValueError(f"limap_amd.optimize: VP track id {v3} of a 2D bipartite is not in the VP tracks")
                edges.append((VL, vi[v3], li[l3], w))
            edges += [(ORTH, vi[a], vi[b], 1.0) for a, b in self.construct_pairs_vp_orthogonality(cfg.th_angle_orthogonality)]
            edges += [(COLL, vi[a], vi[b], 1.0) for a, b in self.construct_pairs_vp_collinearity(cfg.th_angle_collinearity)]
        e = np.array(edges, float).reshape(-1, 4)
        ids = [int(i) for i in self.imagecols_.get_img_ids()]
        cams = _camera_arrays({i: self.imagecols_.camview(i) for i in ids})
        self._keys = (pk, lk, vk)
        self._csr = _track_arrays([self.line_tracks_[k] for k in lk])
        vps = np.array([self.vps_[k] for k in vk], float).reshape(-1, 3)
        self._problem = (cams, _point_arrays([self.point_tracks_[k] for k in pk]), self._csr, vps,
                         (e[:, 0].astype(np.int32), e[:, 1].astype(np.int32), e[:, 2].astype(np.int32), e[:, 3].copy()))
        self._cfg_struct = cfg._assoc_struct(self.enable_pointline_, self.enable_vpline_, self._poll, self._batch, self._kt)
        self._res = None

    def Solve(self):
        """False without a residual block (termination 7), as upstream's Solve()"""
        if self._problem is None:
            raise ValueError("limap_amd.optimize: SetUp was not called")
        self._res = assoc_arrays(*self._problem, self._cfg_struct, self.host_threads)
        pk, lk, vk = self._keys
        if self._res["code"] == 7:
            return False
        self.points_ = {k: self._res["points"][n].copy() for n, k in enumerate(pk)}
        self.vps_ = {k: self._res["vps"][n].copy() for n, k in enumerate(vk)}
        return True

    def result(self):
        """the arrays of the solve: points, params, vps, cost (initial, final), iterations, cg_iterations, code, timers"""
        return self._res

    # ---- output ----
    def GetOutputImagecols(self):
        return copy.copy(self.imagecols_)  # the cameras are constants of this problem

    def GetOutputPoints(self):
        return {k: np.asarray(self.points_[k], float).copy() for k in sorted(self.points_)}

    def GetOutputPointTracks(self):
        return {k: PointTrack(self.points_[k], t.image_id_list, t.p2d_id_list, t.p2d_list)
                for k, t in sorted(self.point_tracks_.items())}

    def _segment(self, n, num_outliers):
        from .optimize import cut_segment
        off, l3 = self._csr[1], self._csr[4]
        return cut_segment(self._res["params"][n], l3[off[n]:off[n + 1]], num_outliers)

    def GetOutputLineTracks(self, num_outliers=2):
        from .optimize import _copy_track
        if self._res is None or self._res["code"] == 7:
            return {k: _copy_track(t, t.line) for k, t in sorted(self.line_tracks_.items())}
        out = {}
        for n, k in enumerate(self._keys[1]):
            seg = self._segment(n, int(num_outliers))
            out[k] = _copy_track(self.line_tracks_[k], Line3d(seg[:3], seg[3:]))
        return out

    def GetOutputVPs(self):
        return {k: np.asarray(self.vps_[k], float).copy() for k in sorted(self.vp_tracks_)}

    def GetOutputVPTracks(self):
        return {k: VPTrack(self.vps_[k], t.supports) for k, t in sorted(self.vp_tracks_.items())}

    def test_linetrack_validity(self, track):
        """at least half of the track's images hold a support the default 2D linker connects to the line's projection"""
        L, p = _capi.load_library(), _capi.ptr
        valid = set()
        for img_id, l2d in zip(track.image_id_list, track.line2d_list):
            v = self.imagecols_.camview(int(img_id))
            K, R, T = v.K(), v.R(), v.T()
            ends = []
            for X in (track.line.start, track.line.end):
                x = K @ (R @ np.asarray(X, float) + T)
                ends.append(x[:2] / x[2])
            a = np.ascontiguousarray(np.concatenate(ends))
            b = np.ascontiguousarray(np.concatenate([l2d.start, l2d.end]).astype(float))
            if L.lt_fn_assoc_link2d(p(a), p(b)):
                valid.add(int(img_id))
        return not len(valid) < 0.5 * track.count_images()

    def _lines_for_output(self, bpt):
        for k, t in self.GetOutputLineTracks(self.config_.num_outliers_aggregator).items():
            if not (np.all(np.isfinite(t.line.as_array())) and self.test_linetrack_validity(t)):
                t.line = self.line_tracks_[k].line
            bpt.add_line(t, k)

    def GetBipartite3d_PointLine_Constraints(self):
        bpt = PL_Bipartite3d()
        for k, t in self.GetOutputPointTracks().items():
            bpt.add_point(t, k)
        self._lines_for_output(bpt)
        for (p3, l3) in self.construct_weights_pointline(self.config_.th_weight_pointline):
            if bpt.exist_point(p3) and bpt.exist_line(l3):
                bpt.add_edge(p3, l3)
        return bpt

    def GetBipartite3d_PointLine(self):
        """with the hard gate: the 3D distance at most th_hard_pl_dist3d times the point's depth-based uncertainty"""
        bpt = PL_Bipartite3d()
        for k, t in self.GetOutputPointTracks().items():
            bpt.add_point(t, k)
        self._lines_for_output(bpt)
        unc = {}
        for k, t in self.point_tracks_.items():
            best = np.finfo(float).max
            for img_id in t.image_id_list:  # the input track's point, as upstream reads it
                v = self.imagecols_.camview(int(img_id))
                depth = float((v.R() @ np.asarray(t.p, float) + v.T())[2])
                kv = v.K()
                best = min(best, 1.0 * depth / ((kv[0, 0] + kv[1, 1]) / 2.0))
            unc[k] = best
        for (p3, l3) in self.construct_weights_pointline(self.config_.th_weight_pointline):
            if not (bpt.exist_point(p3) and bpt.exist_line(l3)):
                continue
            ln, pt = bpt.line(l3).line, np.asarray(bpt.point(p3).p, float)
            d = np.asarray(ln.direction(), float)
            v = pt - np.asarray(ln.start, float)
            dist = float(np.linalg.norm(v - d * float(v @ d)))
            if dist > self.config_.th_hard_pl_dist3d * unc[p3]:
                continue
            bpt.add_edge(p3, l3)
        return bpt

    def GetBipartite3d_VPLine(self):
        bpt = VPLine_Bipartite3d()
        for k, t in self.GetOutputVPTracks().items():
            bpt.add_point(t, k)
        self._lines_for_output(bpt)
        for (v3, l3) in self.construct_weights_vpline(self.config_.th_count_vpline):
            if not (bpt.exist_point(v3) and bpt.exist_line(l3)):
                continue
            if _angle_deg(bpt.point(v3).direction, np.asarray(bpt.line(l3).line.direction(), float)) > self.config_.th_hard_vpline_angle3d:
                continue
            bpt.add_edge(v3, l3)
        for v3 in bpt.get_point_ids():
            if bpt.pdegree(v3) == 0:
                bpt.delete_point(v3)
        return bpt


def solve_global_pl_association(cfg, imagecols, bpt3d, all_bpt2ds, host_threads=None):
    """optimize/global_pl_association/solve.py: the point-line association of a 3D bipartite's tracks under the 2D
    bipartites -> the associated PL_Bipartite3d"""
    associator = GlobalAssociator(cfg if isinstance(cfg, GlobalAssociatorConfig) else GlobalAssociatorConfig(cfg), host_threads)
    associator.InitImagecols(imagecols)
    associator.InitPointTracks(bpt3d.get_dict_points())
    associator.InitLineTracks({k: bpt3d.line(k) for k in bpt3d.get_line_ids()})
    associator.Init2DBipartites_PointLine(all_bpt2ds)
    associator.SetUp()
    associator.Solve()
    return associator.GetBipartite3d_PointLine()


def _export():
    """limap.optimize carries these names: add them to limap_amd.optimize, whichever of the two modules loads first"""
    from . import optimize
    for name in __all__:
        setattr(optimize, name, globals()[name])
        if name not in optimize.__all__:
            optimize.__all__.append(name)


_export()
