"""Mirror of the part of `limap.optimize` that `limap.runners.line_triangulation` runs as its step [E]
(runners/line_triangulation.py:208-219): the geometric refinement of line tracks with constant cameras.

    cfg_ba = optimize.HybridBAConfig(cfg["refinement"]); cfg_ba.set_constant_camera()
    ba_engine = optimize.solve_line_bundle_adjustment(cfg_ba, imagecols, linetracks, max_num_iterations=200)
    linetracks_map = ba_engine.GetOutputLineTracks(num_outliers=cfg["refinement"]["num_outliers_aggregator"])

and, per track, `solve_line_refinement` / `line_refinement` (optimize/line_refinement) with their geometric, VP,
heatmap and feature-consistency terms -- what limap.runners.refinement calls (cfgs/refinement/default.yaml):

    vpresults = vplib.get_vp_detector(cfg["vpdet"]).detect_vp_all_images(all_2d_lines, camviews)
    tracks = optimize.line_refinement(cfg["refinement"], tracks, imagecols, heatmap_dir, patch_dir, featuremap_dir,
                                      vpresults=vpresults)

With constant intrinsics and poses every track is its own 4-degree-of-freedom problem; all of them run in one launch of
the HIP kernels of lt_kernels_refine.hip.  The heatmaps (`heatmap_{img_id}.npy` in heatmap_dir,
or `heatmaps={img_id: array}`) are loaded once, rounded to `dtype` ("float16", upstream's default, or "float32") by
numpy's astype, uploaded once and sampled by the kernel.  The feature term (use_feature) reads
the line patches of limap_amd.features (`patch_dir` with track{t}/track{t}_img{i}.npy, or `patches={(t, img_id):
PatchInfo}`, also those `extract_track_patches(..., device_out=True)` left on the device) or whole feature maps
(`featuremap_dir` with feature_{img_id}.npy stored (C, H, W), or `featuremaps={img_id: (H, W, 128) array or GPU tensor}`);
tracks with patches go to the device in groups of at most `patch_bytes` (FEATURE_PATCH_BYTES) of texels.  limap's cost, parameterisation, weights, residual order and
segment cut are restated; **the minimiser is this project's deterministic Levenberg-Marquardt definition: refined lines
are minimisers of upstream's cost, not the iterates of a particular Ceres run.**

The bundle adjustment with free poses and point tracks -- the call of
runners/hypersim/refine_sfm.py --

    cfg_ba = optimize.HybridBAConfig(cfg["refinement"]); cfg_ba.constant_intrinsics = True
    ba_engine = optimize.solve_hybrid_bundle_adjustment(cfg_ba, imagecols, pointtracks, linetracks)
    new_imagecols = ba_engine.GetOutputImagecols()

is reached only through `solve_point_bundle_adjustment` and `solve_hybrid_bundle_adjustment`, which validate with a check
of their own (HybridBAConfig._check_ba); line-only free-pose bundle adjustment is
`solve_hybrid_bundle_adjustment(cfg, imagecols, {}, linetracks)`.  `solve_line_bundle_adjustment` and
`HybridBAConfig._check()` keep rejecting constant_pose=False.  With constant_pose=True and line tracks only the two new
entry points return what `solve_line_bundle_adjustment` returns, bit for bit (they delegate to it).  **Poses, points and
lines are a stationary point of upstream's cost under upstream's parameterisation, weights and losses, reached from the
input; they are not the iterates of a Ceres run.  Upstream does not fix the gauge, so compare costs and reprojections,
never parameters.**  At most BA_MAX_IMAGES (LT_BA_MAX_IMAGES) images may carry residuals.

With constant_pose=True the problem separates per track: the line tracks go through the line refinement above, every
point track is its own 3-unknown problem under the same loop (its own radius; section 19's termination codes), so every
point equals its own one-point solve.

Not built, and rejected with a ValueError that names the key: constant_intrinsics=False, constant_pose=False and point
tracks on solve_line_bundle_adjustment, use_ref_descriptor, channels other than 128; use_vp, use_heatmap and use_feature
on the hybrid bundle adjustment (the first two are no terms of it upstream either).  A track whose cost cannot be
evaluated at its initial line (a sample line parallel to the projection) ends with TERMINATION 6 and keeps its line,
re-cut.

`host_threads=N` on the solve functions runs the documented host path (lt_fn_refine_host: the same inline functions in
plain C++, bit-identical results) on N OpenMP threads instead of the device; it is a request, never a fallback -- without
it a missing device is an error.
"""
import copy
import ctypes as C

import numpy as np

from . import _capi, _native
from .base import CameraView, ImageCollection, Line3d, LineTrack, PointTrack

__all__ = ["HybridBAConfig", "RefinementConfig", "HybridBAEngine", "RefinementEngine", "Heatmaps",
           "solve_line_bundle_adjustment", "solve_line_refinement", "line_refinement", "TERMINATION", "FeatureMaps",
           "FEATURE_PATCH_BYTES", "solve_point_bundle_adjustment", "solve_hybrid_bundle_adjustment", "BA_MAX_IMAGES"]

TERMINATION = {0: "max_num_iterations", 1: "radius", 2: "zero_gradient", 3: "pivot", 4: "model_decrease", 5: "constant",
               6: "evaluation_failed", 7: "no_residuals"}
BA_MAX_IMAGES = 128  # LT_BA_MAX_IMAGES of include/limap_amd.h: images that may carry residuals in one bundle adjustment
FEATURE_PATCH_BYTES = 512 << 20  # default budget of the feature term for the patch texels of one native call
_TEXELS = {"float16": (np.float16, _capi.TEXEL_F16), "float32": (np.float32, _capi.TEXEL_F32)}


class RefinementConfig:
    """optimize/line_refinement/refinement_config.h:18-90 -- the keys the geometric, VP, heatmap and feature terms
    read (ASSIGN_PYDICT_ITEM: a present key overrides, unknown keys are ignored).  use_ref_descriptor=False and
    ref_multiplier are accepted and not read."""
    _KEYS = dict(use_geometric=bool, min_num_images=int, num_outliers_aggregate=int, geometric_alpha=float,
                 print_summary=bool, vp_multiplier=float, sample_range_min=float, sample_range_max=float,
                 n_samples_heatmap=int, heatmap_multiplier=float, n_samples_feature=int, fconsis_multiplier=float,
                 use_ref_descriptor=bool, ref_multiplier=float)
    _UNSUPPORTED_TRUE = ("use_ref_descriptor",)

    def __init__(self, cfg=None):
        self.use_geometric, self.min_num_images, self.num_outliers_aggregate = True, 4, 2
        self.geometric_alpha, self.print_summary = 10.0, True
        self.vp_multiplier, self.heatmap_multiplier, self.n_samples_heatmap = 1.0, 1.0, 10
        self.sample_range_min, self.sample_range_max = 0.05, 0.95
        self.max_num_iterations = 100  # solver_options.max_num_iterations
        # not keys of upstream's C++ configuration: the python callers read them from the same dict
        self.num_outliers_aggregator = 2
        self.use_vp = self.use_heatmap = self.use_feature = False
        self.n_samples_feature, self.fconsis_multiplier = 100, 1.0
        self.use_ref_descriptor, self.ref_multiplier = False, 5.0
        self.channels = 128     # cfg["channels"] (line_refinement.py: the RefinementEngine's template argument)
        self.dtype = "float16"  # the texels of the heatmaps and features (line_refinement.py:27: cfg["dtype"])
        self._assign(cfg, dict(self._KEYS, num_outliers_aggregator=int, use_vp=bool, use_heatmap=bool, use_feature=bool,
                               dtype=str, channels=int))

    def _assign(self, cfg, keys):
        if cfg is None:
            return
        if not isinstance(cfg, dict):
            raise TypeError("the configuration must be a dict")
        for k, typ in keys.items():
            if k in cfg and cfg[k] is not None:
                setattr(self, k, typ(cfg[k]))

    def _check(self):
        for k in self._UNSUPPORTED_TRUE:
            if getattr(self, k):
                raise ValueError(f"limap_amd.optimize: {k}=True is not built here")
        if not (self.use_geometric or self.use_vp or self.use_heatmap or self.use_feature):
            raise ValueError("limap_amd.optimize: use_geometric=False leaves no residual")
        if (self.use_heatmap or self.use_feature) and self.dtype not in _TEXELS:
            raise ValueError(f"limap_amd.optimize: dtype={self.dtype!r} is not built (float16 or float32 texels)")
        if self.use_feature and self.channels != 128:
            raise ValueError(f"limap_amd.optimize: channels={self.channels} is not built (128, upstream's only instance)")

    def _feature(self, dtype=None):
        """lt_refine_feature, or None without the feature term"""
        if not self.use_feature:
            return None
        f = _capi.LtRefineFeature()
        _capi.load_library().lt_refine_feature_default(C.byref(f))
        f.n_samples_feature, f.fconsis_multiplier = int(self.n_samples_feature), float(self.fconsis_multiplier)
        f.channels, f.texel_type = int(self.channels), _TEXELS[dtype or self.dtype][1]
        return f

    def _terms(self):
        """lt_refine_terms, or None where none of the VP, heatmap and feature terms is on"""
        if not (self.use_vp or self.use_heatmap or self.use_feature):
            return None
        t = _capi.LtRefineTerms()
        _capi.load_library().lt_refine_terms_default(C.byref(t))
        t.use_geometric, t.use_vp, t.use_heatmap = int(self.use_geometric), int(self.use_vp), int(self.use_heatmap)
        t.n_samples_heatmap, t.vp_multiplier = int(self.n_samples_heatmap), float(self.vp_multiplier)
        t.sample_range_min, t.sample_range_max = float(self.sample_range_min), float(self.sample_range_max)
        t.heatmap_multiplier = float(self.heatmap_multiplier)
        t.texel_type = _TEXELS[self.dtype][1] if self.use_heatmap else _capi.TEXEL_F16
        return t

    def _struct(self, num_outliers, constant_line=False):
        c = _capi.LtRefineConfig()
        _capi.load_library().lt_refine_config_default(C.byref(c))
        c.geometric_alpha, c.min_num_images = float(self.geometric_alpha), int(self.min_num_images)
        c.num_outliers_aggregator, c.num_outliers_aggregate = int(num_outliers), int(self.num_outliers_aggregate)
        c.max_num_iterations, c.constant_line = int(self.max_num_iterations), int(bool(constant_line))
        return c


class HybridBAConfig(RefinementConfig):
    """optimize/hybrid_bundle_adjustment/hybrid_bundle_adjustment_config.h:17-49"""
    # no VP or heatmap term in the hybrid bundle adjustment; its feature term is not built
    _UNSUPPORTED_TRUE = ("use_vp", "use_heatmap", "use_feature", "use_ref_descriptor")
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

    def _check_ba(self):
        """the check of solve_point_bundle_adjustment / solve_hybrid_bundle_adjustment: poses may be free"""
        super()._check()
        if not self.constant_intrinsics:
            raise ValueError("limap_amd.optimize: constant_intrinsics=False is not built (set cfg_ba.constant_intrinsics = "
                             "True: the bundle adjustment holds the intrinsics constant)")

    def _ba_struct(self, num_outliers, poll_interval=None, kernel_timers=False):
        c = _capi.LtBaConfig()
        _capi.load_library().lt_ba_config_default(C.byref(c))
        c.geometric_alpha, c.lw_point = float(self.geometric_alpha), float(self.lw_point)
        c.min_num_images, c.num_outliers_aggregator = int(self.min_num_images), int(num_outliers)
        c.max_num_iterations = int(self.max_num_iterations)
        c.constant_intrinsics, c.constant_principal_point = int(self.constant_intrinsics), int(self.constant_principal_point)
        c.constant_pose, c.constant_point, c.constant_line = int(self.constant_pose), int(self.constant_point), int(self.constant_line)
        c.poll_interval, c.kernel_timers = int(poll_interval or 0), int(bool(kernel_timers))
        return c


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


class Heatmaps:
    """The heatmaps of a scene as the native calls take them: {img_id: (h, w) array} rounded to the texel type by
    numpy's astype (float64 -> float16 rounds once; upstream goes through float, which can differ in the last bit of
    a rare value: DESIGN.md section 19)."""

    def __init__(self, heatmaps, dtype="float16"):
        if dtype not in _TEXELS:
            raise ValueError(f"limap_amd.optimize: dtype={dtype!r} is not built (float16 or float32 texels)")
        np_type, self.texel_type = _TEXELS[dtype]
        self.ids = np.array(sorted(int(i) for i in heatmaps), np.int32)
        self.arrays = [np.ascontiguousarray(np.asarray(heatmaps[int(i)]).astype(np_type, copy=False)) for i in self.ids]
        for i, a in zip(self.ids, self.arrays):
            if a.ndim != 2 or a.size == 0:
                raise ValueError(f"limap_amd.optimize: the heatmap of image {i} is not a non-empty 2D array")
        self.h = np.array([a.shape[0] for a in self.arrays], np.int32)
        self.w = np.array([a.shape[1] for a in self.arrays], np.int32)
        self.ptrs = (C.c_void_p * max(len(self.arrays), 1))(*[a.ctypes.data for a in self.arrays])

    def args(self):
        p = _capi.ptr
        return len(self.ids), p(self.ids, C.c_int32), p(self.h, C.c_int32), p(self.w, C.c_int32), self.ptrs

    def upload(self, ctx):
        """once per context: a second call with the same object finds them resident, which the context's generation
        counter confirms (it moves with every set and clear, also one made through the C ABI directly or one whose
        copy failed)"""
        gen = ctx.L.lt_refine_heatmaps_generation(ctx.h)
        if getattr(ctx, "_refine_heatmaps", None) != (id(self), gen):
            ctx._refine_heatmaps = None
            ctx.chk(ctx.L.lt_refine_set_heatmaps(ctx.h, *self.args(), self.texel_type))
            ctx._refine_heatmaps_owner = self  # keeps id(self) from being reused
            ctx._refine_heatmaps = (id(self), ctx.L.lt_refine_heatmaps_generation(ctx.h))


def _texel_array(a, np_type, host, what):
    """an (h, w, 128) array or tensor -> its contiguous Operand in the texel type; a GPU tensor stays on the device
    unless the host path was asked for.  The context is not known yet: _on_context applies the device rule"""
    t = _native.operand(a, host=host, device=None, who="limap_amd.optimize", what=what)
    t = t.astype(np.dtype(np_type).name).contiguous()
    if t.ndim != 3 or t.shape[2] != 128 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"limap_amd.optimize: {what} must be (h, w, 128), got shape {t.shape}")
    return t


def _on_context(ctx, arrays, what):
    """the device rule for what _texel_array kept, against the context the call runs on, and the stream rule"""
    for a in arrays:
        _native.check_device(a, host=False, device=ctx.device, who="limap_amd.optimize", what=what)
    _native.wait_for_torch(ctx.device)


class FeatureMaps:
    """The feature maps of a scene (the map form of the feature term): {img_id: (H, W, 128) array or GPU tensor},
    rounded to the texel type by one astype like the heatmaps.  Host arrays are uploaded once per context, GPU tensors
    are read in place."""

    def __init__(self, featuremaps, dtype="float16", host=False):
        if dtype not in _TEXELS:
            raise ValueError(f"limap_amd.optimize: dtype={dtype!r} is not built (float16 or float32 texels)")
        np_type, self.texel_type = _TEXELS[dtype]
        self.ids = np.array(sorted(int(i) for i in featuremaps), np.int32)
        ent = [_texel_array(featuremaps[int(i)], np_type, host, f"the feature map of image {i}") for i in self.ids]
        dev = {e.on_device for e in ent}
        if len(dev) > 1:
            raise ValueError("limap_amd.optimize: featuremaps mixes host arrays and GPU tensors")
        self.on_device = int(bool(dev and dev.pop()))
        self.keep = [e.keep for e in ent]
        self.h = np.array([e.shape[0] for e in ent], np.int32)
        self.w = np.array([e.shape[1] for e in ent], np.int32)
        self.addr = {int(i): e.address for i, e in zip(self.ids, ent)}
        self.ptrs = (C.c_void_p * max(len(ent), 1))(*self.addr.values())

    def grid(self, img_id):
        """the identity grid of an image (host path)"""
        k = int(np.searchsorted(self.ids, img_id))
        if k >= len(self.ids) or self.ids[k] != img_id:
            return None
        return self.addr[int(img_id)], int(self.h[k]), int(self.w[k]), (1.0, 0.0, 0.0, 1.0), (0.0, 0.0), self.on_device

    def upload(self, ctx):
        """once per context, confirmed by the context's generation counter like Heatmaps.upload"""
        gen = ctx.L.lt_refine_feature_maps_generation(ctx.h)
        if getattr(ctx, "_refine_featuremaps", None) != (id(self), gen):
            ctx._refine_featuremaps = None
            if self.on_device:
                _on_context(ctx, self.keep, "a feature map")
            p = _capi.ptr
            ctx.chk(ctx.L.lt_refine_set_feature_maps(ctx.h, len(self.ids), p(self.ids, C.c_int32), p(self.h, C.c_int32),
                                                     p(self.w, C.c_int32), self.ptrs, self.texel_type, self.on_device))
            ctx._refine_featuremaps_owner = self
            ctx._refine_featuremaps = (id(self), ctx.L.lt_refine_feature_maps_generation(ctx.h))


def _grid_array(grids):
    """[(texels, h, w, R4, tvec2, on_device)] -> (lt_refine_grid array, count); texels: the array or tensor that holds
    them, or their address"""
    arr = (_capi.LtRefineGrid * max(len(grids), 1))()
    for g, (texels, h, w, R, tv, dev) in zip(arr, grids):
        g.data = int(texels) if isinstance(texels, (int, np.integer)) else _native.address(texels)
        g.h, g.w, g.on_device = int(h), int(w), int(dev)
        g.R[:] = [float(x) for x in R]
        g.tvec[:] = [float(x) for x in tv]
    return arr, len(grids)


def refine_arrays(cams, tracks_csr, cfg_struct, host_threads=None, ctx=None, terms=None, vp=None, view_hw=None,
                  heatmaps=None, feature=None, grids=None, featuremaps=None):
    """One call of lt_refine_arrays (device) or lt_fn_refine_host (host_threads given) -> dict of per-track results.
    terms (lt_refine_terms) selects the *_terms entry points: vp = (flag (M,), vp3 (M, 3)) per support in list order,
    view_hw (n_img, 2) or None, heatmaps a Heatmaps.  feature (lt_refine_feature) selects the *_feature entry points:
    grids = [(texels, h, w, R, tvec, on_device)] per (track, sorted image) -- texels the array or tensor itself, which
    the device rule is then applied to, or a bare address, which it cannot see -- or None with featuremaps (a
    FeatureMaps), which the device call reads from the context."""
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
    if terms is not None:
        flag, vp3 = vp if vp is not None else (np.zeros(len(img), np.int32), np.zeros((len(img), 3)))
        flag, vp3 = np.ascontiguousarray(flag, np.int32), np.ascontiguousarray(vp3, np.float64)
        hw = None if view_hw is None else np.ascontiguousarray(view_hw, np.int32)
        targs = (C.byref(terms), p(flag, C.c_int32), p(vp3, C.c_double), None if hw is None else p(hw, C.c_int32))
        if terms.use_heatmap and heatmaps is None:
            raise ValueError("limap_amd.optimize: use_heatmap without heatmaps")
    if feature is not None:
        if terms is None:
            raise ValueError("limap_amd.optimize: the feature term needs the terms")
        if grids is None and featuremaps is None:
            raise ValueError("limap_amd.optimize: use_feature without patches or feature maps")
        if grids is None and host_threads is not None:  # the host twin takes a map as the identity grid
            grids = []
            for n in range(T):
                for i in sorted(set(int(x) for x in img[off[n]:off[n + 1]])):
                    g = featuremaps.grid(i)
                    if g is None:
                        raise ValueError(f"limap_amd.optimize: image {i} supports track {n} and has no feature map")
                    grids.append(g)
        garr, n_grids = _grid_array(grids) if grids is not None else (None, 0)
    if host_threads is not None:
        hm = heatmaps.args() if terms is not None and terms.use_heatmap else (0, None, None, None, None)
        if terms is None:
            rc = L.lt_fn_refine_host(*args, int(host_threads), *outs)
        elif feature is None:
            rc = L.lt_fn_refine_host_terms(*args, *targs, *hm, int(host_threads), *outs)
        else:
            rc = L.lt_fn_refine_host_feature(*args, *targs, *hm, C.byref(feature), n_grids, garr, int(host_threads), *outs)
        if rc != 0:
            _native.raise_host_error(L, "lt_fn_refine_host_error", "limap_amd.optimize: ")
    else:
        ctx = ctx if ctx is not None else _context()
        if terms is None:
            ctx.chk(L.lt_refine_arrays(ctx.h, *args))
        else:
            if terms.use_heatmap:
                heatmaps.upload(ctx)
            if feature is None:
                ctx.chk(L.lt_refine_arrays_terms(ctx.h, *args, *targs))
            else:
                if grids is None:
                    featuremaps.upload(ctx)
                elif any(g[5] for g in grids):
                    _on_context(ctx, [g[0] for g in grids], "a patch")
                ctx.chk(L.lt_refine_arrays_feature(ctx.h, *args, *targs, C.byref(feature), n_grids, garr))
        ctx.chk(L.lt_refine_get(ctx.h, *outs))
        tm = ctx.module_timers("lt_refine_get_timers", 4)
        timers = dict(prepare_ms=float(tm[0]), kernels_ms=float(tm[1]), download_ms=float(tm[2]), lm_device_ms=float(tm[3]))
    return dict(params=P[:T], segments=seg[:T], cost=cost[:T], iterations=it[:T], codes=code[:T], timers=timers)


def _copy_track(t, line):
    n = LineTrack(line, t.image_id_list, t.line_id_list, t.line2d_list)
    n.node_id_list, n.line3d_list, n.score_list = list(t.node_id_list), list(t.line3d_list), list(t.score_list)
    n.active = getattr(t, "active", True)
    return n


def _point_arrays(tracks):
    """[PointTrack] -> p (T, 3), offsets, image ids, 2D points"""
    T = len(tracks)
    off = np.zeros(T + 1, np.int64)
    for n, t in enumerate(tracks):
        if len(t.p2d_list) != len(t.image_id_list) or len(t.p2d_id_list) not in (0, len(t.image_id_list)):
            raise ValueError(f"point track {n}: {len(t.image_id_list)} image ids, {len(t.p2d_id_list)} 2D point ids, "
                             f"{len(t.p2d_list)} 2D points")
        off[n + 1] = off[n] + len(t.image_id_list)
    M = int(off[-1])
    p3 = np.zeros((max(T, 1), 3)); img = np.zeros(max(M, 1), np.int32); xy = np.zeros((max(M, 1), 2))
    for n, t in enumerate(tracks):
        a, b = int(off[n]), int(off[n + 1])
        p3[n] = np.asarray(t.p, float).reshape(3)
        img[a:b] = t.image_id_list
        if b > a:
            xy[a:b] = np.asarray(t.p2d_list, float).reshape(-1, 2)
    return p3, off, img, xy


def ba_arrays(cams, points_csr, lines_csr, cfg_struct, host_threads=None, ctx=None):
    """One call of lt_ba_arrays (device) or lt_fn_ba_host (host_threads given) -> dict: qvec, tvec per image in the
    order of `cams`, points, params (uvec, wvec) and segments per line track, cost (initial, final), iterations, code."""
    ids, k, q, t = cams
    p3, poff, pimg, pxy = points_csr
    line6, loff, limg, l2, l3 = lines_csr
    NP, NL, N = len(poff) - 1, len(loff) - 1, len(ids)
    L = _capi.load_library()
    p = _capi.ptr
    qo = np.zeros((max(N, 1), 4)); to = np.zeros((max(N, 1), 3)); po = np.zeros((max(NP, 1), 3))
    P = np.zeros((max(NL, 1), 6)); seg = np.zeros((max(NL, 1), 6)); cost = np.zeros(2)
    it = np.zeros(1, np.int32); code = np.zeros(1, np.int32)
    args = (N, p(ids, C.c_int32), p(k, C.c_double), p(q, C.c_double), p(t, C.c_double), NP, p(p3, C.c_double),
            p(poff, C.c_int64), p(pimg, C.c_int32), p(pxy, C.c_double), NL, p(line6, C.c_double), p(loff, C.c_int64),
            p(limg, C.c_int32), p(l2, C.c_double), p(l3, C.c_double), C.byref(cfg_struct))
    outs = (p(qo, C.c_double), p(to, C.c_double), p(po, C.c_double), p(P, C.c_double), p(seg, C.c_double),
            p(cost, C.c_double), p(it, C.c_int32), p(code, C.c_int32))
    timers = None
    if host_threads is not None:
        if L.lt_fn_ba_host(*args, int(host_threads), *outs) != 0:
            _native.raise_host_error(L, "lt_fn_ba_host_error", "limap_amd.optimize: ")
    else:
        ctx = ctx if ctx is not None else _context()
        ctx.chk(L.lt_ba_arrays(ctx.h, *args))
        ctx.chk(L.lt_ba_get(ctx.h, *outs))
        tm = ctx.module_timers("lt_ba_get_timers", 16)
        names = ("linearize", "blocks", "images", "damp", "schur", "chol", "backsub", "cost", "decide")
        timers = dict(prepare_ms=float(tm[0]), loop_ms=float(tm[1]), download_ms=float(tm[2]), attempts_enqueued=int(tm[3]),
                      kernels_ms={"k_ba_" + n: float(tm[4 + i]) for i, n in enumerate(names)})
    return dict(qvec=qo[:N], tvec=to[:N], points=po[:NP], params=P[:NL], segments=seg[:NL], cost=cost,
                iterations=int(it[0]), code=int(code[0]), timers=timers)


class HybridBAEngine:
    """HybridBAEngine.  Built by solve_line_bundle_adjustment it is restricted to line tracks with constant cameras;
    built by solve_point_bundle_adjustment / solve_hybrid_bundle_adjustment (`ba=True`) it takes point tracks too and
    poses, points and lines are free unless the configuration holds them.  With constant poses
    the tracks separate: the lines run through the line refinement, every point track through its own solve.  The solve
    runs once, with the configuration's num_outliers_aggregator; GetOutputLineTracks with another num_outliers re-cuts
    the segments from the stored parameters (cut_segment), it does not solve again."""

    def __init__(self, cfg, imagecols, linetracks, host_threads=None, pointtracks=None, ba=False, poll_interval=None,
                 kernel_timers=False):
        self.config, self.host_threads = cfg, host_threads
        self._tracks = dict(enumerate(linetracks)) if not isinstance(linetracks, dict) else dict(linetracks)
        self._keys = sorted(self._tracks)
        pts = pointtracks if pointtracks is not None else {}
        pts = dict(enumerate(pts)) if not isinstance(pts, dict) else dict(pts)
        self._points = {k: (v if hasattr(v, "p2d_list") else PointTrack(v)) for k, v in pts.items()}
        self._pkeys = sorted(self._points)
        self._imagecols = imagecols
        self._cams = _camera_arrays({int(i): imagecols.camview(int(i)) for i in imagecols.get_img_ids()})
        self._csr = _track_arrays([self._tracks[k] for k in self._keys])
        self._n_out = int(cfg.num_outliers_aggregator)
        self._ba = None       # the result of lt_ba_arrays / lt_fn_ba_host, where one ran
        self._moved = set()   # the images that were parameters of the problem
        free = ba and not cfg.constant_pose
        if free:
            pcsr = _point_arrays([self._points[k] for k in self._pkeys])
            c = cfg._ba_struct(self._n_out, poll_interval, kernel_timers)
            self._ba = ba_arrays(self._cams, pcsr, self._csr, c, host_threads)
            n = len(self._keys)
            # the images that carry a residual block (SetUp's order of blocks does not matter for the set)
            self._moved = {int(i) for i in self._csr[2][:int(self._csr[1][-1])]}
            if cfg.lw_point > 0:
                self._moved |= {int(i) for i in pcsr[2][:int(pcsr[1][-1])]}
            # the per-track form of result(): one cost, iteration count and code per solve
            self._res = dict(params=self._ba["params"], segments=self._ba["segments"],
                             cost=np.tile(self._ba["cost"], (n, 1)), iterations=np.full(n, self._ba["iterations"], np.int32),
                             codes=np.full(n, self._ba["code"], np.int32), timers=self._ba["timers"])
        else:
            if self._keys:
                c = cfg._struct(self._n_out, getattr(cfg, "constant_line", False))
                self._res = refine_arrays(self._cams, self._csr, c, host_threads)
            else:
                self._res = dict(params=np.zeros((0, 6)), segments=np.zeros((0, 6)), cost=np.zeros((0, 2)),
                                 iterations=np.zeros(0, np.int32), codes=np.zeros(0, np.int32), timers=None)
            if ba and self._pkeys:
                none = (np.zeros((1, 6)), np.zeros(1, np.int64), np.zeros(1, np.int32), np.zeros((1, 4)), np.zeros((1, 6)))
                self._ba = ba_arrays(self._cams, _point_arrays([self._points[k] for k in self._pkeys]), none,
                                     cfg._ba_struct(self._n_out), host_threads)
        self._segs = {self._n_out: self._res["segments"]}

    def GetOutputPoints(self):
        """{track id: p}: the new points (the input's where no solve moved them)"""
        if self._ba is None:
            return {k: np.asarray(self._points[k].p, float).copy() for k in self._pkeys}
        return {k: self._ba["points"][n].copy() for n, k in enumerate(self._pkeys)}

    def GetOutputPointTracks(self):
        pts = self.GetOutputPoints()
        return {k: PointTrack(pts[k], self._points[k].image_id_list, self._points[k].p2d_id_list, self._points[k].p2d_list)
                for k in self._pkeys}

    def GetOutputImagecols(self):
        """a copy of the collection with the new poses; an image that was no parameter of the problem (constant poses,
        or no residual block) keeps its view"""
        views = {}
        for n, i in enumerate(self._cams[0]):
            v = self._imagecols.camview(int(i))
            if int(i) not in self._moved:
                views[int(i)] = copy.copy(v)
                continue
            name = v.image_name() if hasattr(v, "image_name") else "none"
            hw = (v.h(), v.w()) if hasattr(v, "h") and v.h() is not None else None
            views[int(i)] = CameraView(self._cams[1][n], self._ba["qvec"][n], self._ba["tvec"][n], name, hw)
        return ImageCollection(views)

    def _segments(self, num_outliers):
        if num_outliers not in self._segs:
            off, l3 = self._csr[1], self._csr[4]
            self._segs[num_outliers] = np.array([cut_segment(self._res["params"][n], l3[off[n]:off[n + 1]], num_outliers)
                                                 for n in range(len(self._keys))]).reshape(-1, 6)
        return self._segs[num_outliers]

    def result(self, num_outliers=None):
        """per-track arrays: params (uvec, wvec), segments, cost (initial, final), iterations, codes (TERMINATION).
        After a free-pose solve also `cost_ba` (initial, final), `iterations_ba`, `code` of the one solve, and `qvec`,
        `tvec` (images in ascending id), `points`"""
        n_out = self._n_out if num_outliers is None else int(num_outliers)
        r = dict(self._res, segments=self._segments(n_out))
        if self._ba is not None:  # (with constant poses: of the separated point solves)
            r.update(cost_ba=self._ba["cost"], iterations_ba=self._ba["iterations"], code=self._ba["code"],
                     qvec=self._ba["qvec"], tvec=self._ba["tvec"], points=self._ba["points"])
        return r

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


def solve_hybrid_bundle_adjustment(cfg, imagecols, pointtracks, linetracks, max_num_iterations=100, host_threads=None,
                                   poll_interval=None, kernel_timers=False):
    """optimize/hybrid_bundle_adjustment/solve.py:42-51 with constant intrinsics: poses, points and lines are free unless
    constant_pose / constant_point / constant_line say otherwise.  Lists or dicts of tracks, as the two Init*Tracks
    overloads.  poll_interval: attempts enqueued between two reads of the device's status record (no effect on the
    result).  With constant_pose=True the tracks separate: the lines are solved as solve_line_bundle_adjustment solves
    them, bit for bit, and every point track by its own solve.  ValueError: constant_intrinsics=False; more than
    BA_MAX_IMAGES images with residuals (LT_BA_MAX_IMAGES)."""
    ba = HybridBAConfig(cfg) if isinstance(cfg, dict) or cfg is None else cfg
    if not isinstance(ba, HybridBAConfig):
        raise TypeError("cfg must be a dict or a HybridBAConfig")
    ba._check_ba()
    ba = copy.copy(ba)  # the caller's configuration is not changed
    ba.max_num_iterations = int(max_num_iterations)
    pointtracks = pointtracks if pointtracks is not None else {}
    linetracks = linetracks if linetracks is not None else {}
    return HybridBAEngine(ba, imagecols, linetracks, host_threads, pointtracks=pointtracks, ba=True,
                          poll_interval=poll_interval, kernel_timers=kernel_timers)


def solve_point_bundle_adjustment(cfg, imagecols, pointtracks, max_num_iterations=100, host_threads=None,
                                  poll_interval=None, kernel_timers=False):
    """optimize/hybrid_bundle_adjustment/solve.py:20-28"""
    return solve_hybrid_bundle_adjustment(cfg, imagecols, pointtracks, {}, max_num_iterations, host_threads,
                                          poll_interval, kernel_timers)


class RefinementEngine:
    def __init__(self, result):
        self._r = result

    def GetLine3d(self):
        s = self._r["segments"][0]
        return Line3d(s[:3], s[3:])

    def result(self):
        return self._r


def _refinement_cfg(cfg):
    rf = RefinementConfig(cfg) if isinstance(cfg, dict) or cfg is None else cfg
    rf._check()
    return rf


def _vp_pair(r):
    """a VPResult in any form InitVPResults accepts -> labels, vps (V, 3)"""
    if isinstance(r, dict):
        lab, vps = r["labels"], r["vps"]
    elif hasattr(r, "labels"):
        lab, vps = r.labels, r.vps
    else:
        lab, vps = r
    return np.asarray(lab, np.int64).reshape(-1), np.asarray(vps, float).reshape(-1, 3)


def _vp_arrays(tracks, vpresults):
    """per support, list order: the flag (label >= 0 for line_id_list[k]: HasVP) and the vanishing point
    (refine.cc:101-103); vpresults: {img_id: VPResult}"""
    flat = {}
    flag, vp3 = [], []
    for t in tracks:
        for img_id, line_id in zip(t.image_id_list, t.line_id_list):
            if img_id not in flat:
                if img_id not in vpresults:
                    raise ValueError(f"limap_amd.optimize: use_vp and no VPResult for image {img_id}")
                flat[img_id] = _vp_pair(vpresults[img_id])
            lab, vps = flat[img_id]
            label = int(lab[line_id])
            flag.append(label >= 0)
            vp3.append(vps[label] if label >= 0 else np.zeros(3))
    return np.array(flag, np.int32), np.array(vp3, np.float64).reshape(-1, 3)


def _view_hw(ids, views):
    """(h, w) per camera row; 0 where the view carries no size"""
    return np.array([[views[int(i)].h() or 0, views[int(i)].w() or 0] for i in ids], np.int32).reshape(-1, 2)


def _patch_grids(patches, np_type, host, what):
    """PatchInfos of one track's sorted images -> grid tuples (which hold the texels' memory), their texel bytes"""
    grids, nbytes = [], 0
    for k, pt in enumerate(patches):
        if not hasattr(pt, "array") or not hasattr(pt, "R") or not hasattr(pt, "tvec"):
            raise ValueError(f"limap_amd.optimize: {what}[{k}] is not a features.PatchInfo")
        a = _texel_array(pt.array, np_type, host, f"{what}[{k}].array")
        grids.append((a.keep, *a.shape[:2], np.asarray(pt.R, np.float64).reshape(4),
                      np.asarray(pt.tvec, np.float64).reshape(2), a.on_device))
        nbytes += a.shape[0] * a.shape[1] * 128 * np.dtype(np_type).itemsize
    return grids, nbytes


def _refine(rf, tracks, views, vpresults, heatmaps, host_threads, patches=None, featuremaps=None, dtype=None,
            patch_bytes=FEATURE_PATCH_BYTES):
    """all `tracks` in one native call -- with patches in as many as the byte budget asks for; views, vpresults:
    {img_id: ...}; heatmaps: a Heatmaps; patches: per track the PatchInfos of its sorted images; featuremaps: a
    FeatureMaps"""
    cams = _camera_arrays(views)
    terms = rf._terms()
    cfg = rf._struct(rf.num_outliers_aggregate)
    hw = _view_hw(cams[0], views) if rf.use_heatmap else None

    def call(sub, **kw):
        vp = _vp_arrays(sub, vpresults) if rf.use_vp else None
        return refine_arrays(cams, _track_arrays(sub), cfg, host_threads, terms=terms, vp=vp, view_hw=hw, heatmaps=heatmaps, **kw)

    if not rf.use_feature:
        return call(tracks)
    feature = rf._feature(dtype)
    if patches is None:
        return call(tracks, feature=feature, featuremaps=featuremaps)
    # tracks in their order, a new native call where the next track's texels would pass the budget: every track is its
    # own problem, so the grouping does not reach the results
    np_type = _TEXELS[dtype or rf.dtype][0]
    parts, group, grids, used = [], [], [], 0
    for n, t in enumerate(tracks):
        g, nb = _patch_grids(patches[n], np_type, host_threads is not None, f"the patches of track {n}")
        if group and used + nb > int(patch_bytes):
            parts.append(call(group, feature=feature, grids=grids))
            group, grids, used = [], [], 0
        group.append(t); grids += g; used += nb
    parts.append(call(group, feature=feature, grids=grids))
    out = {k: np.concatenate([r[k] for r in parts]) for k in ("params", "segments", "cost", "iterations", "codes")}
    out["timers"] = None if parts[0]["timers"] is None else {k: sum(r["timers"][k] for r in parts) for k in parts[0]["timers"]}
    out["calls"] = len(parts)
    return out


def solve_line_refinement(cfg, track, p_camviews, p_vpresults=None, p_heatmaps=None, p_patches=None, p_features=None,
                          dtype=None, host_threads=None):
    """optimize/line_refinement/solve.py:4-48: p_camviews, p_vpresults, p_heatmaps, p_patches (features.PatchInfo) and
    p_features ((H, W, 128) arrays or GPU tensors) are the views, VPResults, heatmaps, patches and feature maps of
    track.GetSortedImageIds(), in that order.  dtype: the texels ("float16" / "float32"; the configuration's by
    default).  None below min_num_images."""
    for name, lst in (("p_vpresults", p_vpresults), ("p_heatmaps", p_heatmaps), ("p_patches", p_patches),
                      ("p_features", p_features)):
        if lst is not None and len(lst) != len(p_camviews):
            raise ValueError(f"limap_amd.optimize: {name} has {len(lst)} entries for {len(p_camviews)} views")
    rf = _refinement_cfg(cfg)
    if p_patches is not None and p_features is not None:
        raise ValueError("limap_amd.optimize: p_patches and p_features are both given")
    for name, lst in (("p_patches", p_patches), ("p_features", p_features)):
        if lst is not None and not rf.use_feature:
            raise ValueError(f"limap_amd.optimize: {name} is given and use_feature is off")
    if rf.use_feature and p_patches is None and p_features is None:
        raise ValueError("limap_amd.optimize: use_feature=True needs p_patches / p_features")
    if rf.use_vp and p_vpresults is None:
        raise ValueError("limap_amd.optimize: use_vp=True needs p_vpresults")
    if rf.use_heatmap and p_heatmaps is None:
        raise ValueError("limap_amd.optimize: use_heatmap=True needs p_heatmaps")
    if track.count_images() < rf.min_num_images:
        return None
    ids = track.GetSortedImageIds()
    if len(p_camviews) != len(ids):
        raise ValueError(f"{len(ids)} images support the track, {len(p_camviews)} views given")
    hm = Heatmaps(dict(zip(ids, p_heatmaps)), dtype or rf.dtype) if rf.use_heatmap else None
    fm = None
    if rf.use_feature and p_features is not None:
        fm = FeatureMaps(dict(zip(ids, p_features)), dtype or rf.dtype, host_threads is not None)
    r = _refine(rf, [track], dict(zip(ids, p_camviews)), dict(zip(ids, p_vpresults)) if rf.use_vp else None, hm, host_threads,
                patches=[list(p_patches)] if rf.use_feature and p_patches is not None else None, featuremaps=fm, dtype=dtype)
    return RefinementEngine(r)


def line_refinement(cfg, tracks, imagecols, heatmap_dir=None, patch_dir=None, featuremap_dir=None, vpresults=None,
                    n_visible_views=4, host_threads=None, heatmaps=None, patches=None, featuremaps=None,
                    patch_bytes=FEATURE_PATCH_BYTES):
    """optimize/line_refinement/line_refinement.py:15-136: the tracks seen in at least n_visible_views images and
    min_num_images images are refined, the others pass through.  heatmap_dir holds heatmap_{img_id}.npy;
    heatmaps={img_id: array} gives them directly.  With use_feature, patch_dir holds track{t}/track{t}_img{i}.npy
    (features.load_patch) and patches={(t, img_id): PatchInfo} gives them directly, t the track's index in `tracks`;
    without patches, featuremap_dir holds feature_{img_id}.npy stored (C, H, W) and featuremaps={img_id: (H, W, 128)
    array or GPU tensor} gives the maps directly.  Every image is loaded and uploaded once; tracks with patches run in
    native calls of at most patch_bytes of texels each, which does not change a result."""
    import os
    rf = _refinement_cfg(cfg)
    by_patch = patch_dir is not None or patches is not None
    if rf.use_feature and not by_patch and featuremap_dir is None and featuremaps is None:
        raise ValueError("limap_amd.optimize: use_feature=True needs patches / feature maps (patch_dir, patches, "
                         "featuremap_dir or featuremaps)")
    if rf.use_vp and vpresults is None:
        raise ValueError("limap_amd.optimize: use_vp=True needs vpresults")
    if rf.use_heatmap and heatmap_dir is None and heatmaps is None:
        raise ValueError("limap_amd.optimize: use_heatmap=True needs heatmap_dir or heatmaps")
    sel = [n for n, t in enumerate(tracks) if t.count_images() >= max(int(n_visible_views), rf.min_num_images)]
    out = list(tracks)
    if sel:
        views = {int(i): imagecols.camview(int(i)) for i in imagecols.get_img_ids()}
        hm = fm = plist = None
        if rf.use_heatmap:
            if heatmaps is None:
                files = {i: os.path.join(heatmap_dir, f"heatmap_{i}.npy") for i in views}
                heatmaps = {i: np.load(f) for i, f in files.items() if os.path.exists(f)}
            hm = Heatmaps(heatmaps, rf.dtype)
        if rf.use_feature and by_patch:
            from . import features
            plist = []
            for n in sel:
                row = []
                for i in tracks[n].GetSortedImageIds():
                    pt = patches.get((n, int(i))) if patches is not None else None
                    if pt is None and patch_dir is not None:
                        fname = os.path.join(patch_dir, f"track{n}", f"track{n}_img{int(i)}.npy")
                        pt = features.load_patch(fname, dtype=rf.dtype) if os.path.exists(fname) else None
                    if pt is None:
                        raise ValueError(f"limap_amd.optimize: no patch for track {n}, image {int(i)}")
                    row.append(pt)
                plist.append(row)
        elif rf.use_feature:
            if featuremaps is None:
                files = {i: os.path.join(featuremap_dir, f"feature_{i}.npy") for i in views}
                featuremaps = {i: np.load(f, allow_pickle=False).transpose(1, 2, 0) for i, f in files.items() if os.path.exists(f)}
            for n in sel:
                for i in tracks[n].GetSortedImageIds():
                    if int(i) not in featuremaps:
                        raise ValueError(f"limap_amd.optimize: no feature map for track {n}, image {int(i)}")
            fm = FeatureMaps(featuremaps, rf.dtype, host_threads is not None)
        r = _refine(rf, [tracks[n] for n in sel], views, vpresults, hm, host_threads, patches=plist, featuremaps=fm,
                    patch_bytes=patch_bytes)
        for m, n in enumerate(sel):
            out[n] = _copy_track(tracks[n], Line3d(r["segments"][m, :3], r["segments"][m, 3:]))
    return out


# limap.optimize.hybrid_localization and the null-RANSAC path of limap.estimators.pl_estimate_absolute_pose: the
# point-line pose refinement and the pose scoring
from . import hybrid_localization as _loc  # noqa: E402
from .hybrid_localization import *  # noqa: E402,F401,F403

__all__ += _loc.__all__

# limap.optimize.global_pl_association: the joint optimisation of points, lines and vanishing points under soft
# association constraints
from . import global_pl_association as _assoc  # noqa: E402,F401  (it adds its names to this module, whichever loads first)
