"""Mirror of `limap.fitting` and of the fit step of `limap.runners.line_fitnmerge` with the fitter on the GPU:

    Fit3DPoints, estimate_seg3d, estimate_seg3d_from_depth   (fitting/fitting.py:8-53, fitting/line3d_estimator.cc)
    fit_3d_segs                                              (runners/line_fitnmerge.py:17-70)
    fit_3d_segs_arrays                                       the fast form: (M, 2, 3) per image plus stats
    estimate_seg3d_from_points3d                             (fitting/fitting.py:56-102), 3D point scans
    fit_3d_segs_with_points3d                                (runners/line_fitnmerge.py:73-130)
    fit_3d_segs_with_points3d_arrays                         its fast form
    tracks_from_fit                                          one track per fitted segment (line_fitnmerge.py:210-221)

Same names, arguments and results.  LO-MSAC runs with the project's counter-based generator: `random_seed_` (or `seed`)
decides the draws and a segment's result depends on (seed, image id, line index) alone -- not on the batch, the image
order, the chunking or the device.  The reference reseeds from std::random_device on every call.
"""
import ctypes as C
import math

import numpy as np

from . import _capi, _native
from .base import Line3d

STATUS_OK, STATUS_TOO_FEW_POINTS, STATUS_LOW_INLIER_RATIO, STATUS_SCAN_OUT_OF_RANGE = 0, 1, 2, 3
STATS_FIELDS = ("num_points", "num_inliers", "num_iterations", "number_lo_iterations", "from_lo")  # columns of stats


class LORansacOptions:
    """ransac_lib::LORansacOptions as estimators/bindings.cc:50-75 exposes it, with RansacLib's defaults."""

    def __init__(self):
        self.min_num_iterations_ = 100
        self.max_num_iterations_ = 10000
        self.success_probability_ = 0.9999
        self.squared_inlier_threshold_ = 1.0
        self.random_seed_ = 0
        self.num_lo_steps_ = 10
        self.threshold_multiplier_ = math.sqrt(2.0)
        self.num_lsq_iterations_ = 4
        self.min_sample_multiplicator_ = 7
        self.non_min_sample_multiplier_ = 3
        self.lo_starting_iterations_ = 50
        self.final_least_squares_ = False


class RansacStatistics:
    """ransac_lib::RansacStatistics of Fit3DPoints"""

    def __init__(self, num_iterations, best_num_inliers, inlier_ratio, inlier_indices, number_lo_iterations, from_lo):
        self.num_iterations = num_iterations
        self.best_num_inliers = best_num_inliers
        self.inlier_ratio = inlier_ratio
        self.inlier_indices = inlier_indices
        self.number_lo_iterations = number_lo_iterations
        self.from_lo = from_lo


def _check_int(name, v, lo, hi):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError(f"fitting: {name} must be an integer in [{lo}, {hi}], got {v!r}")
    return int(v)


def _check_float(name, v, nonneg=False):
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"fitting: {name} must be a number, got {v!r}") from None
    if not math.isfinite(f) or (nonneg and f < 0.0):
        raise ValueError(f"fitting: {name} must be finite{' and >= 0' if nonneg else ''}, got {v!r}")
    return f


def _config(options=None, ransac_th=0.75, min_percentage_inliers=0.6, var2d=5.0, seed=None):
    """lt_fit_config from LORansacOptions (or None: defaults), checked here before any device work"""
    o = options if options is not None else LORansacOptions()
    c = _capi.LtFitConfig()
    c.ransac_th = _check_float("ransac_th", ransac_th)
    c.min_percentage_inliers = _check_float("min_percentage_inliers", min_percentage_inliers)
    c.var2d = _check_float("var2d", var2d)
    c.squared_inlier_threshold = _check_float("squared_inlier_threshold_", o.squared_inlier_threshold_, nonneg=True)
    p = _check_float("success_probability_", o.success_probability_)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"fitting: success_probability_ must lie in [0, 1], got {p}")
    c.success_probability = p
    c.threshold_multiplier = _check_float("threshold_multiplier_", o.threshold_multiplier_)
    c.min_num_iterations = _check_int("min_num_iterations_", o.min_num_iterations_, 0, 10_000_000)
    c.max_num_iterations = _check_int("max_num_iterations_", o.max_num_iterations_, 0, 10_000_000)
    c.num_lo_steps = _check_int("num_lo_steps_", o.num_lo_steps_, 0, 100_000)
    c.num_lsq_iterations = _check_int("num_lsq_iterations_", o.num_lsq_iterations_, 0, 100_000)
    c.min_sample_multiplicator = _check_int("min_sample_multiplicator_", o.min_sample_multiplicator_, 0, 1_000_000)
    c.non_min_sample_multiplier = _check_int("non_min_sample_multiplier_", o.non_min_sample_multiplier_, 0, 1_000_000)
    c.lo_starting_iterations = _check_int("lo_starting_iterations_", o.lo_starting_iterations_, 0, 2**31 - 1)
    c.final_least_squares = 1 if bool(o.final_least_squares_) else 0
    s = o.random_seed_ if seed is None else seed
    c.seed = _check_int("seed", s, -(2**63), 2**64 - 1) & (2**64 - 1)
    return c


_context = _capi.per_device_contexts()  # for the calls that bring no scene (lt_fit_points)


# ---- point sets -----------------------------------------------------------------------------------------------------
def fit_points_arrays(point_sets, options=None, min_percentage_inliers=0.0, device=0):
    """lt_fit_points over a list of (N_i, 3) point sets: -> dict(seg (S, 2, 3), status (S,), stats (S, 5),
    inlier_mask (sum N_i,), off (S + 1,))"""
    sets = [np.ascontiguousarray(np.asarray(p, np.float64).reshape(-1, 3)) for p in point_sets]
    off = np.zeros(len(sets) + 1, np.int64)
    off[1:] = np.cumsum([len(p) for p in sets])
    cfg = _config(options, min_percentage_inliers=min_percentage_inliers)
    xyz = np.ascontiguousarray(np.concatenate(sets, 0) if sets else np.zeros((0, 3)))
    S, N = len(sets), int(off[-1])
    seg = np.zeros((max(S, 1), 6)); status = np.zeros(max(S, 1), np.int32); stats = np.zeros((max(S, 1), 5), np.int32)
    mask = np.zeros(max(N, 1), np.uint8)
    ctx = _context(device)
    p = _capi.ptr
    ctx.chk(ctx.L.lt_fit_points(ctx.h, S, p(off, C.c_int64), p(xyz.reshape(-1) if N else np.zeros(3), C.c_double),
                                C.byref(cfg), p(seg, C.c_double), p(status, C.c_int32), p(stats, C.c_int32),
                                p(mask, C.c_uint8)))
    return dict(seg=seg[:S].reshape(S, 2, 3), status=status[:S], stats=stats[:S], inlier_mask=mask[:N].astype(bool),
                off=off)


def Fit3DPoints(points, options):
    """fitting::Fit3DPoints (line3d_estimator.cc:7-44): points (3, N) -> (Line3d, RansacStatistics)"""
    P = np.asarray(points, np.float64)
    if P.ndim != 2 or P.shape[0] != 3:
        raise ValueError(f"Fit3DPoints: points must be (3, N), got shape {P.shape}")
    r = fit_points_arrays([P.T], options, min_percentage_inliers=0.0)
    st = r["stats"][0]
    inl = np.nonzero(r["inlier_mask"])[0].tolist()
    n = P.shape[1]
    ratio = len(inl) / n if n >= 2 else 0.0
    stats = RansacStatistics(int(st[2]), int(st[1]), ratio, inl, int(st[3]), bool(st[4]))
    seg = r["seg"][0]
    return Line3d(seg[0], seg[1]), stats


def estimate_seg3d(points, ransac_th=0.75, min_percentage_inliers=0.6):
    """fitting.py:8-18: None or (start, end)"""
    options = LORansacOptions()
    options.squared_inlier_threshold_ = ransac_th * ransac_th
    line, stats = Fit3DPoints(points, options)
    if stats.inlier_ratio < min_percentage_inliers:
        return None
    return line.start, line.end


# ---- depth maps -----------------------------------------------------------------------------------------------------
def _map_of(depth, device=0):
    """(LtDepthMap, keep-alive) of a NumPy array or a torch tensor; integer maps become float64 (exact), like NumPy's
    promotion in the reference; float16 is refused.  A GPU tensor is read in place (_native.operand)."""
    d = _native.operand(depth, host=False, device=device, who="fitting", what="a depth map")
    if d.ndim != 2:
        raise ValueError(f"fitting: a depth map must be 2-D, got shape {d.shape}")
    if d.dtype in ("float16", "bfloat16"):
        raise ValueError("fitting: float16 depth maps are not supported")
    if d.dtype not in ("float32", "float64"):
        if not d.dtype.startswith(("int", "uint", "bool")):
            raise ValueError(f"fitting: unsupported depth dtype {d.dtype}")
        d = d.astype("float64")
    if d.strides[1] != 1 or d.strides[0] < d.shape[1]:
        d = d.contiguous()
    dm = _capi.LtDepthMap(C.c_void_p(d.address), d.shape[0], d.shape[1], d.strides[0],
                          0 if d.dtype == "float32" else 1, d.on_device)
    return dm, d.keep


def _shape_of(depth):
    return tuple(int(v) for v in depth.shape)


def _view_hw(camview):
    """(h, w) of a view that knows its image size (limap's CameraView, base.CameraView(..., hw=...)), else None"""
    if not (hasattr(camview, "h") and hasattr(camview, "w")):
        return None
    h, w = camview.h(), camview.w()
    if h is None or w is None:
        return None
    return int(h), int(w)


def _read_depth(reader, camview):
    """a reader's map (read_depth(img_hw=[h, w]) when the view knows its size), an array or a tensor"""
    hw = _view_hw(camview)
    if hasattr(reader, "read_depth"):
        d = reader.read_depth(img_hw=list(hw)) if hw is not None else reader.read_depth()
    else:
        d = reader
    if hw is not None:
        if _shape_of(d)[:2] != hw:
            raise ValueError(f"fitting: depth map of shape {_shape_of(d)} for a view of {hw[0]} x {hw[1]}")
    return d


def _segs4(segs):
    s = np.asarray(segs, np.float64)
    if s.size == 0:
        return np.zeros((0, 4))
    s = s.reshape(len(s), -1)
    if s.shape[1] < 4:
        raise ValueError(f"fitting: 2D segments need 4 columns, got {s.shape}")
    s = np.ascontiguousarray(s[:, :4])
    if not (np.abs(s) < 2.0**29).all():
        raise ValueError("fitting: 2D segment coordinates must be finite and below 2^29 in magnitude")
    return s


def _fitting_args(fitting_config):
    fc = dict(fitting_config or {})
    return (fc.get("ransac_th", 0.75), fc.get("min_percentage_inliers", 0.6), fc.get("var2d", 5.0))


def _scene_of(all_2d_segs, imagecols):
    """the images in ascending id order: ids, (kvec, qvec, tvec) arrays, segment offsets, all segments (G, 4)"""
    from .triangulation import _view_arrays
    ids = sorted(int(i) for i in imagecols.get_img_ids())
    segs = {}
    k = np.zeros((len(ids), 4)); q = np.zeros((len(ids), 4)); t = np.zeros((len(ids), 3))
    seg_off = np.zeros(len(ids) + 1, np.int64)
    for n, i in enumerate(ids):
        k[n], q[n], t[n] = _view_arrays(imagecols.camview(i))
        segs[i] = _segs4(all_2d_segs[i]) if i in all_2d_segs else np.zeros((0, 4))
        seg_off[n + 1] = seg_off[n] + len(segs[i])
    allsegs = np.ascontiguousarray(np.concatenate([segs[i] for i in ids], 0)) if ids else np.zeros((0, 4))
    return ids, (k, q, t), seg_off, allsegs


def _fit_chunks(ids, cams, seg_off, allsegs, map_of, nbytes_of, launch, max_chunk_bytes, device):
    """the chunk loop of the per-image fits: map_of(m) -> (map record, keep-alive) for the m-th image, read once;
    launch(ctx, n, maps, seg, status, stats) fits the images [n, n + len(maps)).  Chunks keep their maps' bytes under
    max_chunk_bytes (at least one map each); the results do not depend on the chunking.
    -> (seg (G, 6), status (G,), stats (G, 5), timers)"""
    G = int(seg_off[-1])
    seg = np.zeros((max(G, 1), 6)); status = np.zeros(max(G, 1), np.int32); stats = np.zeros((max(G, 1), 5), np.int32)
    timers = dict(device_ms=0.0, upload_ms=0.0, host_ms=0.0, attempts=0, chunks=0)
    ctx = None
    n = 0
    carry = None  # the map that did not fit into the last chunk: it opens the next one (a reader is not read twice)
    while n < len(ids):
        # the maps of one chunk are read and checked before its device work (the context comes after the first chunk)
        maps, keep, used, on_dev = [], [], 0, False
        m = n
        while m < len(ids):
            if carry is not None:
                (dm, ka), carry = carry, None
            else:
                dm, ka = map_of(m)
            nbytes = nbytes_of(dm)
            if m > n and used + nbytes > max_chunk_bytes:
                carry = (dm, ka)
                break
            maps.append(dm); keep.append(ka); used += nbytes; on_dev = on_dev or bool(dm.on_device)
            m += 1
        if ctx is None:
            ctx = _capi.Context(device=device)
            ctx.init(ids, *cams, seg_off, allsegs)
        if on_dev:
            _native.wait_for_torch(device)
        g0 = int(seg_off[n])
        launch(ctx, n, maps, seg[g0:], status[g0:], stats[g0:])
        tm = ctx.module_timers("lt_fit_get_timers", 4)
        timers["device_ms"] += tm[0]; timers["upload_ms"] += tm[1]; timers["host_ms"] += tm[2]
        timers["attempts"] = max(timers["attempts"], int(tm[3])); timers["chunks"] += 1
        del keep
        n = m
    return seg, status, stats, timers


def _per_image(ids, seg_off, seg, status, stats):
    out, info = {}, {}
    for j, i in enumerate(ids):
        a, b = int(seg_off[j]), int(seg_off[j + 1])
        out[i] = seg[a:b].reshape(b - a, 2, 3).copy()
        info[i] = dict(status=status[a:b].copy(), stats=stats[a:b].copy())
    return out, info


def fit_3d_segs_arrays(all_2d_segs, imagecols, depths, fitting_config=None, seed=0, max_chunk_bytes=1 << 30,
                       options=None, device=0):
    """fit_3d_segs in array form: -> (dict img_id -> (M, 2, 3) float64, dict img_id -> dict(status (M,), stats (M, 5)),
    timers).  Images go through the device in ascending id order in chunks whose depth maps stay under
    max_chunk_bytes; the results do not depend on the chunking."""
    ransac_th, min_pct, var2d = _fitting_args(fitting_config)
    cfg = _config(options, ransac_th, min_pct, var2d, seed)
    ids, cams, seg_off, allsegs = _scene_of(all_2d_segs, imagecols)
    for i in ids:
        if i not in depths:
            raise KeyError(f"fitting: no depth map for image {i}")
    p = _capi.ptr

    def launch(ctx, n, maps, seg, status, stats):
        arr = (_capi.LtDepthMap * len(maps))(*maps)
        ctx.chk(ctx.L.lt_fit_segs(ctx.h, n, len(maps), arr, C.byref(cfg), p(seg, C.c_double), p(status, C.c_int32),
                                  p(stats, C.c_int32)))

    seg, status, stats, timers = _fit_chunks(
        ids, cams, seg_off, allsegs, lambda m: _map_of(_read_depth(depths[ids[m]], imagecols.camview(ids[m])), device),
        lambda dm: int(dm.h) * int(dm.row_stride) * (4 if dm.dtype == 0 else 8), launch, max_chunk_bytes, device)
    out, info = _per_image(ids, seg_off, seg, status, stats)
    return out, info, timers


def fit_3d_segs(all_2d_segs, imagecols, depths, fitting_config, seed=0, max_chunk_bytes=1 << 30):
    """runners/line_fitnmerge.py:17-70: dict img_id -> list of (start, end) float64 (3,) arrays, zeros where the fit
    fails.  fitting_config["n_jobs"] is accepted and ignored."""
    arrs, _, _ = fit_3d_segs_arrays(all_2d_segs, imagecols, depths, fitting_config, seed, max_chunk_bytes)
    return {i: [(a[0].copy(), a[1].copy()) for a in arrs[i]] for i in arrs}


def estimate_seg3d_from_depth(seg2d, depth, camview, ransac_th=0.75, min_percentage_inliers=0.6, var2d=5.0, seed=0):
    """fitting.py:20-53 for one segment: None or (start, end)"""
    from .base import ImageCollection
    ic = ImageCollection({0: camview})
    arrs, info, _ = fit_3d_segs_arrays({0: np.asarray(seg2d, np.float64).reshape(1, -1)}, ic, {0: depth},
                                       dict(ransac_th=ransac_th, min_percentage_inliers=min_percentage_inliers,
                                            var2d=var2d), seed=seed)
    if info[0]["status"][0] != STATUS_OK:
        return None
    return arrs[0][0, 0].copy(), arrs[0][0, 1].copy()


# ---- 3D point scans -------------------------------------------------------------------------------------------------
def _scan_of(p3ds, img_hw, device=0):
    """(LtScanMap, keep-alive) of an (H, W, 3) NumPy array or torch tensor (a reader's read_p3ds()), img_hw the camera's
    (h, w).  float32 and float64 only (the reference's grid_sample takes float64; float32 is widened exactly); any
    non-negative strides are read in place, a GPU tensor where it lies (_native.operand)."""
    s = _native.operand(p3ds, host=False, device=device, who="fitting", what="a scan")
    if s.ndim != 3 or s.shape[2] != 3:
        raise ValueError(f"fitting: a scan must be (H, W, 3), got shape {s.shape}")
    if s.dtype not in ("float32", "float64"):
        raise ValueError(f"fitting: scans must be float32 or float64, got {getattr(p3ds, 'dtype', s.dtype)}")
    if s.shape[0] < 2 or s.shape[1] < 2:
        raise ValueError(f"fitting: a scan needs at least 2 x 2 pixels, got shape {s.shape}")
    if any(v < 0 for v in s.strides):
        s = s.contiguous()
    sm = _capi.LtScanMap(C.c_void_p(s.address), s.shape[0], s.shape[1], *s.strides, img_hw[0], img_hw[1],
                         0 if s.dtype == "float32" else 1, s.on_device)
    return sm, s.keep


def _scan_nbytes(sm):
    return int(sm.h) * int(sm.w) * 3 * (4 if sm.dtype == 0 else 8)


def _view_size(camview, img_id):
    hw = _view_hw(camview)
    if hw is None:
        raise ValueError(f"fitting: the view of image {img_id} has no image size (camview.h(), camview.w()); "
                         "base.CameraView takes it as hw=(h, w)")
    if hw[0] < 2 or hw[1] < 2 or hw[0] > 2**24 or hw[1] > 2**24:
        raise ValueError(f"fitting: image {img_id} of {hw[0]} x {hw[1]}: sizes must lie in [2, 2^24]")
    return hw


def _read_p3ds(reader):
    return reader.read_p3ds() if hasattr(reader, "read_p3ds") else reader


def _pose_rows(T, img_id):
    """Tr[:3, :4] of a 4 x 4 (or 3 x 4) scan pose, row-major, finite"""
    a = np.asarray(T, np.float64)
    if a.shape not in ((4, 4), (3, 4)):
        raise ValueError(f"fitting: the scan pose of image {img_id} must be 4 x 4 or 3 x 4, got {a.shape}")
    a = np.ascontiguousarray(a[:3, :4]).reshape(12)
    if not np.isfinite(a).all():
        raise ValueError(f"fitting: the scan pose of image {img_id} is not finite")
    return a


def fit_3d_segs_with_points3d_arrays(all_2d_segs, imagecols, p3d_reader, fitting_config=None, inloc_dataset=None,
                                     seed=0, max_chunk_bytes=1 << 30, scan_poses=None, options=None, device=0):
    """fit_3d_segs_with_points3d in array form: -> (dict img_id -> (M, 2, 3) float64, dict img_id -> dict(status (M,),
    stats (M, 5)), timers), like fit_3d_segs_arrays.  p3d_reader: img_id -> reader with read_p3ds(), or the (H, W, 3)
    scan itself (NumPy array or torch tensor).  inloc_dataset: the points go through hloc's
    get_scan_pose(inloc_dataset, image_name) instead of the camera (ImportError without hloc, as in the reference);
    scan_poses (img_id -> 4 x 4) gives the same transforms without hloc.  A sample outside hloc's (-1, 1) range (a scan
    smaller than the image) raises ValueError naming the image and the line."""
    if inloc_dataset is not None and scan_poses is not None:
        raise ValueError("fitting: give inloc_dataset or scan_poses, not both")
    ransac_th, min_pct, var2d = _fitting_args(fitting_config)
    cfg = _config(options, ransac_th, min_pct, var2d, seed)
    ids, cams, seg_off, allsegs = _scene_of(all_2d_segs, imagecols)
    sizes = [_view_size(imagecols.camview(i), i) for i in ids]
    for i in ids:
        if i not in p3d_reader:
            raise KeyError(f"fitting: no 3D points for image {i}")
    if inloc_dataset is not None:
        from hloc.localize_inloc import get_scan_pose
        scan_poses = {i: get_scan_pose(inloc_dataset, imagecols.image_name(i)) for i in ids}
    poses = None
    if scan_poses is not None:
        for i in ids:
            if i not in scan_poses:
                raise KeyError(f"fitting: no scan pose for image {i}")
        poses = np.ascontiguousarray(np.stack([_pose_rows(scan_poses[i], i) for i in ids])) if ids else None
    p = _capi.ptr

    def launch(ctx, n, maps, seg, status, stats):
        arr = (_capi.LtScanMap * len(maps))(*maps)
        pp = p(poses[n:], C.c_double) if poses is not None else None
        ctx.chk(ctx.L.lt_fit_scans(ctx.h, n, len(maps), arr, pp, C.byref(cfg), p(seg, C.c_double),
                                   p(status, C.c_int32), p(stats, C.c_int32)))

    seg, status, stats, timers = _fit_chunks(
        ids, cams, seg_off, allsegs, lambda m: _scan_of(_read_p3ds(p3d_reader[ids[m]]), sizes[m], device),
        _scan_nbytes, launch, max_chunk_bytes, device)
    bad = np.nonzero(status[:int(seg_off[-1])] == STATUS_SCAN_OUT_OF_RANGE)[0]
    if len(bad):
        j = int(np.searchsorted(seg_off, bad[0], side="right")) - 1
        raise ValueError(f"fitting: image {ids[j]} line {int(bad[0] - seg_off[j])}: a sample falls outside the scan "
                         "(interpolate_scan's -1 < kp < 1 assertion)")
    out, info = _per_image(ids, seg_off, seg, status, stats)
    return out, info, timers


def fit_3d_segs_with_points3d(all_2d_segs, imagecols, p3d_reader, fitting_config, inloc_dataset=None, seed=0,
                              max_chunk_bytes=1 << 30, scan_poses=None):
    """runners/line_fitnmerge.py:73-130: dict img_id -> list of (start, end) float64 (3,) arrays, zeros where the fit
    fails.  fitting_config["n_jobs"] is accepted and ignored."""
    arrs, _, _ = fit_3d_segs_with_points3d_arrays(all_2d_segs, imagecols, p3d_reader, fitting_config, inloc_dataset,
                                                  seed, max_chunk_bytes, scan_poses)
    return {i: [(a[0].copy(), a[1].copy()) for a in arrs[i]] for i in arrs}


def estimate_seg3d_from_points3d(seg2d, p3ds, camview, image_name, inloc_dataset=None, ransac_th=0.75,
                                 min_percentage_inliers=0.6, var2d=5.0, seed=0):
    """fitting.py:56-102 for one segment: None or (start, end).  camview must know its image size."""
    from .base import ImageCollection
    poses = None
    if inloc_dataset is not None:
        from hloc.localize_inloc import get_scan_pose
        poses = {0: get_scan_pose(inloc_dataset, image_name)}
    arrs, info, _ = fit_3d_segs_with_points3d_arrays(
        {0: np.asarray(seg2d, np.float64).reshape(1, -1)}, ImageCollection({0: camview}), {0: p3ds},
        dict(ransac_th=ransac_th, min_percentage_inliers=min_percentage_inliers, var2d=var2d), seed=seed,
        scan_poses=poses)
    if info[0]["status"][0] != STATUS_OK:
        return None
    return arrs[0][0, 0].copy(), arrs[0][0, 1].copy()


def tracks_from_fit(all_2d_segs, seg3d_list):
    """one LineTrack per 2D segment whose fitted 3D segment has a length > 0, in all_2d_segs' image order and line
    order (runners/line_fitnmerge.py:210-221 and :392-402); seg3d_list[img_id][line_id] is (start, end) or (2, 3)"""
    from .base import Line2d, Line3d, LineTrack
    tracks = []
    for img_id in all_2d_segs:
        for line_id, seg2d in enumerate(all_2d_segs[img_id]):
            seg3d = seg3d_list[img_id][line_id]
            l3d = Line3d(seg3d[0], seg3d[1])
            l2d = Line2d(seg2d[0:2], seg2d[2:4])
            if l3d.length() == 0:
                continue
            tracks.append(LineTrack(l3d, [img_id], [line_id], [l2d]))
    return tracks
