"""Mirror of the minimal-solver layer of `limap.estimators.absolute_pose`: the four solvers
`JointPoseEstimator::MinimalSolver` calls (p3p, p2p1ll, p1p2ll, p3ll) for batches of samples, on the device.

    poses, counts = estimators.minimal_solver("p2p1ll", xs, Xs, ls, Cs, Vs)        # (n, 8, 7), (n,)
    xs, Xs, ls, Cs, Vs = estimators.minimal_inputs(camera, p2ds, p3ds, l2ds, l3ds)  # as MinimalSolver builds them

All four solvers are one problem with one core (lt_est.h): the translation is eliminated by the
left null space of the constraint normals, the three remaining quadrics are solved in the chart w = 1 through an octic
whose real roots a Sturm chain isolates, and every pose gets a fixed Newton polish on its six constraints.  **The
arithmetic is this project's deterministic definition, which the device (k_est_minimal, one lane per sample) and the
host twin compute bit-identically; it is not PoseLib's.**  Poses are the solutions of the sample's constraints with
positive point depths, at most 8, with the quaternion normalised and w > 0.  Rotations at w = 0 are outside the chart:
such a sample, like a degenerate one, returns fewer poses or none, never a NaN pose.

`pl_estimate_absolute_pose` is the entry point of `limap.estimators`: `ransac.method: None` goes to
`optimize.pl_estimate_absolute_pose` unchanged; `"hybrid"` runs the hybrid LO-MSAC of
`pl_absolute_pose_hybrid_ransac.h` on the device by rounds (lt_est_loop.h): limap's control flow, score, thresholds,
weights, cheirality tests and refinements are restated, the sampler and `NumRequiredIterations` are this project's
seedable definition, and **poses are those of a hybrid LO-MSAC, not the iterates of a RansacLib run**.
`pl_estimate_absolute_pose_batch` localises any number of queries in one set of launches.  Not built, and refused by
name: `"ransac"` and `"solver"` (the single-threshold loop of `pl_absolute_pose_ransac.h`) and the `line3dpp` weight.

`host=True` (or `host_threads=N`) runs the documented host twin (lt_fn_est_minimal_host) instead of the device; it is a
request, never a fallback.
"""
import ctypes as C

import numpy as np

from . import _capi, _native
from . import hybrid_localization as _hl

__all__ = ["SOLVER_KINDS", "minimal_solver", "minimal_inputs", "pl_estimate_absolute_pose", "pl_estimate_absolute_pose_batch",
           "ExtendedHybridLORansacOptions", "HybridPoseEstimatorOptions", "HybridRansacStatistics",
           "EstimateAbsolutePose_PointLine_Hybrid", "hybrid_arrays", "TRACE_DOUBLES"]

SOLVER_KINDS = ("p3p", "p2p1ll", "p1p2ll", "p3ll")  # hybrid_pose_estimator.h: MinimalSolverType, kind = lines in a sample
MAX_SOLUTIONS = 8

_context = _capi.per_device_contexts()


def _kind(kind):
    if isinstance(kind, str):
        if kind.lower() not in SOLVER_KINDS:
            raise ValueError(f"limap_amd.estimators: unknown minimal solver {kind!r} (one of {', '.join(SOLVER_KINDS)})")
        return SOLVER_KINDS.index(kind.lower())
    if int(kind) not in range(4):
        raise ValueError(f"limap_amd.estimators: unknown minimal solver {kind!r}")
    return int(kind)


def _samples(a, n_items, what):
    if n_items == 0:
        return None, None
    a = np.ascontiguousarray(np.asarray(a, float))
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3 or a.shape[1:] != (n_items, 3):
        raise ValueError(f"limap_amd.estimators: {what} must have shape (n, {n_items}, 3), not {a.shape}")
    return a, len(a)


def minimal_solver(kind, xs=None, Xs=None, ls=None, Cs=None, Vs=None, host=False, host_threads=None, ctx=None,
                   return_timers=False):
    """n samples of one solver kind ("p3p", "p2p1ll", "p1p2ll", "p3ll" or 0..3 = lines per sample) in one launch.
    xs (unit bearings) and Xs (world points): (n, points, 3); ls (unit image-line normals), Cs (a point of the 3D line)
    and Vs (its unit direction): (n, lines, 3); one sample may be given without the leading axis.
    -> poses (n, 8, 7) rows (qvec w x y z, tvec), zeros past the count, and counts (n,)."""
    k = _kind(kind)
    npts, nl = 3 - k, k
    arrs, ns = [], set()
    for a, cnt, what in ((xs, npts, "xs"), (Xs, npts, "Xs"), (ls, nl, "ls"), (Cs, nl, "Cs"), (Vs, nl, "Vs")):
        if cnt and a is None:
            raise ValueError(f"limap_amd.estimators: {SOLVER_KINDS[k]} needs {what}")
        a, n = _samples(a, cnt, what)
        arrs.append(a)
        if n is not None:
            ns.add(n)
    if len(ns) != 1:
        raise ValueError(f"limap_amd.estimators: the sample arrays differ in length: {sorted(ns)}")
    n = ns.pop()
    poses = np.zeros((max(n, 1), MAX_SOLUTIONS, 7))
    counts = np.zeros(max(n, 1), np.int32)
    L = _capi.load_library()
    p = _capi.ptr
    args = (k, n) + tuple(p(a, C.c_double) if a is not None and len(a) else None for a in arrs)
    outs = (p(poses, C.c_double), p(counts, C.c_int32))
    ht = _native.host_threads(host, host_threads)
    timers = None
    if ht is not None:
        if L.lt_fn_est_minimal_host(*args, int(ht), *outs) != 0:
            _native.raise_host_error(L, "lt_fn_est_host_error", "limap_amd.estimators: ")
    else:
        ctx = ctx if ctx is not None else _context()
        ctx.chk(L.lt_est_minimal(ctx.h, *args))
        ctx.chk(L.lt_est_minimal_get(ctx.h, *outs))
        tm = ctx.module_timers("lt_est_minimal_get_timers", 4)
        timers = dict(prepare_ms=float(tm[0]), kernel_ms=float(tm[1]), download_ms=float(tm[2]), solve_device_ms=float(tm[3]))
    if return_timers:
        return poses[:n], counts[:n], timers
    return poses[:n], counts[:n]


def minimal_inputs(camera, p2ds=(), p3ds=(), l2ds=(), l3ds=()):
    """The solver inputs of correspondences as JointPoseEstimator::MinimalSolver builds them
    (joint_pose_estimator.cc:86-110): x = normalised K^-1 (p2d, 1), X = p3d; l = the normalised cross product of the
    normalised K^-1 (start, 1) and K^-1 (end, 1), C = l3d.start, V = the normalised direction of l3d.  `camera` is a K
    (3x3), a kvec (fx fy cx cy) or an object with K(); l3ds holds the 3D line of each l2d."""
    fx, fy, cx, cy = _hl._kvec(camera)

    def bearing(xy):
        v = np.array([(xy[0] - cx) / fx, (xy[1] - cy) / fy, 1.0])
        return v / np.linalg.norm(v)

    if len(p2ds) != len(p3ds) or len(l2ds) != len(l3ds):
        raise ValueError("limap_amd.estimators: p2ds / p3ds or l2ds / l3ds differ in length")
    xs = np.array([bearing(np.asarray(a, float).reshape(2)) for a in p2ds], float).reshape(-1, 3)
    Xs = np.array([np.asarray(a, float).reshape(3) for a in p3ds], float).reshape(-1, 3)
    ls, Cs, Vs = [], [], []
    for l2, l3 in zip(l2ds, l3ds):
        s, a3 = _hl._l2(l2), _hl._l3(l3)
        n = np.cross(bearing(s[:2]), bearing(s[2:]))
        d = a3[3:] - a3[:3]
        ls.append(n / np.linalg.norm(n)); Cs.append(a3[:3]); Vs.append(d / np.linalg.norm(d))
    arr = lambda v: np.array(v, float).reshape(-1, 3)  # noqa: E731
    return xs, Xs, arr(ls), arr(Cs), arr(Vs)


class ExtendedHybridLORansacOptions:
    """estimators/extended_hybrid_ransac.h over ransac_lib::HybridLORansacOptions, with RansacLib's defaults (the ones
    fitting.LORansacOptions states) and max_num_iterations_per_solver_"""

    def __init__(self):
        self.min_num_iterations_ = 100
        self.max_num_iterations_ = 10000
        self.max_num_iterations_per_solver_ = 10000
        self.success_probability_ = 0.9999
        self.squared_inlier_thresholds_ = [1.0, 1.0]
        self.data_type_weights_ = [1.0, 1.0]
        self.random_seed_ = 0
        self.num_lo_steps_ = 10
        self.threshold_multiplier_ = float(np.sqrt(2.0))
        self.num_lsq_iterations_ = 4
        self.min_sample_multiplicator_ = 7
        self.non_min_sample_multiplier_ = 3
        self.lo_starting_iterations_ = 50
        self.final_least_squares_ = False


class HybridPoseEstimatorOptions:
    """hybrid_pose_estimator.h:21-43.  `random` is False here (a fixed seed); True draws the seed on the host.
    round_size: iterations per round on the device (1: upstream's control flow exactly)."""

    def __init__(self):
        self.ransac_options = ExtendedHybridLORansacOptions()
        self.lineloc_config = _hl.LineLocConfig()
        self.lineloc_config.print_summary = False
        self.solver_flags = [True, True, True, True]
        self.cheirality_min_depth = 0.0
        self.cheirality_overlap_pixels = 10.0
        self.random = False
        self.round_size = 64

    def _struct(self):
        r = self.ransac_options
        if len(r.squared_inlier_thresholds_) != 2 or len(r.data_type_weights_) != 2:  # THROW_CHECK_EQ
            raise ValueError("limap_amd.estimators: squared_inlier_thresholds_ and data_type_weights_ take two values")
        if len(self.solver_flags) != 4:
            raise ValueError("limap_amd.estimators: solver_flags takes four values")
        c = _capi.LtEstConfig()
        _capi.load_library().lt_est_config_default(C.byref(c))
        for i in range(2):
            c.squared_inlier_thresholds[i] = float(r.squared_inlier_thresholds_[i])
            c.data_type_weights[i] = float(r.data_type_weights_[i])
        c.success_probability, c.threshold_multiplier = float(r.success_probability_), float(r.threshold_multiplier_)
        c.cheirality_min_depth, c.cheirality_overlap_pixels = float(self.cheirality_min_depth), float(self.cheirality_overlap_pixels)
        seed = int(np.random.SeedSequence().entropy % (1 << 63)) if self.random else int(r.random_seed_)
        c.random_seed = seed
        c.min_num_iterations, c.max_num_iterations = int(r.min_num_iterations_), int(r.max_num_iterations_)
        c.max_num_iterations_per_solver = int(r.max_num_iterations_per_solver_)
        c.lo_starting_iterations = int(r.lo_starting_iterations_)
        c.num_lo_steps, c.num_lsq_iterations = int(r.num_lo_steps_), int(r.num_lsq_iterations_)
        c.min_sample_multiplicator, c.non_min_sample_multiplier = int(r.min_sample_multiplicator_), int(r.non_min_sample_multiplier_)
        c.final_least_squares, c.round_size = int(bool(r.final_least_squares_)), int(self.round_size)
        for i in range(4):
            c.solver_flags[i] = int(bool(self.solver_flags[i]))
        c.loc = self.lineloc_config._struct()
        return c


class HybridRansacStatistics:
    """ransac_lib::HybridRansacStatistics; `ran` is VerifyData's answer, `trace` the loop's decision records"""

    def __init__(self, d, i, inl_pts, inl_lines, trace=None):
        self.best_model_score = float(d[0])
        self.inlier_ratios = [float(d[1]), float(d[2])]
        self.num_iterations_total = int(i[0])
        self.num_iterations_per_solver = [int(v) for v in i[1:5]]
        self.best_num_inliers = int(i[5])
        self.best_solver_type = int(i[6])
        self.number_lo_iterations = int(i[7])
        self.inlier_indices = [inl_pts, inl_lines]
        self.ran = bool(i[10])
        self.trace = trace


TRACE_DOUBLES = 12


def _query_arrays(queries):
    """queries: dicts with l3ds, l3d_ids, l2ds, p3ds, p2ds, camera (K, kvec or an object with K()) and optionally campose
    -> the CSR arrays of lt_est_solve"""
    Q = len(queries)
    k = np.zeros((max(Q, 1), 4)); q = np.tile([1.0, 0.0, 0.0, 0.0], (max(Q, 1), 1)); t = np.zeros((max(Q, 1), 3))
    pt_off, l3_off, sg_off = [0], [0], [0]
    p3, p2, l3, sg, ids = [], [], [], [], []
    for n, qr in enumerate(queries):
        k[n] = _hl._kvec(qr["camera"])
        pose = qr.get("campose")
        if pose is not None:
            q[n], t[n] = np.asarray(pose.qvec, float).reshape(4), np.asarray(pose.tvec, float).reshape(3)
        a3, a2 = qr.get("p3ds", ()), qr.get("p2ds", ())
        if len(a3) != len(a2) or len(qr.get("l3d_ids", ())) != len(qr.get("l2ds", ())):
            raise ValueError(f"limap_amd.estimators: query {n}: p3ds / p2ds or l3d_ids / l2ds differ in length")
        p3.extend(np.asarray(x, float).reshape(3) for x in a3)
        p2.extend(np.asarray(x, float).reshape(2) for x in a2)
        l3.extend(_hl._l3(x) for x in qr.get("l3ds", ()))
        sg.extend(_hl._l2(x) for x in qr.get("l2ds", ()))
        ids.extend(int(i) for i in qr.get("l3d_ids", ()))
        pt_off.append(len(p3)); l3_off.append(len(l3)); sg_off.append(len(sg))
    arr = lambda v, w: np.ascontiguousarray(np.array(v, float).reshape(-1, w)) if len(v) else np.zeros((1, w))  # noqa: E731
    i64 = lambda v: np.array(v, np.int64)  # noqa: E731
    return (Q, k, q, t, i64(pt_off), arr(p3, 3), arr(p2, 2), i64(l3_off), arr(l3, 6), i64(sg_off),
            np.ascontiguousarray(np.array(ids if ids else [0], np.int32)), arr(sg, 4))


def hybrid_arrays(csr, cfg_struct, host_threads=None, ctx=None, trace_cap=0):
    """One call of lt_est_solve (device) or lt_fn_est_host (host_threads given) -> dict of per-query arrays"""
    Q, k, q, t, pt_off, p3, p2, l3_off, l3, sg_off, ids, sg = csr
    L = _capi.load_library()
    p = _capi.ptr
    N = int(pt_off[-1] + sg_off[-1])
    pose = np.zeros((max(Q, 1), 7)); ds = np.zeros((max(Q, 1), 3)); it = np.zeros((max(Q, 1), 12), np.int32)
    inl = np.zeros(max(N, 1), np.int32); trace = np.zeros((max(Q, 1), max(trace_cap, 1), TRACE_DOUBLES))
    args = (Q, p(k), p(q), p(t), p(pt_off, C.c_int64), p(p3), p(p2), p(l3_off, C.c_int64), p(l3), p(sg_off, C.c_int64),
            p(ids, C.c_int32), p(sg), C.byref(cfg_struct), int(trace_cap))
    outs = (p(pose), p(ds), p(it, C.c_int32), p(inl, C.c_int32), p(trace) if trace_cap else None)
    timers = None
    if host_threads is not None:
        if L.lt_fn_est_host(*args, int(host_threads), *outs) != 0:
            _native.raise_host_error(L, "lt_fn_est_host_error", "limap_amd.estimators: ")
    else:
        ctx = ctx if ctx is not None else _context()
        ctx.chk(L.lt_est_solve(ctx.h, *args))
        ctx.chk(L.lt_est_get(ctx.h, *outs))
        tm = ctx.module_timers("lt_est_get_timers", 8)
        timers = dict(prepare_ms=float(tm[0]), rounds_ms=float(tm[1]), download_ms=float(tm[2]), rounds=int(tm[3]),
                      rounds_device_ms=float(tm[4]))
    stats = []
    for n in range(Q):
        c0, npt, nin = int(pt_off[n] + sg_off[n]), int(it[n, 8]), int(it[n, 8] + it[n, 9])
        tr = trace[n, :min(int(it[n, 11]), trace_cap)].copy() if trace_cap else None
        stats.append(HybridRansacStatistics(ds[n], it[n], inl[c0:c0 + npt].tolist(), inl[c0 + npt:c0 + nin].tolist(), tr))
    return dict(qvec=pose[:Q, :4], tvec=pose[:Q, 4:], stats=stats, dstats=ds[:Q], istats=it[:Q], inliers=inl[:N],
                trace=trace[:Q] if trace_cap else None, timers=timers)


def EstimateAbsolutePose_PointLine_Hybrid(l3ds, l3d_ids, l2ds, p3ds, p2ds, cam, options, campose=None, host=False,
                                          host_threads=None, trace_cap=0):
    """hybrid_pose_estimator.cc:14-42 -> (CameraPose, HybridRansacStatistics).  `campose` comes back where VerifyData
    finds no solver that can run (fewer than three correspondences, or every feasible solver switched off)."""
    res = hybrid_arrays(_query_arrays([dict(l3ds=l3ds, l3d_ids=l3d_ids, l2ds=l2ds, p3ds=p3ds, p2ds=p2ds, camera=cam,
                                            campose=campose)]), options._struct(),
                        _native.host_threads(host, host_threads), trace_cap=trace_cap)
    return _hl.CameraPose(res["qvec"][0], res["tvec"][0]), res["stats"][0]


def _hybrid_options(cfg, jointloc_cfg, seed):
    """_pl_estimate_absolute_pose.py:24-46,86-128"""
    if jointloc_cfg is None:
        jointloc_cfg = {}
        if cfg.get("optimize"):
            jointloc_cfg = dict(cfg["optimize"])
            name, args = jointloc_cfg.pop("loss_func"), jointloc_cfg.pop("loss_func_args", None) or []
            if name not in _hl._LOSSES:
                raise ValueError(f"limap_amd.estimators: loss_func {name!r} is not built")
            jointloc_cfg["loss_function"] = _hl._LOSSES[name](*([] if name == "TrivialLoss" else args))
        else:
            jointloc_cfg["loss_function"] = _hl.TrivialLoss()
    else:
        jointloc_cfg = dict(jointloc_cfg)
    if "line_weight" in cfg:
        jointloc_cfg["weight_point"] = 1.0
        jointloc_cfg["weight_line"] = cfg["line_weight"]
    rc = cfg["ransac"]
    options = HybridPoseEstimatorOptions()
    options.lineloc_config = _hl.LineLocConfig(jointloc_cfg)
    options.lineloc_config.cost_function = _hl.get_lineloc_cost_func(cfg["line_cost_func"])
    options.solver_flags = list(rc["solver_flags"])
    r = options.ransac_options
    r.squared_inlier_thresholds_ = [float(rc["thres_point"]) ** 2, float(rc["thres_line"]) ** 2]
    w = np.array([rc["weight_point"], rc["weight_line"]], float)
    w *= np.array([r.squared_inlier_thresholds_[1], r.squared_inlier_thresholds_[0]]) / np.sum(r.squared_inlier_thresholds_)
    r.data_type_weights_ = [float(w[0]), float(w[1])]
    r.min_num_iterations_ = int(rc["min_num_iterations"])
    r.final_least_squares_ = bool(rc["final_least_squares"])
    if "round_size" in rc:
        options.round_size = int(rc["round_size"])
    if seed is not None:
        r.random_seed_ = int(seed)
    return options


def _method(cfg):
    method = cfg["ransac"]["method"]
    if method in ("ransac", "solver"):
        raise NotImplementedError(f"limap_amd.estimators: ransac method {method!r} is not built (the single-threshold loop "
                                  "of pl_absolute_pose_ransac.h; None and \"hybrid\" are)")
    if method not in (None, "hybrid"):
        raise ValueError(f"limap_amd.estimators: unknown ransac method {method!r}")
    return method


def pl_estimate_absolute_pose(cfg, l3ds, l3d_ids, l2ds, p3ds, p2ds, camera, campose=None, inliers_line=None,
                              inliers_point=None, jointloc_cfg=None, silent=True, logger=None, host=False, seed=None):
    """estimators/absolute_pose/_pl_estimate_absolute_pose.py:9-147 -> (CameraPose, stats).  cfg["ransac"]["method"] None
    is the joint refinement of optimize.pl_estimate_absolute_pose, unchanged (stats None); "hybrid" is the hybrid
    LO-MSAC with the threshold-weighted data_type_weights_ of lines 114-128 (stats: HybridRansacStatistics); "ransac" and
    "solver" raise NotImplementedError naming the method.  seed: random_seed_ (default 0)."""
    if _method(cfg) is None:
        return _hl.pl_estimate_absolute_pose(cfg, l3ds, l3d_ids, l2ds, p3ds, p2ds, camera, campose=campose,
                                             inliers_line=inliers_line, inliers_point=inliers_point,
                                             jointloc_cfg=jointloc_cfg, silent=silent, logger=logger, host=host)
    options = _hybrid_options(cfg, jointloc_cfg, seed)
    return EstimateAbsolutePose_PointLine_Hybrid(l3ds, l3d_ids, l2ds, p3ds, p2ds, camera, options, campose=campose, host=host)


def pl_estimate_absolute_pose_batch(cfg, queries, jointloc_cfg=None, host=False, host_threads=None, seed=None, trace_cap=0):
    """Every query (dicts with l3ds, l3d_ids, l2ds, p3ds, p2ds, camera and optionally campose) under method "hybrid" in one
    set of launches -> list of (CameraPose, HybridRansacStatistics).  The draws of a query are keyed by its index."""
    if _method(cfg) is None:
        raise ValueError("limap_amd.estimators: the batch call is the hybrid estimator's (ransac.method: \"hybrid\")")
    res = hybrid_arrays(_query_arrays(queries), _hybrid_options(cfg, jointloc_cfg, seed)._struct(),
                        _native.host_threads(host, host_threads), trace_cap=trace_cap)
    return [(_hl.CameraPose(res["qvec"][n], res["tvec"][n]), res["stats"][n]) for n in range(len(queries))]
