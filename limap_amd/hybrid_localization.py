"""Mirror of `limap.optimize.hybrid_localization` (LineLocEngine, JointLocEngine, solve_jointloc) and of the
`ransac.method: null` path of `limap.estimators.pl_estimate_absolute_pose`: the refinement of one camera pose from 2D-3D
line and point correspondences, what runners/hybrid_localization.py runs per query.

    engine = optimize.solve_jointloc("PerpendicularDist", cfg, l3ds, l3d_ids, l2ds, p3ds, p2ds, K, R, T)
    pose = base-like CameraPose(engine.GetFinalQ(), engine.GetFinalT())

Every problem is a 6-degree-of-freedom robust least-squares problem; `solve_jointloc_batch` runs any number of them in
one launch of the HIP kernel of lt_kernels_loc.hip, one wave per problem.  limap's cost functions,
weights, losses, block order and block weights are restated; **the minimiser is this project's deterministic
Levenberg-Marquardt definition: refined poses are minimisers of upstream's cost, not the iterates of a particular Ceres
run.**

Not built, and rejected by name: the ELine3dppWeight ("line3dpp": it needs an arccosine), solver options that would
change the minimiser, and every `ransac.method` other than None (PoseLib's minimal solvers and RansacLib's loops).

`host=True` (or `host_threads=N`) runs the documented host path (lt_fn_loc_host: the same inline functions in plain
C++, bit-identical results) instead of the device; it is a request, never a fallback.
"""
import ctypes as C
from collections import defaultdict

import numpy as np

from . import _capi, _native

__all__ = ["LineLocConfig", "TrivialLoss", "HuberLoss", "SoftLOneLoss", "CauchyLoss", "LineLocCostFunction",
           "LineLocCostFunctionWeight", "get_lineloc_cost_func", "get_lineloc_weight_func", "get_line_pairs",
           "LineLocEngine", "JointLocEngine", "solve_lineloc_merged", "solve_jointloc_merged", "solve_jointloc",
           "solve_lineloc", "solve_jointloc_batch", "score_poses", "pl_estimate_absolute_pose", "CameraPose", "LOC_TERMINATION"]

# optimize/hybrid_localization/functions.py lives in this package upstream: the 2D-3D matching of limap_amd.localization
# is re-exported from here, on first use (that module imports this one)
_FUNCTIONS = ("match_line_2to2_epipolarIoU", "filter_line_2to2_epipolarIoU", "match_line_2to3", "midpoint_dist",
              "midpoint_perpendicular_dist", "perpendicular_dist", "get_reprojection_dist_func",
              "reprojection_filter_matches_2to3")
__all__ += list(_FUNCTIONS)


def __getattr__(name):
    if name in _FUNCTIONS:
        from . import localization
        return getattr(localization, name)
    raise AttributeError(name)

LOC_TERMINATION = {0: "max_num_iterations", 1: "radius", 2: "zero_gradient", 3: "pivot", 4: "model_decrease",
                   6: "evaluation_failed", 7: "no_residuals"}


class LineLocCostFunction:
    """hybrid_localization_config.h:18-25"""
    E2DMidpointDist2, E2DMidpointAngleDist3, E2DPerpendicularDist2, E2DPerpendicularDist4 = 0, 1, 2, 3
    E3DLineLineDist2, E3DPlaneLineDist2 = 4, 5


class LineLocCostFunctionWeight:
    """hybrid_localization_config.h:27-33"""
    ENoneWeight, ECosineWeight, ELine3dppWeight, ELengthWeight, EInvLengthWeight = 0, 1, 2, 3, 4


class _Loss:
    code, n_args = 0, 0

    def __init__(self, *args):
        if len(args) != self.n_args:
            raise TypeError(f"{type(self).__name__} takes {self.n_args} argument(s)")
        self.a = float(args[0]) if args else 1.0
        if args and not (self.a > 0.0 and np.isfinite(self.a)):
            raise ValueError(f"limap_amd.optimize: {type(self).__name__}({args[0]!r}): the parameter must be > 0")

    def __repr__(self):
        return f"{type(self).__name__}({self.a})" if self.n_args else f"{type(self).__name__}()"


class TrivialLoss(_Loss):
    code, n_args = 0, 0


class HuberLoss(_Loss):
    code, n_args = 1, 1


class SoftLOneLoss(_Loss):
    code, n_args = 2, 1


class CauchyLoss(_Loss):
    code, n_args = 3, 1


_LOSSES = {c.__name__: c for c in (TrivialLoss, HuberLoss, SoftLOneLoss, CauchyLoss)}
# solver_options keys that only log or print, or that cannot change a dense 6-unknown solve
_IGNORED_SOLVER_KEYS = {"minimizer_progress_to_stdout", "logging_type", "num_threads", "num_linear_solver_threads",
                        "max_linear_solver_iterations", "update_state_every_iteration", "check_gradients",
                        "max_num_consecutive_invalid_steps", "max_consecutive_nonmonotonic_steps"}
_ZERO_TOLERANCES = ("function_tolerance", "gradient_tolerance", "parameter_tolerance")


class LineLocConfig:
    """hybrid_localization_config.h:35-78: weight_line, weight_point, print_summary, loss_function, solver_options
    (ASSIGN_PYDICT_ITEM: a present key overrides, unknown keys are ignored); cost_function and cost_function_weight are
    attributes the solve functions set."""

    def __init__(self, cfg=None):
        self.weight_line, self.weight_point, self.print_summary = 1.0, 1.0, True
        self.loss_function = TrivialLoss()
        self.max_num_iterations = 100
        self.cost_function = LineLocCostFunction.E2DPerpendicularDist2
        self.cost_function_weight = LineLocCostFunctionWeight.ENoneWeight
        if cfg is None:
            return
        if not isinstance(cfg, dict):
            raise TypeError("the configuration must be a dict")
        if "weight_line" in cfg:
            self.weight_line = float(cfg["weight_line"])
        if "weight_point" in cfg:
            self.weight_point = float(cfg["weight_point"])
        if "print_summary" in cfg:
            self.print_summary = bool(cfg["print_summary"])
        if "loss_function" in cfg:
            if not isinstance(cfg["loss_function"], _Loss):
                raise TypeError("loss_function must be a TrivialLoss, HuberLoss, SoftLOneLoss or CauchyLoss")
            self.loss_function = cfg["loss_function"]
        for k, v in (cfg.get("solver_options") or {}).items():
            if k == "max_num_iterations":
                self.max_num_iterations = int(v)
            elif k in _ZERO_TOLERANCES:
                if float(v) != 0.0:
                    raise ValueError(f"limap_amd.optimize: solver_options[{k!r}] must be 0 (the minimiser has no tolerances)")
            elif k not in _IGNORED_SOLVER_KEYS:
                raise ValueError(f"limap_amd.optimize: solver_options[{k!r}] would change the minimiser and is not built")

    def _struct(self):
        if self.cost_function_weight == LineLocCostFunctionWeight.ELine3dppWeight:
            raise ValueError("limap_amd.optimize: the ELine3dppWeight (line3dpp) is not built: it needs an arccosine")
        c = _capi.LtLocConfig()
        _capi.load_library().lt_loc_config_default(C.byref(c))
        c.cost_function, c.weight_function = int(self.cost_function), int(self.cost_function_weight)
        c.loss, c.loss_a = int(self.loss_function.code), float(self.loss_function.a)
        c.max_num_iterations = int(self.max_num_iterations)
        c.weight_line, c.weight_point = float(self.weight_line), float(self.weight_point)
        return c


def get_lineloc_cost_func(func_name):
    """optimize/hybrid_localization/solve.py:6-35"""
    F = LineLocCostFunction
    if func_name in ["MidpointDist", "MidpointDist2", "2DMidpointDist", "2DMidpointDist2"]:
        return F.E2DMidpointDist2
    if func_name in ["MidpointAngle", "MidpointAngleDist", "2DMidpointAngleDist"]:
        return F.E2DMidpointAngleDist3
    if func_name in ["PerpendicularDist", "PerpendicularDist2", "2DPerpendicularDist", "2DPerpendicularDist2"]:
        return F.E2DPerpendicularDist2
    if func_name in ["PerpendicularDist4", "2DPerpendicularDist4"]:
        return F.E2DPerpendicularDist4
    if func_name in ["3DLineLineDist", "3DLineLineDist2"]:
        return F.E3DLineLineDist2
    if func_name in ["3DPlaneLineDist", "3DPlaneLineDist2"]:
        return F.E3DPlaneLineDist2
    raise ValueError(f"[Error] Unknown line localization cost function: {func_name}")


def get_lineloc_weight_func(func_name):
    """optimize/hybrid_localization/solve.py:38-52"""
    W = LineLocCostFunctionWeight
    if func_name is None:
        return W.ENoneWeight
    name = func_name.lower()
    table = {"cosine": W.ECosineWeight, "line3dpp": W.ELine3dppWeight, "length": W.ELengthWeight,
             "invlength": W.EInvLengthWeight}
    if name not in table:
        raise ValueError(f"[Error] Unknown line localization weight function: {func_name}")
    return table[name]


def get_line_pairs(l3ds, l3d_ids, l2ds):
    """solve.py:55-65: the 2D lines grouped by 3D line, groups in the order their 3D line first appears"""
    n = len(l3ds)
    merged = defaultdict(list)
    for l2d, l3d_id in zip(l2ds, l3d_ids):
        i = int(l3d_id)
        if not 0 <= i < n:
            raise ValueError(f"limap_amd.optimize: l3d_id {i} is outside the {n} 3D lines")
        merged[i].append(l2d)
    return [merged[i] for i in merged], [l3ds[i] for i in merged]


def _l3(l):
    return l.as_array().reshape(6) if hasattr(l, "as_array") else np.asarray(l, float).reshape(6)


def _l2(l):
    return l.as_array().reshape(4) if hasattr(l, "as_array") else np.asarray(l, float).reshape(4)


def _kvec(K):
    K = np.asarray(K.K() if hasattr(K, "K") else K, float)
    if K.shape == (3, 3):
        return np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])
    return K.reshape(4)


def _qvec_from_R(R):
    R = np.ascontiguousarray(np.asarray(R, float).reshape(9))
    q = np.zeros(4)
    if _capi.load_library().lt_fn_loc_qvec_from_R(_capi.ptr(R, C.c_double), _capi.ptr(q, C.c_double)) != 0:
        raise ValueError("limap_amd.optimize: non-finite rotation matrix")
    return q


def _rotation(q):
    """CameraPose::R(): QuaternionToRotationMatrix of the normalised quaternion (pose.cc:12-28)"""
    w, x, y, z = np.asarray(q, float) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


class CameraPose:
    """base/camera.h:84-113 reduced to what the localization returns"""

    def __init__(self, qvec, tvec):
        q = np.asarray(qvec, float).reshape(-1)
        if q.size == 9:
            q = _qvec_from_R(q)
        self.qvec = q / np.linalg.norm(q)
        self.tvec = np.asarray(tvec, float).reshape(3).copy()

    def R(self):
        return _rotation(self.qvec)

    def T(self):
        return self.tvec

    def center(self):
        return -self.R().T @ self.tvec


_context = _capi.per_device_contexts()


def _problem_arrays(problems):
    """problems: dicts with l3ds (3D lines), l2ds (per 3D line its 2D lines), p3ds, p2ds, kvec, qvec, tvec -> CSR"""
    P = len(problems)
    k = np.zeros((max(P, 1), 4)); q = np.zeros((max(P, 1), 4)); t = np.zeros((max(P, 1), 3))
    line_off, pt_off, seg_off = [0], [0], [0]
    l3, sg, p3, p2 = [], [], [], []
    for n, pr in enumerate(problems):
        k[n], q[n], t[n] = pr["kvec"], pr["qvec"], pr["tvec"]
        l3ds, l2ds = pr.get("l3ds", ()), pr.get("l2ds", ())
        if len(l3ds) != len(l2ds):
            raise ValueError(f"problem {n}: {len(l3ds)} 3D lines and {len(l2ds)} groups of 2D lines")  # CHECK_EQ
        for a, group in zip(l3ds, l2ds):
            l3.append(_l3(a))
            sg.extend(_l2(s) for s in group)
            seg_off.append(len(sg))
        line_off.append(len(l3))
        a3, a2 = pr.get("p3ds", ()), pr.get("p2ds", ())
        if len(a3) != len(a2):
            raise ValueError(f"problem {n}: {len(a3)} 3D points and {len(a2)} 2D points")  # CHECK_EQ
        p3.extend(np.asarray(x, float).reshape(3) for x in a3)
        p2.extend(np.asarray(x, float).reshape(2) for x in a2)
        pt_off.append(len(p3))
    arr = lambda v, w: np.ascontiguousarray(np.array(v, float).reshape(-1, w)) if len(v) else np.zeros((1, w))  # noqa: E731
    return (P, k, q, t, np.array(line_off, np.int64), arr(l3, 6), np.array(seg_off, np.int64), arr(sg, 4),
            np.array(pt_off, np.int64), arr(p3, 3), arr(p2, 2))


def loc_arrays(csr, cfg_struct, host_threads=None, ctx=None):
    """One call of lt_loc_solve (device) or lt_fn_loc_host (host_threads given) -> dict of per-problem results"""
    P, k, q, t, line_off, l3, seg_off, sg, pt_off, p3, p2 = csr
    L = _capi.load_library()
    p = _capi.ptr
    Q = np.zeros((max(P, 1), 4)); T = np.zeros((max(P, 1), 3)); cost = np.zeros((max(P, 1), 2))
    nres = np.zeros(max(P, 1), np.int32); it = np.zeros(max(P, 1), np.int32); code = np.zeros(max(P, 1), np.int32)
    args = (P, p(k, C.c_double), p(q, C.c_double), p(t, C.c_double), p(line_off, C.c_int64), p(l3, C.c_double),
            p(seg_off, C.c_int64), p(sg, C.c_double), p(pt_off, C.c_int64), p(p3, C.c_double), p(p2, C.c_double),
            C.byref(cfg_struct))
    outs = (p(Q, C.c_double), p(T, C.c_double), p(cost, C.c_double), p(nres, C.c_int32), p(it, C.c_int32),
            p(code, C.c_int32))
    timers = None
    if host_threads is not None:
        if L.lt_fn_loc_host(*args, int(host_threads), *outs) != 0:
            _native.raise_host_error(L, "lt_fn_loc_host_error", "limap_amd.optimize: ")
    else:
        ctx = ctx if ctx is not None else _context()
        ctx.chk(L.lt_loc_solve(ctx.h, *args))
        ctx.chk(L.lt_loc_get(ctx.h, *outs))
        tm = ctx.module_timers("lt_loc_get_timers", 4)
        timers = dict(prepare_ms=float(tm[0]), kernel_ms=float(tm[1]), download_ms=float(tm[2]), lm_device_ms=float(tm[3]))
    return dict(qvec=Q[:P], tvec=T[:P], cost=cost[:P], num_residuals=nres[:P], iterations=it[:P], codes=code[:P],
                timers=timers)


def loc_eval(cfg_struct, problem):
    """lt_fn_loc_eval: residuals (blocks, 4), cost, g (6), H (6, 6) of one problem at its pose (tests)"""
    P, k, q, t, line_off, l3, seg_off, sg, pt_off, p3, p2 = _problem_arrays([problem])
    nb = int(seg_off[-1] + pt_off[-1])
    res = np.zeros((max(nb, 1), 4)); cost = np.zeros(1); g = np.zeros(6); H = np.zeros((6, 6))
    L = _capi.load_library()
    p = _capi.ptr
    rc = L.lt_fn_loc_eval(p(k, C.c_double), p(q, C.c_double), p(t, C.c_double), int(line_off[-1]), p(l3, C.c_double),
                          p(seg_off, C.c_int64), p(sg, C.c_double), int(pt_off[-1]), p(p3, C.c_double), p(p2, C.c_double),
                          C.byref(cfg_struct), p(res, C.c_double), p(cost, C.c_double), p(g, C.c_double), p(H, C.c_double))
    if rc != 0:
        _native.raise_host_error(L, "lt_fn_loc_host_error", "limap_amd.optimize: ")
    return res[:nb], float(cost[0]), g, H


class LineLocEngine:
    """hybrid_localization.h:21-83.  JointLocEngine without points and without weight_line."""
    _joint = False

    def __init__(self, cfg=None, host=False, host_threads=None):
        self.config = cfg if isinstance(cfg, LineLocConfig) else LineLocConfig(cfg)
        self._ht = _native.host_threads(host, host_threads)
        self._problem = self._result = None

    def _pose(self, K, R, T):
        K, R = np.asarray(K, float), np.asarray(R, float)
        kvec = _kvec(K)
        qvec = _qvec_from_R(R) if R.size == 9 else R.reshape(4)  # Initialize(..., K, R, T) / (..., kvec, qvec, tvec)
        return dict(kvec=kvec, qvec=qvec, tvec=np.asarray(T, float).reshape(3))

    def Initialize(self, l3ds, l2ds, K, R, T):
        if len(l3ds) != len(l2ds):
            raise ValueError(f"{len(l3ds)} 3D lines and {len(l2ds)} groups of 2D lines")
        self._problem = dict(self._pose(K, R, T), l3ds=list(l3ds), l2ds=[list(g) for g in l2ds], p3ds=[], p2ds=[])
        self._result = None

    def SetUp(self):
        if self._problem is None:
            raise RuntimeError("Initialize first")

    def _struct(self):
        c = self.config._struct()
        if not self._joint:
            c.weight_line = 1.0
        return c

    def Solve(self):
        self.SetUp()
        self._result = loc_arrays(_problem_arrays([self._problem]), self._struct(), self._ht)
        return int(self._result["codes"][0]) != 7  # false where the problem has no residuals

    def result(self):
        if self._result is None:
            raise RuntimeError("Solve first")
        return self._result

    def GetFinalQ(self):
        return self.result()["qvec"][0].copy()

    def GetFinalT(self):
        return self.result()["tvec"][0].copy()

    def GetFinalR(self):
        return _rotation(self.GetFinalQ())

    def _cost(self, k):
        r = self.result()
        return float(np.sqrt(r["cost"][0, k] / r["num_residuals"][0])) if r["num_residuals"][0] else float("nan")

    def GetInitialCost(self):
        return self._cost(0)

    def GetFinalCost(self):
        return self._cost(1)

    def IsSolutionUsable(self):
        return int(self.result()["codes"][0]) in (0, 1, 2)


class JointLocEngine(LineLocEngine):
    """hybrid_localization.h:85-126"""
    _joint = True

    def Initialize(self, l3ds, l2ds, p3ds, p2ds, K, R, T):
        if len(p3ds) != len(p2ds):
            raise ValueError(f"{len(p3ds)} 3D points and {len(p2ds)} 2D points")
        super().Initialize(l3ds, l2ds, K, R, T)
        self._problem.update(p3ds=list(p3ds), p2ds=list(p2ds))


def _config(cfg, cost_func, weight_func):
    c = LineLocConfig(cfg if cfg is not None else {})
    c.cost_function = get_lineloc_cost_func(cost_func)
    c.cost_function_weight = get_lineloc_weight_func(weight_func)
    return c


def solve_lineloc_merged(cost_func, lineloc_cfg, line_pairs, K, R, T, weight_func=None, silent=False, host=False):
    """solve.py:68-96"""
    l2ds, l3ds = line_pairs
    engine = LineLocEngine(_config(lineloc_cfg, cost_func, weight_func), host=host)
    engine.Initialize(l3ds, l2ds, K, R, T)
    engine.SetUp()
    engine.Solve()
    return engine


def solve_lineloc(cost_func, l3ds, l3d_ids, l2ds, K, R, T, line_weight_func=None, silent=False, lineloc_cfg=None,
                  host=False):
    """solve.py:99-105 as it is evidently meant: upstream passes its arguments to solve_lineloc_merged shifted by one
    (line_pairs lands in lineloc_cfg), which cannot run; here the pairs go where solve_lineloc_merged expects them and
    the configuration is an optional keyword."""
    return solve_lineloc_merged(cost_func, lineloc_cfg, get_line_pairs(l3ds, l3d_ids, l2ds), K, R, T, line_weight_func,
                                silent, host=host)


def solve_jointloc_merged(line_cost_func, jointloc_cfg, line_pairs, point_pairs, K, R, T, line_weight_func=None,
                          silent=False, host=False):
    """solve.py:108-146"""
    p2ds, p3ds = point_pairs
    l2ds, l3ds = line_pairs
    engine = JointLocEngine(_config(jointloc_cfg, line_cost_func, line_weight_func), host=host)
    engine.Initialize(l3ds, l2ds, p3ds, p2ds, K, R, T)
    engine.SetUp()
    engine.Solve()
    return engine


def solve_jointloc(line_cost_func, jointloc_cfg, l3ds, l3d_ids, l2ds, p3ds, p2ds, K, R, T, line_weight_func=None,
                   silent=False, host=False):
    """solve.py:149-175"""
    return solve_jointloc_merged(line_cost_func, jointloc_cfg, get_line_pairs(l3ds, l3d_ids, l2ds), (p2ds, p3ds), K, R, T,
                                 line_weight_func, silent, host=host)


def solve_jointloc_batch(line_cost_func, cfg, problems, line_weight_func=None, host=False, host_threads=None):
    """All `problems` in one set of launches.  A problem is a dict with l3ds, l3d_ids, l2ds (as solve_jointloc takes
    them) or l3ds, l2ds already merged (`merged=True`), p3ds, p2ds, K (3x3, kvec or a camera) and the initial pose as
    R (3x3) or qvec, and T or tvec.  Returns per-problem arrays: qvec, tvec, cost (initial, final: 1/2 sum rho),
    num_residuals, iterations, codes (LOC_TERMINATION), and the timers of the call."""
    c = _config(cfg, line_cost_func, line_weight_func)
    plist = []
    for pr in problems:
        if pr.get("merged"):
            l3ds, l2ds = pr.get("l3ds", []), pr.get("l2ds", [])
        else:
            l2ds, l3ds = get_line_pairs(pr.get("l3ds", []), pr.get("l3d_ids", []), pr.get("l2ds", []))
        q = pr["qvec"] if "qvec" in pr else _qvec_from_R(pr["R"])
        plist.append(dict(l3ds=l3ds, l2ds=l2ds, p3ds=pr.get("p3ds", []), p2ds=pr.get("p2ds", []), kvec=_kvec(pr["K"]),
                          qvec=np.asarray(q, float).reshape(4), tvec=np.asarray(pr.get("tvec", pr.get("T")), float).reshape(3)))
    return loc_arrays(_problem_arrays(plist), c._struct(), _native.host_threads(host, host_threads))


def _pose_arrays(poses):
    """(H, 7) rows (qvec, tvec), or a sequence of CameraPose-like objects / (qvec, tvec) pairs"""
    if isinstance(poses, np.ndarray):
        a = np.asarray(poses, float).reshape(-1, 7)
        return np.ascontiguousarray(a[:, :4]), np.ascontiguousarray(a[:, 4:])
    q = [np.asarray(p.qvec if hasattr(p, "qvec") else p[0], float).reshape(4) for p in poses]
    t = [np.asarray(p.tvec if hasattr(p, "tvec") else p[1], float).reshape(3) for p in poses]
    return (np.ascontiguousarray(np.array(q, float).reshape(-1, 4)), np.ascontiguousarray(np.array(t, float).reshape(-1, 3)))


def score_poses(line_cost_func, l3ds, l3d_ids, l2ds, p3ds, p2ds, K, poses, cheirality_min_depth=0.0,
                cheirality_overlap_pixels=10.0, thresholds=None, weights=None, host=False, host_threads=None, ctx=None):
    """JointPoseEstimator::EvaluateModelOnPoint (joint_pose_estimator.cc:176-251) for every pose x every correspondence
    in one launch: `residuals` (H, n_points + n_lines), the points first, DBL_MAX where a cheirality test fails.
    thresholds = (point, line) squared inlier thresholds (squared_inlier_thresholds_) asks for the MSAC score per pose,
    `scores` = sum min(r2, threshold) weight with weights = data_type_weights_ (1, 1 by default), and the inlier counts
    `inliers` (H, 2).  E2DMidpointAngleDist3 is an error, as upstream throws."""
    cost = get_lineloc_cost_func(line_cost_func)
    if cost == LineLocCostFunction.E2DMidpointAngleDist3:
        raise ValueError("limap_amd.optimize: E2DMidpointAngleDist3 is not compatible with scoring (upstream throws)")
    arr = lambda v, f, w: (np.ascontiguousarray(np.array([f(x) for x in v], float).reshape(-1, w)) if len(v)  # noqa: E731
                           else np.zeros((1, w)))
    l3 = arr(l3ds, _l3, 6); sg = arr(l2ds, _l2, 4)
    p3 = arr(p3ds, lambda x: np.asarray(x, float).reshape(3), 3); p2 = arr(p2ds, lambda x: np.asarray(x, float).reshape(2), 2)
    if len(l3d_ids) != len(l2ds) or len(p3ds) != len(p2ds):
        raise ValueError("limap_amd.optimize: l3d_ids / l2ds or p3ds / p2ds differ in length")
    ids = np.ascontiguousarray(np.asarray(l3d_ids, np.int64).reshape(-1))
    if len(ids) and (ids.min() < 0 or ids.max() >= len(l3ds)):
        bad = int(ids[(ids < 0) | (ids >= len(l3ds))][0])
        raise ValueError(f"limap_amd.optimize: l3d_id {bad} is outside the {len(l3ds)} 3D lines")
    ids = np.ascontiguousarray(ids.astype(np.int32)) if len(ids) else np.zeros(1, np.int32)
    q, t = _pose_arrays(poses)
    H, N = len(q), len(p3ds) + len(l2ds)
    c = _capi.LtLocScoreConfig()
    c.cost_function, c.want_msac = int(cost), int(thresholds is not None)
    c.cheirality_min_depth, c.cheirality_overlap_pixels = float(cheirality_min_depth), float(cheirality_overlap_pixels)
    th = (0.0, 0.0) if thresholds is None else thresholds
    wt = (1.0, 1.0) if weights is None else weights
    for i in range(2):
        c.squared_thresholds[i], c.weights[i] = float(th[i]), float(wt[i])
    kvec = np.ascontiguousarray(_kvec(K))
    L = _capi.load_library()
    p = _capi.ptr
    table = np.zeros((max(H, 1), max(N, 1))); scores = np.zeros(max(H, 1)); inl = np.zeros((max(H, 1), 2), np.int32)
    if H == 0:
        q, t = np.zeros((1, 4)), np.zeros((1, 3))
    args = (p(kvec, C.c_double), len(l3ds), p(l3, C.c_double), len(l2ds), p(ids, C.c_int32), p(sg, C.c_double), len(p3ds),
            p(p3, C.c_double), p(p2, C.c_double), H, p(q, C.c_double), p(t, C.c_double), C.byref(c))
    msac = thresholds is not None
    outs = (p(table, C.c_double), p(scores, C.c_double) if msac else None, p(inl, C.c_int32) if msac else None)
    ht = _native.host_threads(host, host_threads)
    timers = None
    if ht is not None:
        if L.lt_fn_loc_score_host(*args, int(ht), *outs) != 0:
            _native.raise_host_error(L, "lt_fn_loc_host_error", "limap_amd.optimize: ")
    else:
        ctx = ctx if ctx is not None else _context()
        ctx.chk(L.lt_loc_score(ctx.h, *args))
        ctx.chk(L.lt_loc_score_get(ctx.h, *outs))
        tm = ctx.module_timers("lt_loc_score_get_timers", 4)
        timers = dict(prepare_ms=float(tm[0]), kernel_ms=float(tm[1]), download_ms=float(tm[2]), score_device_ms=float(tm[3]))
    table = table.reshape(-1)[:H * N].reshape(H, N)
    return dict(residuals=table, scores=scores[:H] if msac else None, inliers=inl[:H] if msac else None, timers=timers)


def pl_estimate_absolute_pose(cfg, l3ds, l3d_ids, l2ds, p3ds, p2ds, camera, campose=None, inliers_line=None,
                              inliers_point=None, jointloc_cfg=None, silent=True, logger=None, host=False):
    """estimators/absolute_pose/_pl_estimate_absolute_pose.py:9-84 for cfg["ransac"]["method"] is None: one joint
    refinement from `campose` over the inlier correspondences -> (CameraPose, None)."""
    method = cfg["ransac"]["method"]
    if method is not None:
        raise NotImplementedError(f"limap_amd.optimize: ransac method {method!r} is not built (only None: the minimal "
                                  "solvers and the RANSAC loops are PoseLib's and RansacLib's)")
    if campose is None:
        raise ValueError("limap_amd.optimize: the refinement needs an initial campose")
    if jointloc_cfg is None:
        jointloc_cfg = {}
        if cfg.get("optimize"):
            jointloc_cfg = dict(cfg["optimize"])
            name, args = jointloc_cfg.pop("loss_func"), jointloc_cfg.pop("loss_func_args", None) or []
            if name not in _LOSSES:
                raise ValueError(f"limap_amd.optimize: loss_func {name!r} is not built")
            jointloc_cfg["loss_function"] = _LOSSES[name](*([] if name == "TrivialLoss" else args))
        else:
            jointloc_cfg["loss_function"] = TrivialLoss()
    else:
        jointloc_cfg = dict(jointloc_cfg)
    if "line_weight" in cfg:
        jointloc_cfg["weight_point"] = 1.0
        jointloc_cfg["weight_line"] = cfg["line_weight"]
    if inliers_point is not None:
        idx = np.arange(len(p2ds))[np.asarray(inliers_point)]
        p2ds, p3ds = [p2ds[i] for i in idx], [p3ds[i] for i in idx]
    if inliers_line is not None:
        idx = np.arange(len(l3d_ids))[np.asarray(inliers_line)]
        l3d_ids, l2ds = [l3d_ids[i] for i in idx], [l2ds[i] for i in idx]
    engine = solve_jointloc(cfg["line_cost_func"], jointloc_cfg, l3ds, l3d_ids, l2ds, p3ds, p2ds, _kvec(camera),
                            campose.R(), campose.T(), silent=silent, host=host)
    return CameraPose(engine.GetFinalQ(), engine.GetFinalT()), None
