"""NumPy restatement of limap's point-line pose refinement cost, written from the formulas in
upstream's operation order and parameterised on the dtype (float64, longdouble).  Paths relative to src/limap:

    ceresbase/point_projection.h:8-57                           cam_from_img, img_from_cam, pixel_to_world, world_to_pixel
    ceresbase/line_dists.h:8-28                                 sine2d, cosine2d
    optimize/hybrid_localization/cost_functions.h:29-194        weight2d and the six distances
    optimize/hybrid_localization/cost_functions.h:204-347       line_residual, point_residual
    optimize/hybrid_localization/hybrid_localization.cc:91-134  blocks(): order and ScaledLoss weights

Ceres' QuaternionRotatePoint, Eigen's q.conjugate() * v and Ceres' four losses are the published procedures.  Derivatives
come from tests/refine_oracle.py's dual numbers (four directions): a linearisation runs twice, over the directions
(rot 0, rot 1, rot 2, t 0) and (t 1, t 2, -, -) of the project's retraction q+ = normalize((1, dq) (x) q), t+ = t + dt;
d|x|/dx = +1 at 0, derivative 0 at a clamp.  With plain arrays in place of scalars the same expressions evaluate all
blocks at once (cost_only, for scipy).
"""
import numpy as np

from refine_oracle import Dual, _abs, _exp, _sqrt, val

EPS = 1e-12
E8 = 1e-8
COSTS = ("MidpointDist2", "MidpointAngleDist3", "PerpendicularDist2", "PerpendicularDist4", "LineLineDist2", "PlaneLineDist2")
WEIGHTS = {"none": 0, "cosine": 1, "length": 3, "invlength": 4}
LOSSES = ("trivial", "huber", "softlone", "cauchy")


def _clamp1(x, dtype):
    if isinstance(x, Dual):
        return Dual(1, None, x.dtype) if x.v > 1 else x
    return np.minimum(x, 1)


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def rotate_ceres(q, p):
    """ceres::QuaternionRotatePoint"""
    scale = 1 / _sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    u = [scale * x for x in q]
    uv = [u[2] * p[2] - u[3] * p[1], u[3] * p[0] - u[1] * p[2], u[1] * p[1] - u[2] * p[0]]
    uv = [x + x for x in uv]
    r = [p[i] + u[0] * uv[i] for i in range(3)]
    r[0] = r[0] + (u[2] * uv[2] - u[3] * uv[1])
    r[1] = r[1] + (u[3] * uv[0] - u[1] * uv[2])
    r[2] = r[2] + (u[1] * uv[1] - u[2] * uv[0])
    return r


def world_to_pixel(k, q, t, xyz):
    p = rotate_ceres(q, xyz)
    p = [p[i] + t[i] for i in range(3)]
    u, v = p[0] / p[2], p[1] / p[2]
    return [k[0] * u + k[2], k[1] * v + k[3]]


def pixel_to_world(k, q, t, x, y, depth):
    u, v = (x - k[2]) / k[0], (y - k[3]) / k[1]
    loc = [u * depth - t[0], v * depth - t[1], 1 * depth - t[2]]
    vec = [-q[1], -q[2], -q[3]]  # Eigen: conjugate, then v + w uv + vec x uv with uv = 2 vec x v
    uv = _cross(vec, loc)
    uv = [x + x for x in uv]
    c = _cross(vec, uv)
    return [loc[i] + q[0] * uv[i] + c[i] for i in range(3)]


def sine2d(a, b, dtype):
    n1 = _sqrt(a[0] * a[0] + a[1] * a[1] + dtype(EPS))
    n2 = _sqrt(b[0] * b[0] + b[1] * b[1] + dtype(EPS))
    return _clamp1(_abs((a[0] * b[1] - a[1] * b[0]) / (n1 * n2)), dtype)


def cosine2d(a, b, dtype):
    n1 = _sqrt(a[0] * a[0] + a[1] * a[1] + dtype(EPS))
    n2 = _sqrt(b[0] * b[0] + b[1] * b[1] + dtype(EPS))
    return _clamp1(_abs((a[0] * b[0] + a[1] * b[1]) / (n1 * n2)), dtype)


def line_line(k, q, t, p3d, dir3d, p2d, dtype):
    pa = pixel_to_world(k, q, t, p2d[0], p2d[1], dtype(1))
    pb = pixel_to_world(k, q, t, p2d[0], p2d[1], dtype(2))
    d_ = [pb[i] - pa[i] for i in range(3)]
    n = _cross(d_, dir3d)
    nsq = n[0] * n[0] + n[1] * n[1] + n[2] * n[2]
    d = [p3d[i] - pa[i] for i in range(3)]

    def parallel():
        c = _cross(d_, d)
        return _sqrt(_dot(c, c) / _dot(d_, d_) + dtype(E8))

    def skew():
        return _dot(n, d) / _sqrt(nsq)
    if isinstance(nsq, Dual) or np.ndim(nsq) == 0:
        return parallel() if val(nsq) <= E8 else skew()
    with np.errstate(all="ignore"):
        return np.where(nsq <= E8, parallel(), skew())


def line_residual(cost, weight, k, q, t, l3, l2, dtype):
    """ReprojectionLineFunctor; l3 = 6 and l2 = 4 dtype scalars (or arrays over blocks)"""
    s3, e3, s2, e2 = l3[:3], l3[3:], l2[:2], l2[2:]
    dir3d = [e3[i] - s3[i] for i in range(3)]
    n3 = _sqrt(_dot(dir3d, dir3d) + dtype(E8))
    dir3d = [x / n3 for x in dir3d]
    sr, er = world_to_pixel(k, q, t, s3), world_to_pixel(k, q, t, e3)
    dir2d = [er[0] - sr[0], er[1] - sr[1]]
    dn = _sqrt(dir2d[0] * dir2d[0] + dir2d[1] * dir2d[1] + dtype(E8))
    dir2d = [dir2d[0] / dn, dir2d[1] / dn]
    half = dtype(0.5)
    if cost in (0, 1):
        m1 = [half * (sr[0] + er[0]), half * (sr[1] + er[1])]
        m2 = [half * (s2[0] + e2[0]), half * (s2[1] + e2[1])]
        res = [m1[0] - m2[0], m1[1] - m2[1]]
        if cost == 1:
            d1 = [er[0] - sr[0], er[1] - sr[1]]
            n1 = _sqrt(d1[0] * d1[0] + d1[1] * d1[1] + dtype(E8))
            d1 = [d1[0] / n1, d1[1] / n1]
            d2 = [e2[0] - s2[0], e2[1] - s2[1]]
            n2 = _sqrt(d2[0] * d2[0] + d2[1] * d2[1] + dtype(E8))
            d2 = [d2[0] / n2, d2[1] / n2]
            res.append(n1 * sine2d(d1, d2, dtype))
    elif cost in (2, 3):
        disp1 = [s2[0] - sr[0], s2[1] - sr[1]]
        disp2 = [e2[0] - sr[0], e2[1] - sr[1]]
        sin1, sin2 = sine2d(dir2d, disp1, dtype), sine2d(dir2d, disp2, dtype)
        r = [disp1[0] * sin1, disp1[1] * sin1, disp2[0] * sin2, disp2[1] * sin2]
        res = r if cost == 3 else [_sqrt(r[0] * r[0] + r[1] * r[1] + dtype(E8)), _sqrt(r[2] * r[2] + r[3] * r[3] + dtype(E8))]
    elif cost == 4:
        res = [line_line(k, q, t, s3, dir3d, s2, dtype), line_line(k, q, t, s3, dir3d, e2, dtype)]
    else:
        p1a = pixel_to_world(k, q, t, s2[0], s2[1], dtype(1)); p1b = pixel_to_world(k, q, t, s2[0], s2[1], dtype(2))
        p2a = pixel_to_world(k, q, t, e2[0], e2[1], dtype(1)); p2b = pixel_to_world(k, q, t, e2[0], e2[1], dtype(2))
        d1 = [p1b[i] - p1a[i] for i in range(3)]
        d2 = [p2b[i] - p2a[i] for i in range(3)]
        n = _cross(d1, d2)
        nsq = n[0] * n[0] + n[1] * n[1] + n[2] * n[2]
        ds = [s3[i] - p1a[i] for i in range(3)]
        de = [e3[i] - p1a[i] for i in range(3)]
        res = [_dot(n, ds) / _sqrt(nsq), _dot(n, de) / _sqrt(nsq)]
    direc = [e2[0] - s2[0], e2[1] - s2[1]]
    if weight == 1:
        w = _exp(dtype(10) * (dtype(1) - cosine2d(dir2d, direc, dtype)))
    elif weight == 3:
        w = _sqrt(direc[0] * direc[0] + direc[1] * direc[1] + dtype(E8))
    elif weight == 4:
        w = 1 / _sqrt(direc[0] * direc[0] + direc[1] * direc[1] + dtype(E8))
    else:
        return res
    return [x * w for x in res]


def point_residual(use3d, k, q, t, p3, p2, dtype):
    if use3d:
        pa = pixel_to_world(k, q, t, p2[0], p2[1], dtype(1))
        pb = pixel_to_world(k, q, t, p2[0], p2[1], dtype(2))
        d_ = [pb[i] - pa[i] for i in range(3)]
        dn = _sqrt(_dot(d_, d_) + dtype(E8))
        d_ = [x / dn for x in d_]
        d = [p3[i] - pa[i] for i in range(3)]
        dp = _dot(d, d_)
        return [_sqrt(_dot(d, d) - dp * dp + dtype(E8)), 0 * dp]
    xy = world_to_pixel(k, q, t, p3)
    return [xy[0] - p2[0], xy[1] - p2[1]]


def loss(kind, a, s, dtype):
    """rho(s), rho'(s) of Ceres' TrivialLoss / HuberLoss / SoftLOneLoss / CauchyLoss; s a scalar or an array"""
    a = dtype(a) if np.ndim(s) == 0 else a
    b = a * a
    tiny = np.finfo(np.float64).tiny
    if kind == 1:
        with np.errstate(all="ignore"):
            r = np.sqrt(s)
            return np.where(s > b, 2 * a * r - b, s), np.where(s > b, np.maximum(tiny, a / r), 1)
    if kind == 2:
        tmp = np.sqrt(1 + s / b)
        return 2 * b * (tmp - 1), np.maximum(tiny, 1 / tmp)
    if kind == 3:
        return b * np.log(1 + s / b), np.maximum(tiny, 1 / (1 + s / b))
    return s, s * 0 + 1


def blocks(problem, weight_line, weight_point, dtype):
    """JointLocEngine::AddResiduals: (kind, 3D, 2D, ScaledLoss weight) per block"""
    out = []
    for l3, group in zip(problem["l3ds"], problem["l2ds"]):
        g = [np.asarray(s, dtype).reshape(4) for s in group]
        lengths = [np.sqrt((s[2] - s[0]) ** 2 + (s[3] - s[1]) ** 2) for s in g]
        total = dtype(0)
        for x in lengths:
            total = total + x
        for s, x in zip(g, lengths):
            out.append((0, np.asarray(l3, dtype).reshape(6), s, dtype(weight_line) * x / total))
    for p3, p2 in zip(problem["p3ds"], problem["p2ds"]):
        out.append((1, np.asarray(p3, dtype).reshape(3), np.asarray(p2, dtype).reshape(2), dtype(weight_point)))
    return out


def _seeds(pose, which, dtype):
    q0, q1, q2, q3 = [dtype(x) for x in pose[:4]]
    t = [dtype(x) for x in pose[4:]]
    z, o = dtype(0), dtype(1)
    if which == 0:
        q = [Dual(q0, [-q1, -q2, -q3, z], dtype), Dual(q1, [q0, q3, -q2, z], dtype), Dual(q2, [-q3, q0, q1, z], dtype),
             Dual(q3, [q2, -q1, q0, z], dtype)]
        return q, [Dual(t[0], [z, z, z, o], dtype), Dual(t[1], None, dtype), Dual(t[2], None, dtype)]
    q = [Dual(x, None, dtype) for x in (q0, q1, q2, q3)]
    return q, [Dual(t[0], None, dtype), Dual(t[1], [o, z, z, z], dtype), Dual(t[2], [z, o, z, z], dtype)]


def normalise_pose(pose, dtype):
    """CameraPose's constructor normalises its quaternion once"""
    p = np.asarray(pose, dtype).copy()
    q = p[:4]
    p[:4] = q / np.sqrt((q[0] * q[0] + q[2] * q[2]) + (q[1] * q[1] + q[3] * q[3]))
    return p


def evaluate(problem, cfg, pose, dtype=np.float64):
    """residuals (blocks, 4; NaN where a block has fewer), cost, g (6), H (6, 6) at pose = (qvec, tvec).
    cfg: dict(cost=0..5, weight=0/1/3/4, loss=0..3, loss_a, weight_line, weight_point)"""
    pose = normalise_pose(pose, dtype)
    k = [dtype(x) for x in problem["kvec"]]
    use3d = cfg["cost"] in (4, 5)
    bl = blocks(problem, cfg["weight_line"], cfg["weight_point"], dtype)
    R = np.full((len(bl), 4), np.nan, dtype)
    g, H, cost = np.zeros(6, dtype), np.zeros((6, 6), dtype), dtype(0)
    for n, (kind, x3, x2, w) in enumerate(bl):
        J = None
        for which in (0, 1):
            q, t = _seeds(pose, which, dtype)
            rr = (point_residual(use3d, k, q, t, list(x3), list(x2), dtype) if kind else
                  line_residual(cfg["cost"], cfg["weight"], k, q, t, list(x3), list(x2), dtype))
            if J is None:
                J = np.zeros((len(rr), 6), dtype)
                rv = np.array([x.v for x in rr], dtype)
                J[:, :4] = np.stack([x.d for x in rr])
            else:
                J[:, 4:] = np.stack([x.d[:2] for x in rr])
        s = (rv * rv).sum()
        rho, rho1 = loss(cfg["loss"], cfg["loss_a"], s, dtype)
        cost = cost + w * rho
        H += w * rho1 * (J.T @ J)
        g += w * rho1 * (J.T @ rv)
        R[n, :len(rv)] = rv
    return R, cost / dtype(2), g, H


def pack(problem, cfg):
    """the blocks as float64 arrays for residual_vector (pose-independent)"""
    bl = blocks(problem, cfg["weight_line"], cfg["weight_point"], np.float64)
    ln = [b for b in bl if b[0] == 0]
    pt = [b for b in bl if b[0] == 1]
    f = lambda rows, i, w: np.array([r[i] for r in rows], float).reshape(-1, w).T  # noqa: E731
    return dict(k=np.asarray(problem["kvec"], float), l3=f(ln, 1, 6), l2=f(ln, 2, 4), lw=np.array([r[3] for r in ln], float),
                p3=f(pt, 1, 3), p2=f(pt, 2, 2), pw=np.array([r[3] for r in pt], float))


def residual_vector(pk, cfg, pose):
    """f with 1/2 |f|^2 = the cost: per block r sqrt(w rho(s) / s) (r sqrt(w) where s = 0); float64, all blocks as array
    lanes of the same expressions; the pose's quaternion already normalised"""
    arr = lambda x: np.asarray(x, np.float64)  # noqa: E731
    q, t, k = [np.float64(x) for x in pose[:4]], [np.float64(x) for x in pose[4:]], list(pk["k"])
    out = []
    for rr, w in ((line_residual(cfg["cost"], cfg["weight"], k, q, t, list(pk["l3"]), list(pk["l2"]), arr), pk["lw"]),
                  (point_residual(cfg["cost"] in (4, 5), k, q, t, list(pk["p3"]), list(pk["p2"]), arr), pk["pw"])):
        if len(w) == 0:
            continue
        rr = np.array([np.broadcast_to(x, w.shape) for x in rr], float)
        s = (rr * rr).sum(0)
        rho, _ = loss(cfg["loss"], cfg["loss_a"], s, arr)
        with np.errstate(all="ignore"):
            f = np.where(s > 0, np.sqrt(w * rho / s), np.sqrt(w))
        out.append((rr * f).ravel())
    return np.concatenate(out) if out else np.zeros(0)


def cost_only(pk, cfg, pose):
    f = residual_vector(pk, cfg, pose)
    return 0.5 * float(f @ f)


def retract(pose, dl):
    q0, q1, q2, q3 = pose[:4]
    r = np.array([q0 - dl[0] * q1 - dl[1] * q2 - dl[2] * q3, q1 + dl[0] * q0 + dl[1] * q3 - dl[2] * q2,
                  q2 - dl[0] * q3 + dl[1] * q0 + dl[2] * q1, q3 + dl[0] * q2 - dl[1] * q1 + dl[2] * q0])
    return np.concatenate([r / np.linalg.norm(r), np.asarray(pose[4:], float) + dl[3:]])


# ---- pose scoring: JointPoseEstimator::EvaluateModelOnPoint (joint_pose_estimator.cc:176-251), float64 or longdouble ----
DBL_MAX = np.finfo(np.float64).max
COS_1_DEG = 0.9998476951563913  # cos(pi / 180)


def _rot_eigen(q, dtype):
    """CameraPose::R(): the quaternion re-normalised, then Eigen's toRotationMatrix"""
    q = np.asarray(q, dtype)
    w, x, y, z = q / np.sqrt((q * q).sum())
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype)


def score_cell(cost, kvec, q, t, kind, x3, x2, l3d, min_depth, overlap, dtype=np.float64, margins=None):
    """the squared error of one correspondence, DBL_MAX where a cheirality test fails.  margins (a list): receives the
    distance of every threshold quantity the cell reached from its threshold -- (|dot| - cos 1 deg) for the two rays,
    (depth - min_depth) for the depths, (length - overlap) for the overlap"""
    m = margins if margins is not None else []
    q = np.asarray(q, dtype); t = np.asarray(t, dtype)
    if np.isnan(np.sqrt((q * q).sum())) or np.isnan(np.sqrt((t * t).sum())):
        return DBL_MAX
    q = q / np.sqrt((q * q).sum())
    k = [dtype(v) for v in kvec]
    R = _rot_eigen(q, dtype)
    depth = lambda p: (R @ p + t)[2]  # noqa: E731
    if kind == 1:
        d = depth(np.asarray(x3, dtype))
        m.append(("depth", float(d - dtype(min_depth))))
        if not d >= min_depth:
            return DBL_MAX
        r = point_residual(cost in (4, 5), k, list(q), list(t), [dtype(v) for v in x3], [dtype(v) for v in x2], dtype)
        return r[0] * r[0] + r[1] * r[1]
    l3 = np.asarray(l3d, dtype).reshape(2, 3)
    s2, e2 = np.asarray(x2, dtype).reshape(2, 2)
    ld = (l3[1] - l3[0]) / np.sqrt(((l3[1] - l3[0]) ** 2).sum())
    lm = np.cross(l3[0], ld)
    Kinv = np.array([[1 / k[0], 0, -k[2] / k[0]], [0, 1 / k[1], -k[3] / k[1]], [0, 0, 1]], dtype)
    C = -R.T @ t
    rays = []
    for p2 in (s2, e2):
        v = (R.T @ Kinv) @ np.array([p2[0], p2[1], 1], dtype)
        rays.append(v / np.sqrt((v * v).sum()))
    for ray in rays:
        c = abs(ray @ ld)
        m.append(("angle", float(c - dtype(COS_1_DEG))))
        if c > COS_1_DEG:
            return DBL_MAX
    for ray in rays:
        c = np.cross(ld, ray)
        p = (-np.cross(lm, np.cross(ray, c)) + (np.cross(C, ray) @ c) * ld) / (c @ c)
        d = depth(p)
        m.append(("depth", float(d - dtype(min_depth))))
        if not d >= min_depth:
            return DBL_MAX
    Km = np.array([[k[0], 0, k[2]], [0, k[1], k[3]], [0, 0, 1]], dtype)
    proj = []
    for p in l3:
        h = Km @ (R @ p + t)
        proj.append(h[:2] / (h[2] + dtype(EPS)))
    a, b = proj
    dirv = (b - a) / np.sqrt(((b - a) ** 2).sum())
    length = np.sqrt(((a - b) ** 2).sum())
    pp = []
    for p2 in (s2, e2):
        pr = (p2 - a) @ dirv
        pp.append(a if pr < 0 else (b if pr > length else a + pr * dirv))
    ov = np.sqrt(((pp[0] - pp[1]) ** 2).sum())
    m.append(("overlap", float(ov - dtype(overlap))))
    if ov < overlap:
        return DBL_MAX
    r = line_residual(cost, 0, k, list(q), list(t), [dtype(v) for v in l3.reshape(6)], [dtype(v) for v in (*s2, *e2)], dtype)
    return sum(x * x for x in r)


def score_table(cost, kvec, poses, l3ds, l3d_ids, l2ds, p3ds, p2ds, min_depth, overlap, dtype=np.float64):
    """-> table (H, N) and per cell the smallest |margin| among the thresholds it reached (inf where it reached none)"""
    H, N = len(poses), len(p3ds) + len(l2ds)
    tab = np.zeros((H, N), dtype)
    mar = np.full((H, N), np.inf)
    for h, pose in enumerate(poses):
        for i in range(N):
            ms = []
            if i < len(p3ds):
                tab[h, i] = score_cell(cost, kvec, pose[:4], pose[4:], 1, p3ds[i], p2ds[i], None, min_depth, overlap, dtype, ms)
            else:
                j = i - len(p3ds)
                tab[h, i] = score_cell(cost, kvec, pose[:4], pose[4:], 0, None, l2ds[j], l3ds[l3d_ids[j]], min_depth, overlap,
                                       dtype, ms)
            if ms:
                mar[h, i] = min(abs(v) for _, v in ms)
    return tab, mar


def msac_from_table(tab, n_points, thr2, weights, width=64):
    """the MSAC score and the inlier counts of every pose from its row of the table, summed in the project's order: lane
    i % 64 adds its terms in ascending order, then the xor tree over the 64 lanes"""
    H, N = tab.shape
    scores, inl = np.zeros(H), np.zeros((H, 2), np.int32)
    for h in range(H):
        part = np.zeros(width)
        for i in range(N):
            ty = 0 if i < n_points else 1
            part[i % width] = part[i % width] + min(tab[h, i], thr2[ty]) * weights[ty]
            inl[h, ty] += tab[h, i] < thr2[ty]
        m = width // 2
        while m >= 1:
            part = part + part[np.arange(width) ^ m]
            m //= 2
        scores[h] = part[0]
    return scores, inl
