"""NumPy restatement of limap's own part of the bundle adjustment with free poses: both residual
blocks of HybridBAEngine with the pose as a variable, in upstream's operation order, on any dtype.  Paths relative to
src/limap:

    optimize/hybrid_bundle_adjustment/cost_functions.h:28-85           point_residual()
    ceresbase/point_projection.h:8-57                                  WorldToPixel (Ceres' QuaternionRotatePoint)
    optimize/line_refinement/cost_functions.h:96-178                   line_residual()
    ceresbase/line_transforms.h:8-29, line_projection.h:14-80          refine_oracle.plucker, world_to_pixel below
    optimize/hybrid_bundle_adjustment/hybrid_bundle_adjustment.cc:125-225   blocks(): order, weights, switches

Derivatives come from refine_oracle's dual-number class (four directions at a time): one pass for the rotation's three
directions, one for the translation's, one for the structure's three or four -- the project's retractions
(q + dq_i (0, e_i) (x) q, t + dt, p + dp, section 19's line chart).  The scalar functions also take arrays (one lane per
block), which the scipy comparison uses.
"""
import numpy as np

import refine_oracle as ro
from refine_oracle import Dual, EPS, CAUCHY_B


def rotate_point(q, p):
    """ceres::QuaternionRotatePoint: the scale 1 / |q|, then UnitQuaternionRotatePoint in its cross-product form"""
    scale = 1 / ro._sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    a, b, c, d = scale * q[0], scale * q[1], scale * q[2], scale * q[3]
    uv0, uv1, uv2 = c * p[2] - d * p[1], d * p[0] - b * p[2], b * p[1] - c * p[0]
    uv0, uv1, uv2 = uv0 + uv0, uv1 + uv1, uv2 + uv2
    return [p[0] + a * uv0 + (c * uv2 - d * uv1), p[1] + a * uv1 + (d * uv0 - b * uv2), p[2] + a * uv2 + (b * uv1 - c * uv0)]


def point_residual(kvec, q, t, X, xy):
    r = rotate_point(q, X)
    z = r[2] + t[2]
    u, v = (r[0] + t[0]) / z, (r[1] + t[1]) / z
    return [kvec[0] * u + kvec[2] - xy[0], kvec[1] * v + kvec[3] - xy[1]]


def world_to_pixel(kvec, q, t, d, m, dtype):
    """refine_oracle.world_to_pixel with the pose a variable (Duals or arrays)"""
    zero = dtype(0)
    R = ro._mat3(ro.quat_to_rot_ceres(q))
    Rd = [R[i][0] * d[0] + R[i][1] * d[1] + R[i][2] * d[2] for i in range(3)]
    RmR = ro._mm(ro._mm(R, ro._skew(m, zero)), ro._T(R))
    M = [[RmR[i][j] - t[i] * Rd[j] + Rd[i] * t[j] for j in range(3)] for i in range(3)]
    mt = [M[2][1], M[0][2], M[1][0]]
    fx, fy, cx, cy = kvec
    K = [[fx, zero, cx], [zero, fy, cy], [zero, zero, dtype(1)]]
    Cm = ro._mm(ro._mm(K, ro._skew(mt, zero)), ro._T(K))
    c = [Cm[2][1], Cm[0][2], Cm[1][0]]
    n = ro._sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2] + dtype(EPS))
    return [c[0] / n, c[1] / n, c[2] / n]


def line_residual(kvec, q, t, u, w, seg4, alpha, dtype):
    d, m = ro.plucker(u, w, dtype)
    coor = world_to_pixel(kvec, q, t, d, m, dtype)
    p1, p2 = [seg4[0], seg4[1]], [seg4[2], seg4[3]]
    dn = ro._sqrt(coor[0] * coor[0] + coor[1] * coor[1] + dtype(EPS))
    dir2d = [-coor[1] / dn, coor[0] / dn]
    direc = [p2[0] - p1[0], p2[1] - p1[1]]
    cos = ro.cosine2d(dir2d, direc, dtype)
    wgt = ro._exp(dtype(alpha) * (dtype(1) - cos))
    d1 = (p1[0] * coor[0] + p1[1] * coor[1] + coor[2]) / dn
    d2 = (p2[0] * coor[0] + p2[1] * coor[1] + coor[2]) / dn
    return [d1 * wgt, d2 * wgt]


def blocks(s, lw_point=0.1, constant_point=False, constant_line=False, min_num_images=4):
    """SetUp()'s residual blocks in order: dicts kind, row (of the collection), s (structure), obs, w; the structures'
    constant flags; the rows of the images with residuals in ascending id"""
    row = {int(i): n for n, i in enumerate(s["img_ids"])}
    out, const = [], []
    NP, NL = len(s["poff"]) - 1, len(s["loff"]) - 1
    for n in range(NP):
        a, b = int(s["poff"][n]), int(s["poff"][n + 1])
        cnt = 0
        if lw_point > 0:
            for i in range(a, b):
                out.append(dict(kind=0, row=row[int(s["pimg"][i])], s=n, obs=s["pxy"][i], w=lw_point))
                cnt += 1
        const.append(bool(constant_point) or cnt == 0)
    for n in range(NL):
        a, b = int(s["loff"][n]), int(s["loff"][n + 1])
        order = np.argsort(s["limg"][a:b], kind="stable") + a
        for i in order:
            sg = s["l2d"][i]
            out.append(dict(kind=1, row=row[int(s["limg"][i])], s=NP + n, obs=sg, w=np.hypot(sg[0] - sg[2], sg[1] - sg[3]) / 30.0))
        const.append(bool(constant_line) or len(set(int(x) for x in s["limg"][a:b])) < min_num_images)
    rows = sorted({b["row"] for b in out}, key=lambda r: int(s["img_ids"][r]))
    return out, const, rows


def start_params(s, params6=None):
    """per image (q normalised once, t), per structure its parameters (points 3, lines uvec + wvec)"""
    poses = [np.concatenate([ro.normalise_q(s["q"][n], np.float64), s["t"][n]]) for n in range(len(s["img_ids"]))]
    sp = [np.asarray(x, float) for x in s["p3"]]
    for n in range(len(s["loff"]) - 1):
        sp.append(np.asarray(params6[n], float) if params6 is not None else ro.minimal(s["line6"][n]))
    return poses, sp


def _seed_q(q, dtype):
    z = dtype(0)
    q0, q1, q2, q3 = [dtype(x) for x in q]
    return [Dual(q0, [-q1, -q2, -q3, z], dtype), Dual(q1, [q0, q3, -q2, z], dtype), Dual(q2, [-q3, q0, q1, z], dtype),
            Dual(q3, [q2, -q1, q0, z], dtype)]


def _const(v, dtype):
    return [Dual(x, None, dtype) for x in v]


def block_jets(b, kvec, pose, sp, alpha, dtype):
    """the residuals of a block and its Jacobians: r (2), Jc (2, 6), Js (2, 3 or 4)"""
    k = [dtype(x) for x in kvec]
    obs = [dtype(x) for x in b["obs"]]
    qc, tc = _const(pose[:4], dtype), _const(pose[4:], dtype)
    if b["kind"]:
        xc = _const(sp, dtype)
        us, ws = ro.seeds(sp, dtype)
        xs = us + ws
        nd = 4
    else:
        xc = _const(sp, dtype)
        xs = [Dual(sp[i], np.eye(4)[i], dtype) for i in range(3)]
        nd = 3

    def res(q, t, x):
        if b["kind"]:
            return line_residual(k, q, t, x[:4], x[4:], obs, alpha, dtype)
        return point_residual(k, q, t, x, obs)
    rq = res(_seed_q(pose[:4], dtype), tc, xc)
    rt = res(qc, [Dual(pose[4 + i], np.eye(4)[i], dtype) for i in range(3)], xc)
    rs = res(qc, tc, xs)
    r = np.array([rq[0].v, rq[1].v], dtype)
    Jc = np.array([np.concatenate([rq[m].d[:3], rt[m].d[:3]]) for m in range(2)], dtype)
    Js = np.array([rs[m].d[:nd] for m in range(2)], dtype)
    return r, Jc, Js


def evaluate(s, dtype=np.float64, alpha=10.0, params6=None, **switches):
    """residuals (NB, 2), cost, g (nu), H (nu, nu) at the scene's start; the unknowns: (dq, dt) of the images with
    residuals in ascending id, then the free structures in order"""
    blks, const, rows = blocks(s, **switches)
    poses, sp = start_params(s, params6)
    cam_of = {r: n for n, r in enumerate(rows)}
    off, nu = [], 6 * len(rows)
    for n, c in enumerate(const):
        off.append(-1 if c else nu)
        if not c:
            nu += 4 if len(sp[n]) == 6 else 3
    r_all = np.zeros((len(blks), 2), dtype)
    g, H, cost = np.zeros(nu, dtype), np.zeros((nu, nu), dtype), dtype(0)
    bb = dtype(CAUCHY_B)
    for i, b in enumerate(blks):
        r, Jc, Js = block_jets(b, s["k"][b["row"]], poses[b["row"]], sp[b["s"]], alpha, dtype)
        sq = r[0] * r[0] + r[1] * r[1]
        w = dtype(b["w"])
        if b["kind"]:
            cost = cost + w * bb * np.log(dtype(1) + sq / bb)
            rho1 = w / (dtype(1) + sq / bb)
        else:
            cost = cost + w * sq
            rho1 = w
        cols = list(range(6 * cam_of[b["row"]], 6 * cam_of[b["row"]] + 6))
        J = Jc
        if off[b["s"]] >= 0:
            cols += list(range(off[b["s"]], off[b["s"]] + Js.shape[1]))
            J = np.concatenate([Jc, Js], 1)
        cols = np.array(cols)
        H[np.ix_(cols, cols)] += rho1 * (J.T @ J)
        g[cols] += rho1 * (J.T @ r)
        r_all[i] = r
    return r_all, cost / dtype(2), g, H


# ---- the cost on arrays, one lane per block (float64), for scipy ----
class Packed:
    """the scene's blocks as arrays and the global chart: x = per image (q4, t3), per point 3, per line (u4, w2), raw --
    the residuals normalise them as upstream's do"""

    def __init__(self, s, alpha=10.0, **switches):
        blks, _, rows = blocks(s, **switches)
        self.alpha = alpha
        self.n_img, self.NP, self.NL = len(s["img_ids"]), len(s["poff"]) - 1, len(s["loff"]) - 1
        self.k = np.asarray(s["k"], float)
        pb = [b for b in blks if b["kind"] == 0]
        lb = [b for b in blks if b["kind"] == 1]
        self.p_row = np.array([b["row"] for b in pb], int); self.p_s = np.array([b["s"] for b in pb], int)
        self.p_obs = np.array([b["obs"] for b in pb], float).reshape(-1, 2); self.p_w = np.array([b["w"] for b in pb], float)
        self.l_row = np.array([b["row"] for b in lb], int); self.l_s = np.array([b["s"] - self.NP for b in lb], int)
        self.l_obs = np.array([b["obs"] for b in lb], float).reshape(-1, 4); self.l_w = np.array([b["w"] for b in lb], float)

    def pack(self, poses, sp):
        return np.concatenate([np.concatenate(poses)] + [np.asarray(x, float) for x in sp]) if len(sp) else np.concatenate(poses)

    def start(self, s, params6=None):
        return self.pack(*start_params(s, params6))

    def split(self, x):
        n7 = 7 * self.n_img
        return x[:n7].reshape(-1, 7), x[n7:n7 + 3 * self.NP].reshape(-1, 3), x[n7 + 3 * self.NP:].reshape(-1, 6)

    def residuals(self, x):
        """the blocks' residuals scaled by sqrt(rho(s) / s): half their squared norm is the cost"""
        arr = lambda v: np.asarray(v, np.float64)  # noqa: E731
        pose, pts, lines = self.split(np.asarray(x, float))
        out = []
        if len(self.p_row):
            P, X, K = pose[self.p_row].T, pts[self.p_s].T, self.k[self.p_row].T
            r = point_residual(K, P[:4], P[4:], X, self.p_obs.T)
            sw = np.sqrt(self.p_w)
            out += [r[0] * sw, r[1] * sw]
        if len(self.l_row):
            P, U, K = pose[self.l_row].T, lines[self.l_s].T, self.k[self.l_row].T
            r = line_residual(K, P[:4], P[4:], U[:4], U[4:], self.l_obs.T, self.alpha, arr)
            sq = r[0] * r[0] + r[1] * r[1]
            rho = self.l_w * CAUCHY_B * np.log1p(sq / CAUCHY_B)
            sc = np.sqrt(rho / np.where(sq > 0, sq, 1.0))
            out += [r[0] * sc, r[1] * sc]
        return np.concatenate(out)

    def cost(self, x):
        f = self.residuals(x)
        return 0.5 * float(f @ f)

    def chart(self, x0):
        """the minimiser's chart around the packed point x0: y = per image (dq, dt), per point dp, per line (du, dw) ->
        the packed point the project's retractions reach (the charts of lt_lm.h's loop: LcChart, p + dp, section 19's RfChart)"""
        pose0, pts0, lines0 = [a.copy() for a in self.split(np.asarray(x0, float))]
        n6, n3 = 6 * self.n_img, 3 * self.NP

        def to_point(y):
            dc, dp, dl = y[:n6].reshape(-1, 6), y[n6:n6 + n3].reshape(-1, 3), y[n6 + n3:].reshape(-1, 4)
            q0, q1, q2, q3 = pose0[:, :4].T
            a, b, c = dc[:, :3].T
            q = np.stack([q0 - a * q1 - b * q2 - c * q3, q1 + a * q0 + b * q3 - c * q2, q2 - a * q3 + b * q0 + c * q1,
                          q3 + a * q2 - b * q1 + c * q0], 1)
            q = q / np.linalg.norm(q, axis=1, keepdims=True)
            pose = np.concatenate([q, pose0[:, 4:] + dc[:, 3:]], 1)
            lines = np.array([ro.retract(l, d) for l, d in zip(lines0, dl)]).reshape(-1, 6)
            return np.concatenate([pose.ravel(), (pts0 + dp).ravel(), lines.ravel()])
        return to_point, n6 + n3 + 4 * self.NL


def cholesky_loop(S, rhs=None):
    """the defined recurrence as a straight loop: L_ij = (S_ij - sum_{k<j} L_ik L_jk) / L_jj, the sum in ascending k from
    S_ij; forward and back substitution under the same rule"""
    n = len(S)
    L = np.zeros((n, n))
    for j in range(n):
        col = np.array(S[j:, j], float)  # rows i >= j of column j, every row its own ascending-k chain
        for k in range(j):
            col = col - L[j:, k] * L[j, k]
        L[j, j] = np.sqrt(col[0])
        L[j + 1:, j] = col[1:] / L[j, j]
    if rhs is None:
        return L, None
    x = np.zeros(n)
    for i in range(n):
        sm = rhs[i]
        for k in range(i):
            sm = sm - L[i, k] * x[k]
        x[i] = sm / L[i, i]
    for i in range(n - 1, -1, -1):
        sm = x[i]
        for k in range(i + 1, n):
            sm = sm - L[k, i] * x[k]
        x[i] = sm / L[i, i]
    return L, x
