"""NumPy restatement of MeshEvaluator's distance, the contract limap_amd.evaluation.MeshEvaluator
is held to bit for bit.

For a query p and a face (a, b, c): Ericson's ClosestPtPointTriangle (Real-Time Collision Detection, section 5.1.5), all
FP64, never contracted to FMA, with dot(u, v) = (u0*v0 + u1*v1) + u2*v2 and sqn(u) = dot(u, u):

    ab = b - a, ac = c - a, ap = p - a, d1 = dot(ab, ap), d2 = dot(ac, ap)
    1. d1 <= 0 and d2 <= 0                                   -> q = a
    2. bp = p - b, d3 = dot(ab, bp), d4 = dot(ac, bp)
       d3 >= 0 and d4 <= d3                                  -> q = b
    3. vc = d1*d4 - d3*d2; vc <= 0 and d1 >= 0 and d3 <= 0   -> q = a + (d1 / (d1 - d3)) * ab
    4. cp = p - c, d5 = dot(ab, cp), d6 = dot(ac, cp)
       d6 >= 0 and d5 <= d6                                  -> q = c
    5. vb = d5*d2 - d1*d6; vb <= 0 and d2 >= 0 and d6 <= 0   -> q = a + (d2 / (d2 - d6)) * ac
    6. va = d3*d6 - d5*d4; va <= 0 and (d4 - d3) >= 0 and (d5 - d6) >= 0
                                                             -> q = b + ((d4 - d3) / ((d4 - d3) + (d5 - d6))) * (c - b)
    7. s = (va + vb) + vc; s > 0: denom = 1.0 / s, v = vb*denom, w = vc*denom, q = (a + ab*v) + ac*w
       otherwise (project rule, a degenerate face): the minimum with < over the edges AB, BC, CA of the clamped
       projection u + t*e, t = dot(p - u, e) / dot(e, e) if dot(e, e) > 0 else 0, clamped to [0, 1]

The face's squared distance is sqn(p - q); the distance to the mesh is sqrt of the minimum over the faces, kept with <
from +inf (a NaN, e.g. from 0/0 in region 3 of a face with a == b, never wins).  libigl's
point_simplex_squared_distance restates the same routine, but agreement with it is not claimed or checked.

Elementwise ufuncs only (no BLAS, no einsum): nothing reorders or fuses.  Brute force over the faces, chunked.  The
sampling and segment helpers of the base evaluator come from eval_oracle.py."""
import numpy as np

import eval_oracle as eo


def dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _edge(u, w, p):
    e = w - u
    ee = dot(e, e)
    up = p - u
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(ee > 0, dot(up, e) / np.where(ee > 0, ee, 1.0), 0.0)
    t = np.where(t < 0, 0.0, np.where(t > 1, 1.0, t))
    q = u + t[..., None] * e
    r = p - q
    return dot(r, r)


def tri_dist2(a, b, c, p):
    """squared distances, broadcasting a, b, c (..., 3) against p (..., 3)"""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ab, ac, ap = b - a, c - a, p - a
        d1, d2 = dot(ab, ap), dot(ac, ap)
        bp = p - b
        d3, d4 = dot(ab, bp), dot(ac, bp)
        vc = d1 * d4 - d3 * d2
        cp = p - c
        d5, d6 = dot(ab, cp), dot(ac, cp)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        s = (va + vb) + vc
        # region 7, and the project rule where s is not > 0
        denom = 1.0 / s
        v7, w7 = vb * denom, vc * denom
        q = (a + ab * v7[..., None]) + ac * w7[..., None]
        r = p - q
        out = dot(r, r)
        m1, m2, m3 = _edge(a, b, p), _edge(b, c, p), _edge(c, a, p)
        deg = np.where(m1 < np.inf, m1, np.inf)
        deg = np.where(m2 < deg, m2, deg)
        deg = np.where(m3 < deg, m3, deg)
        out = np.where(s > 0, out, deg)
        # regions 6 .. 1, the first match wins: assigned last
        bc = c - b
        q6 = b + (e43 / (e43 + e56))[..., None] * bc
        q5 = a + (d2 / (d2 - d6))[..., None] * ac
        q3 = a + (d1 / (d1 - d3))[..., None] * ab
        for m, qq in (((va <= 0) & (e43 >= 0) & (e56 >= 0), q6),
                      ((vb <= 0) & (d2 >= 0) & (d6 <= 0), q5),
                      ((d6 >= 0) & (d5 <= d6), np.broadcast_to(c, q.shape)),
                      ((vc <= 0) & (d1 >= 0) & (d3 <= 0), q3),
                      ((d3 >= 0) & (d4 <= d3), np.broadcast_to(b, q.shape)),
                      ((d1 <= 0) & (d2 <= 0), np.broadcast_to(a, q.shape))):
            rr = p - qq
            out = np.where(m, dot(rr, rr), out)
    return out


def region(a, b, c, p):
    """the region (1-7, 0 = the project rule) that decides the closest point, for the known-answer tests"""
    a, b, c, p = (np.asarray(x, np.float64) for x in (a, b, c, p))
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = dot(ab, ap), dot(ac, ap)
    if d1 <= 0 and d2 <= 0:
        return 1
    bp = p - b
    d3, d4 = dot(ab, bp), dot(ac, bp)
    if d3 >= 0 and d4 <= d3:
        return 2
    vc = d1 * d4 - d3 * d2
    if vc <= 0 and d1 >= 0 and d3 <= 0:
        return 3
    cp = p - c
    d5, d6 = dot(ab, cp), dot(ac, cp)
    if d6 >= 0 and d5 <= d6:
        return 4
    vb = d5 * d2 - d1 * d6
    if vb <= 0 and d2 >= 0 and d6 <= 0:
        return 5
    va = d3 * d6 - d5 * d4
    if va <= 0 and (d4 - d3) >= 0 and (d5 - d6) >= 0:
        return 6
    return 7 if (va + vb) + vc > 0 else 0


def scale_vertices(V, mpau):
    return np.asarray(V, np.float64).reshape(-1, 3) * float(mpau)


def nearest_dists(V, F, queries, block=512, fblock=2048):
    """distance of each query (Q, 3) to the mesh (V already scaled): sqrt of the < minimum of the faces' squared
    distances, from +inf"""
    V = np.asarray(V, np.float64).reshape(-1, 3)
    F = np.asarray(F, np.int64).reshape(-1, 3)
    Q = np.asarray(queries, np.float64).reshape(-1, 3)
    A, B, Cc = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    out = np.empty(Q.shape[0])
    for q0 in range(0, Q.shape[0], block):
        p = Q[q0:q0 + block][:, None, :]
        best = np.full(p.shape[0], np.inf)
        for f0 in range(0, F.shape[0], fblock):
            d = tri_dist2(A[None, f0:f0 + fblock], B[None, f0:f0 + fblock], Cc[None, f0:f0 + fblock], p)
            # the < fold from +inf: NaN never wins; over the rest (all >= +0) it is the order-free minimum
            m = np.where(np.isnan(d), np.inf, d).min(axis=1)
            best = np.where(m < best, m, best)
        out[q0:q0 + block] = np.sqrt(best)
    return out


# ---- the base evaluator's functions over the mesh distance ------------------------------------------------------------
def sample_dists(V, F, lines, n, center=True):
    a = eo.as_lines(lines)
    s = eo.samples_center(a, n) if center else eo.samples_ends(a, n)
    return nearest_dists(V, F, s.reshape(-1, 3)).reshape(a.shape[0], n)


def inlier_ratios(V, F, lines, thresholds, n=1000):
    d = sample_dists(V, F, lines, n)
    th = np.asarray(thresholds, np.float64).reshape(-1)
    c = np.stack([(d <= t).sum(axis=1) for t in th], 1).astype(np.int64)
    return c.astype(np.float64) / float(n)


def dist_line(V, F, line, n=1000):
    d = sample_dists(V, F, line, n, center=False).reshape(-1)
    s = 0.0
    for v in d.tolist():  # std::accumulate
        s += v
    return s / float(n)


def segs(V, F, lines, threshold, n, inlier):
    """(S, 6) endpoints of ComputeInlierSegs / ComputeOutlierSegs"""
    a = eo.as_lines(lines)
    if a.shape[0] == 0:
        return np.zeros((0, 6))
    d = sample_dists(V, F, a, n)
    interval = 1.0 / n
    out = []
    for k in range(a.shape[0]):
        s, v = a[k, 0:3], a[k, 3:6] - a[k, 0:3]
        flag = (d[k] <= threshold) if inlier else ~(d[k] <= threshold)
        start = -1
        for i in range(n + 1):
            f = bool(flag[i]) if i < n else False
            if f and start == -1:
                start = i
            elif not f and start != -1:
                out.append(np.concatenate([s + (start * interval) * v, s + (i * interval) * v]))
                start = -1
    return np.array(out).reshape(-1, 6)
