"""NumPy restatement of limap.evaluation's semantics (evaluation/base_evaluator.cc, point_cloud_evaluator.cc,
refline_evaluator.cc; base/linebase.cc:67-80), the contract limap_amd.evaluation is held to.  Elementwise ufuncs only:
nothing contracts to FMA and there are no BLAS dots, so every double is the reference's expression in its order.
Minima are taken over squared distances with one sqrt at the end (sqrt is correctly rounded, hence monotone).
Brute force, chunked: meant for test-sized scenes."""
import numpy as np

EPS = 1e-12
DBL_MAX = np.finfo(np.float64).max


def as_lines(lines):
    a = np.asarray(lines, np.float64)
    return a.reshape(-1, 6)


def sqn(v):
    """squaredNorm of 3-vectors along the last axis: (x*x + y*y) + z*z"""
    return (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def length(a):
    return np.sqrt(sqn(a[:, 0:3] - a[:, 3:6]))


def direction(a):
    """Eigen normalized(): divided by the norm when the squared norm is > 0, unchanged otherwise"""
    v = a[:, 3:6] - a[:, 0:3]
    z = sqn(v)
    n = np.sqrt(z)
    out = v.copy()
    pos = z > 0
    out[pos] = v[pos] / n[pos][:, None]
    return out


def samples_center(a, n):
    """start + ((i + 0.5) * (1.0 / n)) * (end - start): ComputeInlierRatio and the seg functions"""
    c = (np.arange(n, dtype=np.float64) + 0.5) * (1.0 / n)
    s, v = a[:, None, 0:3], (a[:, 3:6] - a[:, 0:3])[:, None, :]
    return s + c[None, :, None] * v


def samples_ends(a, n):
    """start + (i * (1.0 / (n - 1))) * (end - start): ComputeDistLine"""
    c = np.arange(n, dtype=np.float64) * (1.0 / (n - 1))
    s, v = a[:, None, 0:3], (a[:, 3:6] - a[:, 0:3])[:, None, :]
    return s + c[None, :, None] * v


def samples_refline(a, n):
    """start + ((length / (n - 1)) * i) * direction(): RefLineEvaluator::ComputeRecallLength"""
    with np.errstate(divide="ignore", invalid="ignore"):
        interval = length(a) / float(n - 1)
        c = interval[:, None] * np.arange(n, dtype=np.float64)[None, :]
        return a[:, None, 0:3] + c[:, :, None] * direction(a)[:, None, :]


def nearest_dists(points, queries, block=4096):
    """exact distance of each query (Q, 3) to its nearest cloud point: sqrt of the minimum of (q - p) squared norms"""
    P = np.asarray(points, np.float64).reshape(-1, 3)
    Q = np.asarray(queries, np.float64).reshape(-1, 3)
    out = np.empty(Q.shape[0])
    pb = max(1, (1 << 24) // max(block, 1))
    for q0 in range(0, Q.shape[0], block):
        q = Q[q0:q0 + block]
        best = np.full(q.shape[0], np.inf)
        for p0 in range(0, P.shape[0], pb):
            d = q[:, None, :] - P[None, p0:p0 + pb, :]
            best = np.minimum(best, sqn(d).min(axis=1))
        out[q0:q0 + block] = np.sqrt(best)
    return out


def seg_dist2(a, p):
    """Line3d::point_distance squared, points p (P, 3) x lines a (L, 6) -> (P, L)"""
    s, e = a[None, :, 0:3], a[None, :, 3:6]
    d = direction(a)[None, :, :]
    ln = length(a)[None, :]
    w = p[:, None, :] - s
    proj = dot(w, d)
    c = s + proj[..., None] * d
    c = np.where((proj > ln)[..., None], e, c)
    c = np.where((proj < 0)[..., None], s, c)
    return sqn(p[:, None, :] - c)


def refline_dist2(a, p):
    """RefLineEvaluator::DistPointLine squared: min(max(|p-s|^2 - ((p-s).dir)^2, 0), min(|p-s|^2, |p-e|^2))"""
    s, e = a[None, :, 0:3], a[None, :, 3:6]
    d = direction(a)[None, :, :]
    w = p[:, None, :] - s
    ds2 = sqn(w)
    de2 = sqn(p[:, None, :] - e)
    t = dot(w, d)
    perp = ds2 - t * t
    perp = np.where(perp < 0, 0.0, perp)
    ends = np.where(de2 < ds2, de2, ds2)
    return np.where(ends < perp, ends, perp)


def _min_over_lines(fn, a, p, block=2048):
    a = as_lines(a)
    p = np.asarray(p, np.float64).reshape(-1, 3)
    best = np.full(p.shape[0], np.inf)
    if a.shape[0] == 0:
        return best
    lb = max(1, (1 << 22) // max(block, 1))
    for p0 in range(0, p.shape[0], block):
        for l0 in range(0, a.shape[0], lb):
            m = fn(a[l0:l0 + lb], p[p0:p0 + block]).min(axis=1)
            best[p0:p0 + block] = np.minimum(best[p0:p0 + block], m)
    return best


def dists_for_each_point(points, lines):
    """ComputeDistsforEachPoint: min over lines of point_distance, DBL_MAX when the minimum never drops below it"""
    b = _min_over_lines(seg_dist2, lines, points)
    return np.where(b < np.inf, np.sqrt(b), DBL_MAX)


def dist_point_lines(p, lines):
    """DistPointLines with its EPS early exit (a minimum below EPS returns 0)"""
    with np.errstate(invalid="ignore"):
        b = _min_over_lines(refline_dist2, lines, p)
    m = np.where(b < np.inf, np.sqrt(b), DBL_MAX)
    return np.where(m < EPS, 0.0, m)


# ---- the evaluator functions --------------------------------------------------------------------------------------------
def inlier_counts(points, lines, thresholds, n=1000):
    a = as_lines(lines)
    d = nearest_dists(points, samples_center(a, n).reshape(-1, 3)).reshape(a.shape[0], n)
    th = np.asarray(thresholds, np.float64).reshape(-1)
    return np.stack([(d <= t).sum(axis=1) for t in th], 1).astype(np.int64), d


def inlier_ratios(points, lines, thresholds, n=1000):
    c, _ = inlier_counts(points, lines, thresholds, n)
    return c.astype(np.float64) / float(n)


def dist_line(points, line, n=1000):
    a = as_lines(line)
    d = nearest_dists(points, samples_ends(a, n).reshape(-1, 3))
    s = 0.0
    for v in d.tolist():
        s += v
    return s / float(n)


def segs(points, lines, threshold, n, inlier):
    """the (start, end) pairs of ComputeInlierSegs / ComputeOutlierSegs, as an (S, 6) array"""
    a = as_lines(lines)
    if a.shape[0] == 0:
        return np.zeros((0, 6))
    d = nearest_dists(points, samples_center(a, n).reshape(-1, 3)).reshape(a.shape[0], n)
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


def refline_counts(qlines, lines, thresholds, n=1000):
    q = as_lines(qlines)
    th = np.asarray(thresholds, np.float64).reshape(-1)
    if q.shape[0] == 0:
        return np.zeros((0, th.size), np.int64)
    d = dist_point_lines(samples_refline(q, n).reshape(-1, 3), lines).reshape(q.shape[0], n)
    return np.stack([(d < t).sum(axis=1) for t in th], 1).astype(np.int64)


def recall_length(qlines, lines, thresholds, n=1000):
    q = as_lines(qlines)
    c = refline_counts(q, lines, thresholds, n)
    lens = length(q).tolist()
    out = []
    for t in range(c.shape[1]):
        r = 0.0
        for k, ln in enumerate(lens):
            r += ln * float(c[k, t]) / n
        out.append(r)
    return np.array(out)


def sum_length(lines):
    s = 0.0
    for v in length(as_lines(lines)).tolist():
        s += v
    return s
