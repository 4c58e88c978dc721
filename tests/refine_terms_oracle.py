"""NumPy restatement of the VP and the heatmap term of limap.optimize.line_refinement, written
from upstream's files in their operation order and parameterised on the dtype (float64, longdouble); the geometric term,
the dual numbers and the parameterisation come from refine_oracle.  Paths relative to src/limap:

    optimize/line_refinement/cost_functions.h:35-90, refine.cc:87-126          vp_residual(), the VP blocks
    ceresbase/line_dists.h:40-57, ceresbase/line_projection.h:125-134          sine3d(), direction_from_vp()
    optimize/line_refinement/pixel_cost_functions.h:34-107, refine.cc:315-360  heatmap_residuals(), the heatmap blocks
    base/linetrack.cc:324-351, base/infinite_line.cc:9-16                      sample_lines()
    ceresbase/line_transforms.h:55-72                                          intersect()
    ceresbase/interpolation.h:526-579, features/featuremap.h:71-85             bilinear(): Grid2D clamps, forward
                                                                               differences, one node at (0, 0)
Ceres' own parts by their published procedures: QuaternionRotatePoint, CrossProduct, TrivialLoss, HuberLoss,
ScaledLoss, the Jet of an interpolated value (dfdr dr + dfdc dc).  A sample with |p_homo[2]| < EPS fails; an
evaluation with a failed sample has cost +inf (this project's rule).
"""
import numpy as np

import refine_oracle as ro
from refine_oracle import EPS, Dual, _abs, _sqrt, val

HUBER_A = 0.001
DEFAULT_TERMS = dict(use_geometric=True, use_vp=False, vp_multiplier=1.0, use_heatmap=False, n_samples_heatmap=10,
                     sample_range_min=0.05, sample_range_max=0.95, heatmap_multiplier=1.0)


def terms_of(**kw):
    t = dict(DEFAULT_TERMS)
    t.update(kw)
    return t


def _cross(x, y):
    return [x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0]]


def rotate_point(q, pt, dtype):
    """ceres::QuaternionRotatePoint: the scale 1 / |q|, then UnitQuaternionRotatePoint"""
    q = [dtype(x) for x in q]
    scale = dtype(1) / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    q = [x * scale for x in q]
    uv = _cross(q[1:], pt)
    uv = [x + x for x in uv]
    c = _cross(q[1:], uv)
    return [pt[i] + q[0] * uv[i] + c[i] for i in range(3)]


def direction_from_vp(vp, kvec, dtype):
    vp = [dtype(x) for x in vp]
    k = [dtype(x) for x in kvec]
    d = [vp[0] / k[0] - k[2] / k[0] * vp[2], vp[1] / k[1] - k[3] / k[1] * vp[2], vp[2]]
    n = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + dtype(EPS))
    return [x / n for x in d]


def sine3d(a, b, dtype):
    na = _sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2] + dtype(EPS))
    nb = _sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2] + dtype(EPS))
    r = _cross([x / na for x in a], [x / nb for x in b])
    s = _sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + dtype(EPS))
    if val(s) > 1:
        return Dual(1, None, dtype) if isinstance(s, Dual) else dtype(1)
    return s


def vp_residual(cam11n, vp, u, w, dtype):
    """cam11n: the view with its quaternion normalised once (ro.cams_normalised)"""
    d, _ = ro.plucker(u, w, dtype)
    rot = rotate_point(cam11n[4:8], d, dtype)
    return sine3d(rot, direction_from_vp(vp, cam11n[:4], dtype), dtype)


def sample_lines(seg4, n, tmin, tmax, dtype):
    """ComputeHeatmapSamples for one support: n normalised line coordinates"""
    s = np.array([dtype(x) for x in seg4[:2]])
    e = np.array([dtype(x) for x in seg4[2:]])
    interval = (dtype(tmax) - dtype(tmin)) / dtype(n - 1)
    d = (e - s) / np.sqrt((e - s)[0] ** 2 + (e - s)[1] ** 2)
    perp = np.array([d[1], -d[0]])
    out = []
    for j in range(n):
        p = s + (dtype(tmin) + interval * dtype(j)) * (e - s)
        coor = np.array([perp[1], -perp[0], -perp[1] * p[0] + perp[0] * p[1]])
        out.append(coor / np.sqrt(coor[0] ** 2 + coor[1] ** 2 + coor[2] ** 2))
    return out


def intersect(c1, c2, dtype):
    """Ceres_IntersectLineCoordinates -> (ok, xy)"""
    p = _cross(c1, c2)
    n = _sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2])
    p = [x / n for x in p]
    if not abs(val(p[2])) >= dtype(EPS):
        return False, None
    return True, [p[0] / p[2], p[1] / p[2]]


def _texel(hm, r, c, dtype):
    h, w = hm.shape
    return dtype(hm[min(max(r, 0), h - 1), min(max(c, 0), w - 1)])


def _interp(dx, dy, ll, lr, ul, ur):
    one = type(dx)(1)
    return (one - dy) * ((one - dx) * ll + dx * lr) + dy * ((one - dx) * ul + dx * ur)


def bilinear(hm, r, c, dtype):
    """BiLinearInterpolator::Evaluate at (r, c) -> f; as Duals the Jet with the forward differences"""
    rv, cv = dtype(val(r)), dtype(val(c))
    row, col = int(np.floor(rv)), int(np.floor(cv))
    dy, dx = rv - dtype(row), cv - dtype(col)
    t = lambda a, b: _texel(hm, row + a, col + b, dtype)  # noqa: E731
    ll, lr, ul, ur = t(0, 0), t(0, 1), t(1, 0), t(1, 1)
    f = _interp(dx, dy, ll, lr, ul, ur)
    if not isinstance(r, Dual):
        return f
    dfdr = _interp(dx, dy, ul, ur, t(2, 0), t(2, 1)) - f
    dfdc = _interp(dx, dy, lr, t(0, 2), ur, t(1, 2)) - f
    return Dual(f, dfdr * r.d + dfdc * c.d, dtype)


def heatmap_residuals(cam11n, seg4, hm, u, w, terms, dtype):
    """-> (ok, residuals (n), xy (n, 2) values) of one support"""
    d, m = ro.plucker(u, w, dtype)
    coor = ro.world_to_pixel(cam11n[:4], cam11n[4:8], cam11n[8:11], d, m, dtype)
    res, xys, ok = [], [], True
    for k in sample_lines(seg4, terms["n_samples_heatmap"], terms["sample_range_min"], terms["sample_range_max"], dtype):
        good, xy = intersect(coor, [dtype(x) for x in k], dtype)
        if not good:
            ok = False
            res.append(None)
            xys.append([np.nan, np.nan])
            continue
        res.append(dtype(1) - bilinear(hm, xy[1], xy[0], dtype))
        xys.append([float(val(xy[0])), float(val(xy[1]))])
    return ok, res, np.array(xys)


def huber(s, dtype):
    """HuberLoss(0.001) -> rho, rho'"""
    a = dtype(HUBER_A)
    b = a * a
    if s > b:
        r = np.sqrt(s)
        return dtype(2) * a * r - b, max(dtype(np.finfo(np.float64).tiny), a / r)
    return s, dtype(1)


def evaluate(cam11, segs4, p, terms, vp_flag=None, vp3=None, heatmaps=None, alpha=10.0, dtype=np.float64):
    """One track at the minimal parameters p, supports in residual order; heatmaps: one array per support.
    -> dict(r (K, 3 + n) with NaN where a block is absent, cost, g, H, failed, xy (K, n, 2), huber_s (K))"""
    cams = ro.cams_normalised(cam11, dtype)
    u, w = ro.seeds(p, dtype)
    K = len(segs4)
    n = terms["n_samples_heatmap"] if terms["use_heatmap"] else 0
    r = np.full((K, 3 + n), np.nan, dtype)
    g = np.zeros(4, dtype)
    H = np.zeros((4, 4), dtype)
    cost = dtype(0)
    failed = False
    xy = np.full((K, n, 2), np.nan)
    hub = np.full(K, np.nan)
    b = dtype(ro.CAUCHY_B)

    def add(rho1, blocks):
        nonlocal g, H
        J = np.stack([x.d for x in blocks])
        rv = np.array([x.v for x in blocks], dtype)
        H += rho1 * (J.T @ J)
        g += rho1 * (J.T @ rv)

    for k in range(K):
        s = [dtype(x) for x in segs4[k]]
        wk = np.sqrt((s[0] - s[2]) ** 2 + (s[1] - s[3]) ** 2) / dtype(30)
        if terms["use_geometric"]:
            rr = ro.residual(cams[k], s, u, w, alpha, dtype)
            sq = rr[0].v * rr[0].v + rr[1].v * rr[1].v
            cost = cost + wk * b * np.log(dtype(1) + sq / b)
            add(wk / (dtype(1) + sq / b), rr)
            r[k, 0], r[k, 1] = rr[0].v, rr[1].v
        if terms["use_vp"] and vp_flag[k]:
            rv = vp_residual(cams[k], vp3[k], u, w, dtype)
            wv = wk * dtype(terms["vp_multiplier"])
            cost = cost + wv * (rv.v * rv.v)
            add(wv, [rv])
            r[k, 2] = rv.v
        if terms["use_heatmap"]:
            ok, res, xy[k] = heatmap_residuals(cams[k], s, heatmaps[k], u, w, terms, dtype)
            if not ok:
                failed = True
                continue
            wh = wk * dtype(terms["heatmap_multiplier"]) / (dtype(n) / dtype(10))
            sq = dtype(0)
            for x in res:
                sq = sq + x.v * x.v
            rho, rho1 = huber(sq, dtype)
            hub[k] = float(sq)
            cost = cost + wh * rho
            add(wh * rho1, res)
            r[k, 3:] = [x.v for x in res]
    cost = dtype(np.inf) if failed else cost / dtype(2)
    return dict(r=r, cost=cost, g=g, H=H, failed=failed, xy=xy, huber_s=hub)


def cost_only(cam11n, segs4, p, terms, vp_flag=None, vp3=None, heatmaps=None, alpha=10.0):
    """the float64 cost at p = (u4, w2) without derivatives (cameras already normalised); for a minimiser that is not
    the code under test"""
    f = np.float64
    u, w = [f(x) for x in p[:4]], [f(x) for x in p[4:]]
    cost = 0.0
    for k in range(len(segs4)):
        s = [f(x) for x in segs4[k]]
        wk = np.sqrt((s[0] - s[2]) ** 2 + (s[1] - s[3]) ** 2) / 30.0
        if terms["use_geometric"]:
            rr = ro.residual(cam11n[k], s, u, w, alpha, f)
            cost += wk * ro.CAUCHY_B * np.log1p((rr[0] * rr[0] + rr[1] * rr[1]) / ro.CAUCHY_B)
        if terms["use_vp"] and vp_flag[k]:
            rv = vp_residual(cam11n[k], vp3[k], u, w, f)
            cost += wk * terms["vp_multiplier"] * rv * rv
        if terms["use_heatmap"]:
            ok, res, _ = heatmap_residuals(cam11n[k], s, heatmaps[k], u, w, terms, f)
            if not ok:
                return np.inf
            cost += wk * terms["heatmap_multiplier"] / (terms["n_samples_heatmap"] / 10.0) * huber(sum(x * x for x in res), f)[0]
    return 0.5 * float(cost)
