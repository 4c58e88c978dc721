"""CPU oracle of the GPU line fitter (limap_amd.fitting, lt_kernels_fit.hip): pure NumPy and Python.

It restates, in the device's operation order:
  - the front half of estimate_seg3d_from_depth (fitting/fitting.py:20-53): Bresenham pixels in closed form, the image
    bounds, the depth gather, the inf filter, the exact median, the threshold and the unprojection;
  - LO-MSAC (RansacLib's LocallyOptimizedMSAC as restated in DESIGN §12) over Line3dEstimator
    (fitting/line3d_estimator.cc), with the project's counter-based generator and its 3x3 Jacobi eigen-solver;
  - the reduction orders: the MSAC score as 64 lane partial sums (lane l takes points l, l+64, ...) folded by a
    butterfly of 32, 16, ..., 1; centroid and covariance sums in sample order.
`ref_front_half` repeats the reference's NumPy arithmetic in its order (np.linalg.inv, @) for the CPU tests.
"""
import math

import numpy as np

M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15
DBL_MAX = float(np.finfo(np.float64).max)
EPS = 1e-12
LN2 = 0.6931471805599453

STATUS_OK, STATUS_TOO_FEW, STATUS_LOW_RATIO = 0, 1, 2


# ---- generator ------------------------------------------------------------------------------------------------------
def fmix(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def stream_key(seed, img_id, line, stream):
    k = fmix((seed + GOLD) & M64)
    k = fmix(k ^ (((img_id & 0xFFFFFFFF) + GOLD) & M64))
    k = fmix(k ^ (((line & M64) + GOLD) & M64))
    return fmix(k ^ ((stream + GOLD) & M64))


class Stream:
    """draw c of a stream: the high 32 bits of fmix(key + (c + 1) * GOLD); uniform(n) rejects draws below
    2^32 mod n, then takes the draw mod n."""

    def __init__(self, seed, img_id, line, stream):
        self.k = stream_key(seed, img_id, line, stream)
        self.c = 0

    def draw(self):
        self.c += 1
        return fmix((self.k + self.c * GOLD) & M64) >> 32

    def uniform(self, n):
        thr = ((1 << 32) - n) % n
        while True:
            u = self.draw()
            if u >= thr:
                return u % n


# ---- Bresenham ------------------------------------------------------------------------------------------------------
def bresenham_seq(x0, y0, x1, y1):
    """the `bresenham` package's generator, restated (sign / major axis, ties y-major, D = 2 dy - dx, step on D >= 0)"""
    dx, dy = x1 - x0, y1 - y0
    xs, ys = (1 if dx > 0 else -1), (1 if dy > 0 else -1)
    dx, dy = abs(dx), abs(dy)
    if dx > dy:
        xx, xy, yx, yy = xs, 0, 0, ys
    else:
        dx, dy = dy, dx
        xx, xy, yx, yy = 0, ys, xs, 0
    D = 2 * dy - dx
    y = 0
    out = []
    for x in range(dx + 1):
        out.append((x0 + x * xx + y * yx, y0 + x * xy + y * yy))
        if D >= 0:
            y += 1
            D -= 2 * dx
        D += 2 * dy
    return out


def bresenham_closed(x0, y0, x1, y1, i):
    """pixel i of bresenham_seq: minor step k = floor((2 dmin i + dmaj) / (2 dmaj))"""
    dx, dy = x1 - x0, y1 - y0
    xs, ys = (1 if dx > 0 else -1), (1 if dy > 0 else -1)
    adx, ady = abs(dx), abs(dy)
    if adx > ady:
        k = (2 * ady * i + adx) // (2 * adx)
        return x0 + xs * i, y0 + ys * k
    k = (2 * adx * i + ady) // (2 * ady) if ady > 0 else 0
    return x0 + xs * k, y0 + ys * i


def raster(seg4, w, h):
    """the in-image pixels of the truncated segment in Bresenham order: the device walks only the indices whose major
    coordinate lies in the image and filters the minor one"""
    x0, y0, x1, y1 = (int(v) for v in seg4[:4])
    dx, dy = x1 - x0, y1 - y0
    xs, ys = (1 if dx > 0 else -1), (1 if dy > 0 else -1)
    if abs(dx) > abs(dy):
        a0, sa, A, m0, sm, M, dmaj, dmin = x0, xs, w, y0, ys, h, abs(dx), abs(dy)
    else:
        a0, sa, A, m0, sm, M, dmaj, dmin = y0, ys, h, x0, xs, w, abs(dy), abs(dx)
    if sa > 0:
        lo, hi = max(0, -a0), min(dmaj, A - 1 - a0)
    else:
        lo, hi = max(0, a0 - A + 1), min(dmaj, a0)
    px, py = [], []
    for i in range(lo, hi + 1):
        k = (2 * dmin * i + dmaj) // (2 * dmaj) if dmaj > 0 else 0
        a, m = a0 + sa * i, m0 + sm * k
        if 0 <= m < M:
            if abs(dx) > abs(dy):
                px.append(a); py.append(m)
            else:
                px.append(m); py.append(a)
    return np.asarray(px, np.int64), np.asarray(py, np.int64)


# ---- camera ---------------------------------------------------------------------------------------------------------
def cam_R(q4):
    """the rotation of the native camera table (lt_geom.h cam_build), same operation order"""
    q4 = [float(v) for v in q4]
    n0 = math.sqrt((q4[0] * q4[0] + q4[2] * q4[2]) + (q4[1] * q4[1] + q4[3] * q4[3]))
    q = [v / n0 if n0 > 0.0 else v for v in q4]
    n = math.sqrt((q[0] * q[0] + q[2] * q[2]) + (q[1] * q[1] + q[3] * q[3]))
    if n == 0.0:
        w, x, y, z = 1.0, q[1], q[2], q[3]
    else:
        w, x, y, z = q[0] / n, q[1] / n, q[2] / n, q[3] / n
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [1.0 - (tyy + tzz), txy - twz, txz + twy,
            txy + twz, 1.0 - (txx + tzz), tyz - twx,
            txz - twy, tyz + twx, 1.0 - (txx + tyy)]


# ---- front half -----------------------------------------------------------------------------------------------------
def median_of(d):
    """np.median's value: float32 maps in float32 (mean of the two middle values), others in float64"""
    f32 = d.dtype == np.float32
    d = d if f32 else d.astype(np.float64)
    n = len(d)
    if np.isnan(d).any():
        return d.dtype.type(np.nan)
    s = np.sort(d, kind="stable")
    if n % 2:
        return s[n // 2]
    if f32:
        return np.float32(s[n // 2 - 1] + s[n // 2]) / np.float32(2)
    return (float(s[n // 2 - 1]) + float(s[n // 2])) / 2.0


def front_half(seg4, depth, k4, q4, t3, var2d=5.0, ransac_th=0.75):
    """-> dict(px, py, depth, median, unc, t2, points (n, 3)); points None when n <= 6"""
    h, w = depth.shape
    px, py = raster(seg4, w, h)
    d = depth[py, px]
    if d.dtype.kind == "f":
        keep = ~np.isinf(d)
        px, py, d = px[keep], py[keep], d[keep]
    out = dict(px=px, py=py, depth=d, median=None, unc=None, t2=None, points=None)
    n = len(d)
    if n <= 6:
        return out
    med = median_of(d)
    fx, fy, cx, cy = (float(v) for v in k4)
    f = (fx + fy) / 2.0
    if d.dtype == np.float32:
        unc = float(np.float32(np.float32(var2d) * med)) / f
    else:
        unc = (float(var2d) * float(med)) / f
    th = float(ransac_th) * unc
    R = cam_R(q4)
    t = [float(v) for v in t3]
    ct = [(R[i] * t[0] + R[3 + i] * t[1]) + R[6 + i] * t[2] for i in range(3)]
    dd = d.astype(np.float64)
    ux = (px.astype(np.float64) - cx) / fx
    uy = (py.astype(np.float64) - cy) / fy
    p0, p1, p2 = ux * dd, uy * dd, dd
    pts = np.stack([((R[i] * p0 + R[3 + i] * p1) + R[6 + i] * p2) - ct[i] for i in range(3)], 1)
    out.update(median=med, unc=unc, t2=th * th, points=pts)
    return out


def ref_front_half(seg2d, depth, K, R, T, var2d=5.0, ransac_th=0.75):
    """The reference's NumPy arithmetic for the front half (fitting.py:25-52), operation for operation, as a checker of
    front_half: integer pixels of the truncated segment (bresenham_seq), the image bounds, the depth lookup, the inf
    filter, then inv(K) times homogeneous pixels scaled by depth and moved to the world by R^T (p - T) written as
    R^T p - R^T T, with NumPy's median and the var2d formula in NumPy's promotion."""
    rows, cols = depth.shape
    ends = [int(v) for v in np.asarray(seg2d)[:4].astype(int)]
    xy = np.array(bresenham_seq(*ends)).T  # (2, n): x over y
    inside = (xy[0] >= 0) & (xy[1] >= 0) & (xy[0] < cols) & (xy[1] < rows)
    xy = xy[:, inside]
    z = depth[xy[1], xy[0]]
    keep = ~np.isinf(z)
    xy, z = xy[:, keep], z[keep]
    hom = np.vstack([xy, np.ones((1, xy.shape[1]))])  # float64
    cam = (np.linalg.inv(K) @ hom) * z
    world = (R.T @ cam) - (R.T @ T)[:, None]
    res = dict(px=xy[0], py=xy[1], depth=z, points=world.T, median=None, th=None)
    if world.shape[1] > 6:
        mid = np.median(z)
        unc = var2d * mid / ((K[0, 0] + K[1, 1]) / 2.0)
        res.update(median=mid, unc=unc, th=ransac_th * unc)
    return res


# ---- LO-MSAC --------------------------------------------------------------------------------------------------------
class Options:
    """LORansacOptions with the binding's defaults (estimators/bindings.cc:50-75, RansacLib's defaults)"""

    def __init__(self, **kw):
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
        for k, v in kw.items():
            setattr(self, k, v)


def lt_log(x):
    """the project's natural log (device and oracle): x = m 2^e, m in [sqrt(1/2), sqrt(2)), s = (m-1)/(m+1),
    log = e ln2 + 2 (s + s^3/3 + ... + s^25/25) by Horner in s^2; +, -, *, / only"""
    if x != x or x < 0.0:
        return float("nan")
    if x == 0.0:
        return float("-inf")
    if x == float("inf"):
        return x
    m, e = math.frexp(x)
    if m < 0.7071067811865476:
        m *= 2.0
        e -= 1
    s = (m - 1.0) / (m + 1.0)
    s2 = s * s
    p = 1.0 / 25.0
    for k in range(23, 0, -2):
        p = p * s2 + 1.0 / k
    return float(e) * LN2 + 2.0 * (s * p)


def num_required_iterations(ratio, prob_missing, sample_size, min_it, max_it):
    """utils::NumRequiredIterations; pow(r, 2) is r * r, a count at or above max_it is max_it"""
    if ratio <= 0.0:
        return max_it
    if ratio >= 1.0:
        return min_it
    q = 1.0 - ratio * ratio
    if q >= 0.99999999999999:
        return max_it
    with np.errstate(divide="ignore", invalid="ignore"):
        it = float(np.ceil(np.float64(lt_log(prob_missing)) / np.float64(lt_log(q)) + 0.5))
    n = int(it) if it < float(max_it) else max_it
    return max(min_it, n)


def wave_sum(v):
    """lane l sums v[l], v[l + 64], ... in order from 0.0, then lanes fold by 32, 16, 8, 4, 2, 1"""
    n = len(v)
    rows = (n + 63) // 64
    pad = np.zeros(rows * 64)
    pad[:n] = v
    acc = np.zeros(64)
    for r in range(rows):
        acc = acc + pad[64 * r:64 * r + 64]
    s = 32
    while s >= 1:
        acc = acc[:s] + acc[s:2 * s]
        s //= 2
    return float(acc[0])


def jacobi_min_eigvec(C):
    """3x3 symmetric eigen-solver of the device: cyclic Jacobi, pairs (0,1), (0,2), (1,2), at most 16 sweeps, stop when
    the off-diagonal sum is 0; the column of the smallest diagonal entry (first on ties), unit length, its entry of
    largest magnitude (first on ties) made positive.  None for a non-finite matrix."""
    a = [[C[0], C[1], C[2]], [C[1], C[3], C[4]], [C[2], C[4], C[5]]]
    for v in C:
        if not math.isfinite(v):
            return None
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(16):
        off = (abs(a[0][1]) + abs(a[0][2])) + abs(a[1][2])
        if off == 0.0:
            break
        for p, q, r in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
            apq = a[p][q]
            if apq == 0.0:
                continue
            theta = (a[q][q] - a[p][p]) / (2.0 * apq)
            t = 1.0 / (abs(theta) + math.sqrt(theta * theta + 1.0))
            if theta < 0.0:
                t = -t
            c = 1.0 / math.sqrt(t * t + 1.0)
            s = t * c
            app = a[p][p] - t * apq
            aqq = a[q][q] + t * apq
            arp, arq = a[r][p], a[r][q]
            nrp = c * arp - s * arq
            nrq = s * arp + c * arq
            a[r][p] = a[p][r] = nrp
            a[r][q] = a[q][r] = nrq
            a[p][p], a[q][q] = app, aqq
            a[p][q] = a[q][p] = 0.0
            for k in range(3):
                vkp, vkq = V[k][p], V[k][q]
                V[k][p] = c * vkp - s * vkq
                V[k][q] = s * vkp + c * vkq
    k = 0
    if a[1][1] < a[k][k]:
        k = 1
    if a[2][2] < a[k][k]:
        k = 2
    v = [V[0][k], V[1][k], V[2][k]]
    nrm = math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    v = [x / nrm for x in v]
    j = 0
    if abs(v[1]) > abs(v[j]):
        j = 1
    if abs(v[2]) > abs(v[j]):
        j = 2
    if v[j] < 0.0:
        v = [-x for x in v]
    return v


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


class Fitter:
    """LO-MSAC over one point set; models are (d, m, from_lo)"""

    def __init__(self, pts, opt, t2, img_id, line):
        self.P = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
        self.X, self.Y, self.Z = self.P[:, 0].copy(), self.P[:, 1].copy(), self.P[:, 2].copy()
        self.n = len(self.P)
        self.o = opt
        self.t2 = float(t2)
        self.smp = Stream(int(opt.random_seed_), img_id, line, 0)
        self.shf = Stream(int(opt.random_seed_), img_id, line, 1)

    def residuals(self, mdl):
        (dx, dy, dz), (mx, my, mz) = mdl[0], mdl[1]
        X, Y, Z = self.X, self.Y, self.Z
        c0, c1, c2 = dy * Z - dz * Y, dz * X - dx * Z, dx * Y - dy * X
        q0, q1, q2 = mx + c0, my + c1, mz + c2
        e0, e1, e2 = dy * q2 - dz * q1, dz * q0 - dx * q2, dx * q1 - dy * q0
        f0, f1, f2 = X - (X + e0), Y - (Y + e1), Z - (Z + e2)
        return (f0 * f0 + f1 * f1) + f2 * f2

    def score(self, mdl):
        r = self.residuals(mdl)
        t2 = self.t2
        with np.errstate(invalid="ignore"):
            s = np.where(t2 < r, t2, r)  # std::min(r, t2)
        return wave_sum(s)

    def inliers(self, mdl, thr):
        r = self.residuals(mdl)
        with np.errstate(invalid="ignore"):
            return list(np.nonzero(r < thr)[0])

    def minimal(self, i0, i1):
        p1, p2 = self.P[i0], self.P[i1]
        d = (float(p2[0]) - float(p1[0]), float(p2[1]) - float(p1[1]), float(p2[2]) - float(p1[2]))
        ln = math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        if ln != ln or ln < EPS:
            return None
        dd = (d[0] / ln, d[1] / ln, d[2] / ln)
        p = (float(p1[0]), float(p1[1]), float(p1[2]))
        return (dd, cross(p, dd), False)

    def nonminimal(self, sample):
        k = len(sample)
        if k < 6:
            return None
        sx = sy = sz = 0.0
        for i in sample:
            sx += float(self.X[i]); sy += float(self.Y[i]); sz += float(self.Z[i])
        c = (sx / k, sy / k, sz / k)
        C = [0.0] * 6
        for i in sample:
            a, b, e = float(self.X[i]) - c[0], float(self.Y[i]) - c[1], float(self.Z[i]) - c[2]
            C[0] += a * a; C[1] += a * b; C[2] += a * e; C[3] += b * b; C[4] += b * e; C[5] += e * e
        den = float(k - 1)
        C = [v / den for v in C]
        v = jacobi_min_eigvec(C)
        if v is None:
            return None
        v = tuple(v)
        return (v, cross(c, v), True)

    def shuffle_resize(self, lst, target):
        if len(lst) > target:
            m = len(lst)
            for i in range(target):
                j = i + self.shf.uniform(m - i)
                lst[i], lst[j] = lst[j], lst[i]
            del lst[target:]
        return lst

    def lsq_fit(self, thr, mdl):
        inl = self.inliers(mdl, thr)
        if len(inl) < 2:
            return mdl
        k = min(self.o.min_sample_multiplicator_ * 2, len(inl))
        self.shuffle_resize(inl, k)
        r = self.nonminimal(inl)
        return mdl if r is None else r

    def local_opt(self, best, best_score):
        o, t2 = self.o, self.t2
        if 6 > self.n:
            return best, best_score
        mult = float(o.threshold_multiplier_)
        m_init = self.lsq_fit(t2 * mult, best)
        sc = self.score(m_init)
        if sc < best_score:
            best, best_score = m_init, sc
        base = self.inliers(m_init, t2 * mult)
        k_nm = max(6, min(2 * o.non_min_sample_multiplier_, len(base) // 2))
        for _ in range(o.num_lo_steps_):
            sample = self.shuffle_resize(list(base), k_nm)
            mnm = self.nonminimal(sample)
            if mnm is None:
                continue
            sc = self.score(mnm)
            if sc < best_score:
                best, best_score = mnm, sc
            mnm = self.lsq_fit(t2, mnm)
            thresh = mult * t2
            den = o.num_lsq_iterations_ - 1
            with np.errstate(divide="ignore", invalid="ignore"):
                upd = float(np.float64((mult - 1.0) * t2) / np.float64(den))
            for _ in range(o.num_lsq_iterations_):
                mnm = self.lsq_fit(thresh, mnm)
                sc = self.score(mnm)
                if sc < best_score:
                    best, best_score = mnm, sc
                thresh -= upd
        return best, best_score

    def run(self):
        o, n, t2 = self.o, self.n, self.t2
        st = dict(num_iterations=0, best_num_inliers=0, inlier_ratio=0.0, number_lo_iterations=0, inliers=[],
                  best_model_score=DBL_MAX)
        zero = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), False)
        best = zero
        if 2 > n:
            return best, st
        pmiss = 1.0 - float(o.success_probability_)
        max_it = max(o.max_num_iterations_, o.min_num_iterations_)
        best_min_score = DBL_MAX
        best_min = zero
        have = False

        def refresh():
            inl = self.inliers(best, t2)
            st["inliers"] = inl
            st["best_num_inliers"] = len(inl)
            st["inlier_ratio"] = len(inl) / n
            return num_required_iterations(st["inlier_ratio"], pmiss, 2, o.min_num_iterations_, o.max_num_iterations_)

        it = 0
        while it < max_it:
            if it == o.lo_starting_iterations_ and best_min_score < DBL_MAX:
                st["number_lo_iterations"] += 1
                best, st["best_model_score"] = self.local_opt(best, st["best_model_score"])
                max_it = refresh()
                have = True
            i0 = self.smp.uniform(n)
            while True:
                i1 = self.smp.uniform(n)
                if i1 != i0:
                    break
            mdl = self.minimal(i0, i1)
            if mdl is None:
                it += 1
                continue
            sc = self.score(mdl)
            loc = sc if sc < DBL_MAX else DBL_MAX
            if loc < best_min_score or it == o.lo_starting_iterations_:
                k_best = loc < best_min_score
                if k_best:
                    best_min_score, best_min = loc, mdl
                    if best_min_score < st["best_model_score"]:
                        st["best_model_score"], best = best_min_score, best_min
                run_lo = it >= o.lo_starting_iterations_ and best_min_score < DBL_MAX
                if not k_best and not run_lo:
                    it += 1
                    continue
                if run_lo:
                    st["number_lo_iterations"] += 1
                    best_min, s2 = self.local_opt(best_min, best_min_score)
                    if s2 < st["best_model_score"]:
                        st["best_model_score"], best = s2, best_min
                max_it = refresh()
                have = True
            it += 1
        st["num_iterations"] = it
        if it <= o.lo_starting_iterations_ and st["best_model_score"] < DBL_MAX:
            st["number_lo_iterations"] += 1
            best, st["best_model_score"] = self.local_opt(best, st["best_model_score"])
            refresh()
            have = True
        if o.final_least_squares_:
            inl = st["inliers"] if have else []
            r = self.nonminimal(list(inl))
            refined = best if r is None else r
            sc = self.score(refined)
            if sc < st["best_model_score"]:
                st["best_model_score"], best = sc, refined
                refresh()
                have = True
        return best, st


def fit_points(pts, opt, t2=None, img_id=-1, line=0):
    """Fit3DPoints: -> dict(start, end, inliers, num_iterations, number_lo_iterations, best_num_inliers, inlier_ratio,
    from_lo)"""
    t2 = opt.squared_inlier_threshold_ if t2 is None else t2
    f = Fitter(pts, opt, t2, img_id, line)
    best, st = f.run()
    out = dict(st)
    out["from_lo"] = bool(best[2]) and len(st["inliers"]) > 0
    inl = st["inliers"]
    if not inl:
        out["start"], out["end"] = np.zeros(3), np.zeros(3)
        return out
    d = best[0]
    P = f.P
    r = P[inl[0]]
    pr = [(float(P[i, 0]) - r[0]) * d[0] + (float(P[i, 1]) - r[1]) * d[1] + (float(P[i, 2]) - r[2]) * d[2] for i in inl]
    # the sums above run ((a + b) + c) left to right, like the device
    lo, hi = min(pr), max(pr)
    out["start"] = np.array([r[0] + d[0] * lo, r[1] + d[1] * lo, r[2] + d[2] * lo])
    out["end"] = np.array([r[0] + d[0] * hi, r[1] + d[1] * hi, r[2] + d[2] * hi])
    return out


def fit_segment(seg4, depth, k4, q4, t3, img_id, line, opt, ransac_th=0.75, min_pct=0.6, var2d=5.0):
    """one segment of lt_fit_segs: -> dict(status, seg (2, 3), kept, inliers, num_iterations, number_lo_iterations,
    from_lo, inlier_list, front)"""
    fh = front_half(seg4, depth, k4, q4, t3, var2d, ransac_th)
    kept = len(fh["depth"])
    if fh["points"] is None:
        return dict(status=STATUS_TOO_FEW, seg=np.zeros((2, 3)), kept=kept, inliers=0, num_iterations=0,
                    number_lo_iterations=0, from_lo=False, inlier_list=[], front=fh)
    r = fit_points(fh["points"], opt, fh["t2"], img_id, line)
    ok = not (r["inlier_ratio"] < min_pct)
    seg = np.stack([r["start"], r["end"]]) if ok else np.zeros((2, 3))
    return dict(status=STATUS_OK if ok else STATUS_LOW_RATIO, seg=seg, kept=kept, inliers=r["best_num_inliers"],
                num_iterations=r["num_iterations"], number_lo_iterations=r["number_lo_iterations"],
                from_lo=r["from_lo"], inlier_list=r["inliers"], front=fh)


def fit_scene(all_2d_segs, cams, depths, opt, ransac_th=0.75, min_pct=0.6, var2d=5.0):
    """fit_3d_segs over a scene: cams img_id -> (k4, q4, t3); -> img_id -> list of fit_segment results"""
    out = {}
    for i in sorted(all_2d_segs):
        segs = np.asarray(all_2d_segs[i], np.float64).reshape(-1, 4) if len(all_2d_segs[i]) else np.zeros((0, 4))
        k4, q4, t3 = cams[i]
        out[i] = [fit_segment(segs[l], depths[i], k4, q4, t3, i, l, opt, ransac_th, min_pct, var2d)
                  for l in range(len(segs))]
    return out
