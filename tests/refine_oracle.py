"""NumPy restatement of limap's own part of the geometric line refinement, written from the
formulas in upstream's operation order and parameterised on the dtype (float64, longdouble).  Paths relative to src/limap:

    base/infinite_line.cc:67-71,180-231,265-287   minimal(), infinite(), cut()
    base/linetrack.cc:315-322                     weights: length / 30
    ceresbase/line_transforms.h:8-29              plucker()
    ceresbase/line_projection.h:14-80             world_to_pixel()
    ceresbase/line_dists.h:19-28, optimize/line_refinement/cost_functions.h:96-127   residual()

Derivatives come from a small dual-number class over the four local directions of the project's retraction
(u + du_i (0, e_i) (x) u, w + dw (-w1, w0)); d|x|/dx = +1 at 0.  exp / log are numpy's in the working dtype.
"""
import numpy as np

EPS = 1e-12
CAUCHY_B = 0.0625


class Dual:
    """value + derivative along 4 directions"""
    __array_priority__ = 100

    def __init__(self, v, d=None, dtype=np.float64):
        self.v = dtype(v)
        self.d = np.zeros(4, dtype) if d is None else np.asarray(d, dtype)
        self.dtype = dtype

    def _c(self, o):
        return o if isinstance(o, Dual) else Dual(o, None, self.dtype)

    def __add__(self, o):
        o = self._c(o)
        return Dual(self.v + o.v, self.d + o.d, self.dtype)
    __radd__ = __add__

    def __sub__(self, o):
        o = self._c(o)
        return Dual(self.v - o.v, self.d - o.d, self.dtype)

    def __rsub__(self, o):
        return self._c(o) - self

    def __neg__(self):
        return Dual(-self.v, -self.d, self.dtype)

    def __mul__(self, o):
        o = self._c(o)
        return Dual(self.v * o.v, self.v * o.d + self.d * o.v, self.dtype)
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = self._c(o)
        q = self.v / o.v
        return Dual(q, (self.d - q * o.d) / o.v, self.dtype)

    def __rtruediv__(self, o):
        return self._c(o) / self


def val(x):
    return x.v if isinstance(x, Dual) else x


def _sqrt(x):
    if isinstance(x, Dual):
        s = np.sqrt(x.v)
        return Dual(s, x.d / (2 * s), x.dtype)
    return np.sqrt(x)


def _abs(x):
    if isinstance(x, Dual):
        return -x if x.v < 0 else x
    return np.abs(x)


def _exp(x):
    if isinstance(x, Dual):
        e = np.exp(x.v)
        return Dual(e, e * x.d, x.dtype)
    return np.exp(x)


def quat_to_rot_ceres(q):
    """ceres::QuaternionToRotation: the scaled rotation, then the division by the squared norm; row-major 9"""
    a, b, c, d = q
    aa, ab, ac, ad, bb, bc, bd, cc, cd, dd = a * a, a * b, a * c, a * d, b * b, b * c, b * d, c * c, c * d, d * d
    R = [aa + bb - cc - dd, 2 * (bc - ad), 2 * (ac + bd), 2 * (ad + bc), aa - bb + cc - dd, 2 * (cd - ab),
         2 * (bd - ac), 2 * (ab + cd), aa - bb - cc + dd]
    n = 1 / (aa + bb + cc + dd)
    return [r * n for r in R]


def plucker(u, w, dtype):
    R = quat_to_rot_ceres(u)
    w1, w2 = _abs(w[0]), _abs(w[1])
    d = [R[0], R[3], R[6]]
    bn = w2 / (w1 + dtype(EPS))
    return d, [R[1] * bn, R[4] * bn, R[7] * bn]


def _mat3(rows):
    return [[rows[3 * i + j] for j in range(3)] for i in range(3)]


def _mm(A, B):
    return [[A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]


def _T(A):
    return [[A[j][i] for j in range(3)] for i in range(3)]


def _skew(m, zero):
    return [[zero, -m[2], m[1]], [m[2], zero, -m[0]], [-m[1], m[0], zero]]


def world_to_pixel(kvec, qvec, tvec, d, m, dtype):
    zero = dtype(0)
    R = _mat3(quat_to_rot_ceres([dtype(x) for x in qvec]))
    t = [dtype(x) for x in tvec]
    Rd = [R[i][0] * d[0] + R[i][1] * d[1] + R[i][2] * d[2] for i in range(3)]
    RmR = _mm(_mm(R, _skew(m, zero)), _T(R))
    M = [[RmR[i][j] - t[i] * Rd[j] + Rd[i] * t[j] for j in range(3)] for i in range(3)]
    mt = [M[2][1], M[0][2], M[1][0]]
    fx, fy, cx, cy = [dtype(x) for x in kvec]
    one = dtype(1)
    K = [[fx, zero, cx], [zero, fy, cy], [zero, zero, one]]
    C = _mm(_mm(K, _skew(mt, zero)), _T(K))
    c = [C[2][1], C[0][2], C[1][0]]
    n = _sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2] + dtype(EPS))
    return [c[0] / n, c[1] / n, c[2] / n]


def cosine2d(a, b, dtype):
    n1 = _sqrt(a[0] * a[0] + a[1] * a[1] + dtype(EPS))
    n2 = _sqrt(b[0] * b[0] + b[1] * b[1] + dtype(EPS))
    c = _abs((a[0] * b[0] + a[1] * b[1]) / (n1 * n2))
    if isinstance(c, Dual):
        return Dual(1, None, dtype) if c.v > 1 else c
    return np.minimum(c, 1)


def residual(cam11, seg4, u, w, alpha, dtype):
    """the two residuals of one support; u, w: lists of dtype scalars or Duals"""
    d, m = plucker(u, w, dtype)
    coor = world_to_pixel(cam11[:4], cam11[4:8], cam11[8:11], d, m, dtype)
    p1 = [dtype(seg4[0]), dtype(seg4[1])]
    p2 = [dtype(seg4[2]), dtype(seg4[3])]
    dn = _sqrt(coor[0] * coor[0] + coor[1] * coor[1] + dtype(EPS))
    dir2d = [-coor[1] / dn, coor[0] / dn]
    direc = [p2[0] - p1[0], p2[1] - p1[1]]
    cos = cosine2d(dir2d, direc, dtype)
    wgt = _exp(dtype(alpha) * (dtype(1) - cos))
    d1 = (p1[0] * coor[0] + p1[1] * coor[1] + coor[2]) / dn
    d2 = (p2[0] * coor[0] + p2[1] * coor[1] + coor[2]) / dn
    return [d1 * wgt, d2 * wgt]


def normalise_q(q, dtype):
    q = np.asarray(q, dtype)
    return q / np.sqrt((q[0] * q[0] + q[2] * q[2]) + (q[1] * q[1] + q[3] * q[3]))


def cams_normalised(cam11, dtype):
    """CameraPose's constructor normalises its quaternion once (camera.h:94-95)"""
    c = np.asarray(cam11, dtype).copy()
    for r in c:
        r[4:8] = normalise_q(r[4:8], dtype)
    return c


def seeds(p, dtype):
    q0, q1, q2, q3, w0, w1 = [dtype(x) for x in p]
    z = dtype(0)
    u = [Dual(q0, [-q1, -q2, -q3, z], dtype), Dual(q1, [q0, q3, -q2, z], dtype), Dual(q2, [-q3, q0, q1, z], dtype),
         Dual(q3, [q2, -q1, q0, z], dtype)]
    w = [Dual(w0, [z, z, z, -w1], dtype), Dual(w1, [z, z, z, w0], dtype)]
    return u, w


def evaluate(cam11, segs4, p, alpha=10.0, dtype=np.float64):
    """residuals (2K), cost, g (4), H (4, 4) of one track at the minimal parameters p; supports in residual order"""
    cams = cams_normalised(cam11, dtype)
    u, w = seeds(p, dtype)
    K = len(segs4)
    r = np.zeros(2 * K, dtype)
    g = np.zeros(4, dtype)
    H = np.zeros((4, 4), dtype)
    cost = dtype(0)
    b = dtype(CAUCHY_B)
    for k in range(K):
        s = [dtype(x) for x in segs4[k]]
        rr = residual(cams[k], s, u, w, alpha, dtype)
        wk = np.sqrt((s[0] - s[2]) ** 2 + (s[1] - s[3]) ** 2) / dtype(30)
        sq = rr[0].v * rr[0].v + rr[1].v * rr[1].v
        cost = cost + wk * b * np.log(dtype(1) + sq / b)
        rho1 = wk / (dtype(1) + sq / b)
        J = np.stack([rr[0].d, rr[1].d])
        rv = np.array([rr[0].v, rr[1].v], dtype)
        H += rho1 * (J.T @ J)
        g += rho1 * (J.T @ rv)
        r[2 * k], r[2 * k + 1] = rv
    return r, cost / dtype(2), g, H


def cost_only(cam11n, segs4, p, alpha=10.0):
    """float64 cost at p = (u4, w2), the supports as array lanes of the same expressions (cameras already
    normalised); for scipy"""
    arr = lambda x: np.asarray(x, np.float64)  # noqa: E731
    cam, sg = np.asarray(cam11n, float).T, np.asarray(segs4, float).T
    rr = residual(cam, sg, [np.float64(x) for x in p[:4]], [np.float64(x) for x in p[4:]], alpha, arr)
    wk = np.sqrt((sg[0] - sg[2]) ** 2 + (sg[1] - sg[3]) ** 2) / 30.0
    return 0.5 * float((wk * CAUCHY_B * np.log1p((rr[0] * rr[0] + rr[1] * rr[1]) / CAUCHY_B)).sum())


def retract(p, dl):
    q0, q1, q2, q3 = p[:4]
    r = np.array([q0 - dl[0] * q1 - dl[1] * q2 - dl[2] * q3, q1 + dl[0] * q0 + dl[1] * q3 - dl[2] * q2,
                  q2 - dl[0] * q3 + dl[1] * q0 + dl[2] * q1, q3 + dl[0] * q2 - dl[1] * q1 + dl[2] * q0])
    w = np.array([p[4] - dl[3] * p[5], p[5] + dl[3] * p[4]])
    return np.concatenate([r / np.linalg.norm(r), w / np.linalg.norm(w)])


# ---- conversions (float64, upstream's order) ----
def rot_to_quat_eigen(m):
    """Eigen's Quaternion(Matrix3): (w, x, y, z)"""
    t = m[0, 0] + m[1, 1] + m[2, 2]
    q = np.zeros(4)  # x y z w
    if t > 0:
        t = np.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (m[2, 1] - m[1, 2]) * t
        q[1] = (m[0, 2] - m[2, 0]) * t
        q[2] = (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (m[k, j] - m[j, k]) * t
        q[j] = (m[j, i] + m[i, j]) * t
        q[k] = (m[k, i] + m[i, k]) * t
    return np.array([q[3], q[0], q[1], q[2]])


def quat_to_rot_eigen(q):
    q = np.asarray(q, float)
    n = np.sqrt((q[0] * q[0] + q[2] * q[2]) + (q[1] * q[1] + q[3] * q[3]))  # Eigen's 4-vector norm, as lt_geom.h takes it
    w, x, y, z = q / n if n != 0 else np.array([1.0, q[1], q[2], q[3]])
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _n3(v):
    return np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def minimal(line6):
    s, e = np.asarray(line6[:3], float), np.asarray(line6[3:], float)
    a = (e - s) / _n3(e - s)
    b = np.cross(s, a)
    bn = _n3(b)
    den = np.sqrt(1.0 + bn * bn)
    w = np.array([1.0 / den, bn / den])
    Q = np.zeros((3, 3))
    Q[:, 0] = a / _n3(a)
    if bn > EPS:
        Q[:, 1] = b / bn
        axb = np.cross(a, b)
    else:
        best = 0
        if abs(a[1]) > abs(a[0]):
            best = 1
        if abs(a[2]) > abs(a[best]):
            best = 2
        i1, i2 = (best + 1) % 3, (best + 2) % 3
        bp = np.zeros(3)
        bp[i1] = bp[i2] = 1.0
        bp[best] = -(a[i1] + a[i2]) / a[best]
        Q[:, 1] = bp / _n3(bp)
        axb = np.cross(a, bp)
    Q[:, 2] = axb / _n3(axb)
    return np.concatenate([rot_to_quat_eigen(Q), w])


def infinite(p):
    Q = quat_to_rot_eigen(p[:4])
    return Q[:, 0], abs(p[5]) / abs(p[4]) * Q[:, 1]


def cut(p, line3d6, num_outliers):
    """GetLineSegmentFromInfiniteLine3d over the line3d list (K, 6): sorted() of the 2K values"""
    d, m = infinite(p)
    q = np.asarray(line3d6[0][:3], float)
    pref = q + np.cross(d, m + np.cross(d, q))
    vals = []
    for l in line3d6:
        for e in (l[:3], l[3:]):
            x = np.asarray(e, float) - pref
            vals.append((x[0] * d[0] + x[1] * d[1]) + x[2] * d[2])
    vals = sorted(vals)
    a, b = vals[num_outliers], vals[2 * len(line3d6) - 1 - num_outliers]
    return np.concatenate([pref + d * a, pref + d * b])


def residual_order(img_ids):
    """AddLineGeometricResiduals: sorted image ids, the id map's order within an image"""
    return np.argsort(np.asarray(img_ids), kind="stable")
