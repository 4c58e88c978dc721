"""A slow, literal NumPy / Python restatement of the vanishing-point detector: DESIGN.md section 18 (hypotheses,
consistency, clustering) plus the reference's own tail in the reference's operation order (vplib/JLinkage/JLinkage.cc,
vplib/base_vp_detector.cc, base/infinite_line.cc, base/linebase.{h,cc}, base/graph.cc:157-166 and the JacobiSVD
procedure of Eigen 3.4 as the stand-in headers of oracle/ref_shim carry it).  It includes no product code.  NumPy's
elementwise FP64 operations are IEEE and never fused, so every expression below has one value.

The clustering keeps the full matrix of pair ratios and takes its first maximum in row-major order at every step: the
definition, not the product's nearest-partner bookkeeping.  Two ratios c/u with u <= 2^21 that differ, differ by more
than 2^-42 relatively, so their FP64 quotients order exactly as the fractions do and equal fractions give equal quotients.
"""
import math

import numpy as np

EPS = 1e-12  # util/types.h:34
TH_PERP_USED = 3.0  # count_valid_supports_2d reads BaseVPDetector::config_, which JLinkage's constructors never fill
M64 = (1 << 64) - 1
DEFAULTS = dict(min_length=40.0, inlier_threshold=1.0, min_num_supports=5, th_perp_supports=3.0, num_hypotheses=5000,
                seed=0)


def config(d=None):
    """ASSIGN_PYDICT_ITEM: present keys overwrite, unknown keys are ignored"""
    c = dict(DEFAULTS)
    for k in c:
        if d and k in d:
            c[k] = type(c[k])(d[k])
    return c


def lengths(lines):
    dx, dy = lines[:, 0] - lines[:, 2], lines[:, 1] - lines[:, 3]
    return np.sqrt(dx * dx + dy * dy)


def sample(seed, m, n):
    """splitmix64 of seed * K + m -> (a, b), two distinct valid lines"""
    z = (seed * 0x9E3779B97F4A7C15 + m) & M64
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    hi, lo = z >> 32, z & 0xFFFFFFFF
    a = hi % n
    return a, (a + 1 + lo % (n - 1)) % n


def preference(lines_valid, cfg):
    """(n, M) bool: line k is consistent with hypothesis m"""
    e = lines_valid.astype(np.float32).astype(np.float64)
    x1, y1, x2, y2 = e[:, 0], e[:, 1], e[:, 2], e[:, 3]
    cx, cy = (x1 + x2) * 0.5, (y1 + y2) * 0.5
    h0, h1, h2 = y1 - y2, x2 - x1, x1 * y2 - y1 * x2
    n, M = e.shape[0], cfg["num_hypotheses"]
    ab = np.array([sample(cfg["seed"], m, n) for m in range(M)], np.int64).reshape(M, 2)
    a, b = ab[:, 0], ab[:, 1]
    v0 = h1[a] * h2[b] - h2[a] * h1[b]
    v1 = h2[a] * h0[b] - h0[a] * h2[b]
    v2 = h0[a] * h1[b] - h1[a] * h0[b]
    out = np.zeros((n, M), bool)
    with np.errstate(all="ignore"):
        for k0 in range(0, n, 256):
            s = slice(k0, k0 + 256)
            l0 = cy[s, None] * v2[None, :] - v1[None, :]
            l1 = v0[None, :] - cx[s, None] * v2[None, :]
            l2 = cx[s, None] * v1[None, :] - cy[s, None] * v0[None, :]
            err = np.abs((l0 * x1[s, None] + l1 * y1[s, None]) + l2) / np.sqrt(l0 * l0 + l1 * l1)
            out[s] = err <= cfg["inlier_threshold"]
    return out


def cluster(pref):
    """pref: (n, M) bool.  Returns per row the id of its cluster (the smallest row index of the cluster)."""
    pref = np.array(pref, bool)
    n = pref.shape[0]
    ids = np.arange(n)
    if n < 2:
        return ids
    B = pref.astype(np.float64)
    inter = B @ B.T  # exact: counts below 2^53
    size = pref.sum(1).astype(np.float64)
    alive = np.ones(n, bool)
    upper = np.triu(np.ones((n, n), bool), 1)

    def ratios(rows_inter, rows_size, cols_size):
        with np.errstate(all="ignore"):
            r = rows_inter / (rows_size + cols_size - rows_inter)
        return np.where(rows_inter > 0, r, -1.0)

    R = np.where(upper, ratios(inter, size[:, None], size[None, :]), -1.0)
    while True:
        flat = int(np.argmax(R))  # the first maximum in row-major order: smallest i, then smallest j
        i, j = divmod(flat, n)
        if not R[i, j] > 0:
            break
        pref[i] &= pref[j]
        alive[j] = False
        ids[ids == j] = i
        size[i] = pref[i].sum()
        R[j, :] = -1.0
        R[:, j] = -1.0
        c = (B[:, pref[i]]).sum(1) if pref[i].any() else np.zeros(n)
        B[i] = pref[i]
        r = np.where(alive, ratios(c, size[i], size), -1.0)
        r[i] = -1.0
        R[i, i + 1:] = r[i + 1:]
        R[:i, i] = r[:i]
    return ids


# ---- the reference's tail ----------------------------------------------------------------------------------------------
def _unit(v):
    z = v[..., 0] * v[..., 0]
    if v.shape[-1] == 2:
        z = z + v[..., 1] * v[..., 1]
    else:
        z = (z + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]  # the shim's 3-vector order: (x0 + x1) + x2
    with np.errstate(all="ignore"):
        out = v / np.sqrt(z)[..., None]
    return np.where((z > 0)[..., None], out, v)


def coords(lines):
    """Line2d::coords(): homogeneous(start).cross(homogeneous(end)).normalized()"""
    sx, sy, ex, ey = lines[..., 0], lines[..., 1], lines[..., 2], lines[..., 3]
    one = np.ones_like(sx)
    return _unit(np.stack([sy * one - one * ey, one * ex - sx * one, sx * ey - sy * ex], -1))


def inf_line_distance(line, q):
    """InfiniteLine2d(line).point_distance(q), elementwise over leading axes; raises where the reference throws"""
    co = coords(line)
    direc = _unit(np.stack([co[..., 1], -co[..., 0]], -1))
    dp = np.stack([direc[..., 1], -direc[..., 0]], -1)
    if not np.all(np.abs(np.sqrt(dp[..., 0] * dp[..., 0] + dp[..., 1] * dp[..., 1]) - 1.0) < EPS):
        raise ValueError("THROW_CHECK_LT(std::abs(direc.norm() - 1.0), EPS)")
    cp = _unit(np.stack([dp[..., 1], (-1) * dp[..., 0], (-1) * dp[..., 1] * q[..., 0] + dp[..., 0] * q[..., 1]], -1))
    px = co[..., 1] * cp[..., 2] - co[..., 2] * cp[..., 1]
    py = co[..., 2] * cp[..., 0] - co[..., 0] * cp[..., 2]
    pz = co[..., 0] * cp[..., 1] - co[..., 1] * cp[..., 0]
    if not np.all(pz > EPS):
        raise ValueError("THROW_CHECK_GT(p_homo(2), EPS)")
    ux, uy = q[..., 0] - px / (pz + EPS), q[..., 1] - py / (pz + EPS)
    return np.sqrt(ux * ux + uy * uy)


def _root(k, parents):  # union_find_get_root, with its path compression
    if parents[k] == -1:
        return k
    parents[k] = _root(parents[k], parents)
    return parents[k]


def count_valid_supports_2d(lines, th=TH_PERP_USED):
    n = lines.shape[0]
    if n == 0:
        return 0
    ln = lengths(lines)
    ii, jj = np.triu_indices(n, 1)
    swap = ln[ii] > ln[jj]  # the shorter line (k1) is projected on the longer one (k2)
    k1, k2 = np.where(swap, jj, ii), np.where(swap, ii, jj)
    if ii.size and not np.all(ln[k2] > 0):
        raise ValueError("CHECK_GT(line.length(), 0.0)")
    dist = np.zeros((n, n))
    if ii.size:
        ds = inf_line_distance(lines[k2], lines[k1][:, 0:2])
        de = inf_line_distance(lines[k2], lines[k1][:, 2:4])
        dist[ii, jj] = np.where(ds < de, de, ds)  # std::max(ds, de)
    parents = [-1] * n
    import sys
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 4 * n + 1000))
    for i in range(n - 1):
        root_i = _root(i, parents)
        for j in range(i + 1, n):
            root_j = _root(j, parents)
            if root_j == root_i:
                continue
            if dist[i, j] > th:
                continue
            parents[root_j] = root_i
    return sum(1 for p in parents if p == -1)


# ---- Eigen 3.4's JacobiSVD<MatrixXd>(A, ComputeThinV).matrixV() for rows >= cols ---------------------------------------
DBL_MIN, DBL_EPS = 2.2250738585072014e-308, 2.220446049250313e-16


def _make_jacobi(x, y, z):
    deno = 2.0 * abs(y)
    if deno < DBL_MIN:
        return 1.0, 0.0
    tau = (x - z) / deno
    w = math.sqrt(tau * tau + 1.0)
    t = 1.0 / (tau + w) if tau > 0.0 else 1.0 / (tau - w)
    sign_t = 1.0 if t > 0.0 else -1.0
    nn = 1.0 / math.sqrt(t * t + 1.0)
    return nn, -sign_t * (y / abs(y)) * abs(t) * nn


def _svd2x2(m00, m01, m10, m11):
    t, d = m00 + m11, m10 - m01
    if abs(d) < DBL_MIN:
        c1, s1 = 1.0, 0.0
    else:
        u = t / d
        tmp = math.sqrt(1.0 + u * u)
        s1, c1 = 1.0 / tmp, u / tmp
    if not (c1 == 1.0 and s1 == 0.0):
        a0, a1, b0, b1 = m00, m01, m10, m11
        m00, m01 = c1 * a0 + s1 * b0, c1 * a1 + s1 * b1
        m10, m11 = -s1 * a0 + c1 * b0, -s1 * a1 + c1 * b1
    rc, rs = _make_jacobi(m00, m01, m11)
    oc, os_ = rc, -rs
    return (c1 * oc - s1 * os_, c1 * os_ + s1 * oc), (rc, rs)


def _colpiv_qr(qr):
    rows, cols = len(qr), len(qr[0])
    size = min(rows, cols)

    def col_norm(j, r0):
        s = 0.0
        for i in range(r0, rows):
            s += qr[i][j] * qr[i][j]
        return math.sqrt(s)

    upd = [col_norm(k, 0) for k in range(cols)]
    dire = list(upd)
    transp = [0] * cols
    thr = math.sqrt(DBL_EPS)
    tmp = [0.0] * cols
    for k in range(size):
        big = k
        for j in range(k + 1, cols):
            if upd[j] > upd[big]:
                big = j
        transp[k] = big
        if k != big:
            for i in range(rows):
                qr[i][k], qr[i][big] = qr[i][big], qr[i][k]
            upd[k], upd[big] = upd[big], upd[k]
            dire[k], dire[big] = dire[big], dire[k]
        tail_sq = 0.0
        for i in range(k + 1, rows):
            tail_sq += qr[i][k] * qr[i][k]
        c0 = qr[k][k]
        if tail_sq <= DBL_MIN:
            tau, beta = 0.0, c0
            for i in range(k + 1, rows):
                qr[i][k] = 0.0
        else:
            beta = math.sqrt(c0 * c0 + tail_sq)
            if c0 >= 0.0:
                beta = -beta
            den = c0 - beta
            for i in range(k + 1, rows):
                qr[i][k] = qr[i][k] / den
            tau = (beta - c0) / beta
        qr[k][k] = beta
        if cols - k - 1 > 0:
            if rows - k == 1:
                for j in range(k + 1, cols):
                    qr[k][j] *= 1.0 - tau
            elif tau != 0.0:
                for j in range(k + 1, cols):
                    t = 0.0
                    for i in range(k + 1, rows):
                        t += qr[i][k] * qr[i][j]
                    tmp[j] = t + qr[k][j]
                for j in range(k + 1, cols):
                    qr[k][j] -= tau * tmp[j]
                for j in range(k + 1, cols):
                    for i in range(k + 1, rows):
                        qr[i][j] -= (tau * qr[i][k]) * tmp[j]
        for j in range(k + 1, cols):
            if upd[j] != 0.0:
                temp = abs(qr[k][j]) / upd[j]
                temp = (1.0 + temp) * (1.0 - temp)
                temp = 0.0 if temp < 0.0 else temp
                ratio = upd[j] / dire[j]
                temp2 = temp * (ratio * ratio)
                if temp2 <= thr:
                    dire[j] = col_norm(j, k + 1)
                    upd[j] = dire[j]
                else:
                    upd[j] *= math.sqrt(temp)
    perm = list(range(cols))
    for k in range(size):
        perm[k], perm[transp[k]] = perm[transp[k]], perm[k]
    return perm


def jacobi_svd_v(A):
    """A: rows x cols with rows >= cols -> V (cols x cols, list of rows), columns sorted by singular value"""
    rows, cols = A.shape
    assert rows >= cols
    n = cols
    scale = 0.0
    for x in A.ravel(order="F"):
        ax = abs(float(x))
        if not ax <= scale:
            scale = ax
    if not math.isfinite(scale):
        raise ValueError("non-finite matrix")
    if scale == 0.0:
        scale = 1.0
    V = [[0.0] * n for _ in range(n)]
    if rows > cols:
        qr = [[float(A[i, j]) / scale for j in range(cols)] for i in range(rows)]
        perm = _colpiv_qr(qr)
        w = [[qr[i][j] if i <= j else 0.0 for j in range(n)] for i in range(n)]
        for i in range(cols):
            V[perm[i]][i] = 1.0
    else:
        w = [[float(A[i, j]) / scale for j in range(n)] for i in range(n)]
        for i in range(n):
            V[i][i] = 1.0
    max_diag = 0.0
    for i in range(n):
        max_diag = abs(w[i][i]) if abs(w[i][i]) > max_diag else max_diag
    precision = 2.0 * DBL_EPS

    def rot_rows(M, p, q, c, s, width):  # x = row p, y = row q
        if c == 1.0 and s == 0.0:
            return
        for k in range(width):
            xi, yi = M[p][k], M[q][k]
            M[p][k] = c * xi + s * yi
            M[q][k] = -s * xi + c * yi

    def rot_cols(M, p, q, c, s, height):
        if c == 1.0 and s == 0.0:
            return
        for k in range(height):
            xi, yi = M[k][p], M[k][q]
            M[k][p] = c * xi + s * yi
            M[k][q] = -s * xi + c * yi

    finished = False
    while not finished:
        finished = True
        for p in range(1, n):
            for q in range(p):
                pm = precision * max_diag
                threshold = DBL_MIN if DBL_MIN > pm else pm
                if abs(w[p][q]) > threshold or abs(w[q][p]) > threshold:
                    finished = False
                    (lc, ls), (rc, rs) = _svd2x2(w[p][p], w[p][q], w[q][p], w[q][q])
                    rot_rows(w, p, q, lc, ls, n)
                    rot_cols(w, p, q, rc, -rs, n)
                    rot_cols(V, p, q, rc, -rs, cols)
                    dp, dq = abs(w[p][p]), abs(w[q][q])
                    m2 = dp if dp > dq else dq
                    max_diag = max_diag if max_diag > m2 else m2
    sv = [abs(w[i][i]) * scale for i in range(n)]
    for i in range(n):
        pos = i
        for k in range(i + 1, n):
            if sv[k] > sv[pos]:
                pos = k
        if sv[pos] == 0.0:
            break
        if pos != i:
            sv[i], sv[pos] = sv[pos], sv[i]
            for r in range(cols):
                V[r][i], V[r][pos] = V[r][pos], V[r][i]
    return V


def fit_vp(lines):
    """fitVP: the third right singular vector of the rows coords(), normalised"""
    if lines.shape[0] < 3:
        raise ValueError("fitVP needs three lines")
    V = jacobi_svd_v(coords(lines))
    return _unit(np.array([V[0][2], V[1][2], V[2][2]]))


def tail(lines, valid_ids, labels_valid, cfg):
    """ComputeVPLabels after the two library calls (JLinkage.cc:55-83) and AssociateVPs (:102-127).  labels_valid: the
    library's Labels (one per valid line), None when the guard returned early.  -> (labels, vps)"""
    n_lines = lines.shape[0]
    final = np.full(n_lines, -1, np.int64)
    if n_lines == 0 or labels_valid is None:
        return final, np.zeros((0, 3))
    n_labels = int(labels_valid.max()) + 1 if len(labels_valid) else 0
    supports = [[] for _ in range(n_labels)]
    for k, lab in enumerate(labels_valid):
        supports[lab].append(valid_ids[k])
    vp_ids, counter = [-1] * n_labels, 0
    for c in range(n_labels):
        if len(supports[c]) < cfg["min_num_supports"]:
            continue
        if count_valid_supports_2d(lines[supports[c]]) < cfg["min_num_supports"]:
            continue
        vp_ids[c] = counter
        counter += 1
    for k, lab in enumerate(labels_valid):
        if vp_ids[lab] >= 0:
            final[valid_ids[k]] = vp_ids[lab]
    n_vps = int(final.max()) + 1
    vps = np.zeros((n_vps, 3))
    for v in range(n_vps):
        vps[v] = fit_vp(lines[final == v])
    return final, vps


def valid_lines(lines, cfg):
    """the ids that pass `length() < min_length`, and whether the guard lets the image through"""
    ids = np.nonzero(~(lengths(lines) < cfg["min_length"]))[0]
    return ids, not (len(ids) < 2 * max(cfg["min_num_supports"], 10))


def renumber(ids):
    """cluster ids -> Labels: the clusters renumbered in ascending id"""
    return np.unique(ids, return_inverse=True)[1].astype(np.int64) if len(ids) else np.zeros(0, np.int64)


def detect(lines, cfg=None):
    """The whole detector on one image.  -> dict(labels (n_lines,), vps (V, 3), clusters (n_lines,))"""
    cfg = config(cfg)
    lines = np.asarray(lines, np.float64).reshape(-1, 4)
    clusters = np.full(lines.shape[0], -1, np.int64)
    if lines.shape[0] == 0:
        return dict(labels=clusters.copy(), vps=np.zeros((0, 3)), clusters=clusters)
    ids, go = valid_lines(lines, cfg)
    lab = None
    if go:
        lab = renumber(cluster(preference(lines[ids], cfg)))
        clusters[ids] = lab
    labels, vps = tail(lines, ids, lab, cfg)
    return dict(labels=labels, vps=vps, clusters=clusters)


def recovery(dirs, labels, vps, K, R):
    """Manhattan scenes: per true direction d (column d of R, camera frame) the vanishing point most of its lines carry,
    the angle in degrees between K^-1 vp and the direction, and the share of the direction's lines with that label.
    Plain Python floats in a fixed order."""
    out = []
    for d in range(3):
        mine = np.asarray(labels)[np.asarray(dirs) == d]
        lab = mine[mine >= 0]
        if lab.size == 0:
            out.append(dict(vp=-1, angle_deg=-1.0, share=0.0))
            continue
        v = int(np.bincount(lab).argmax())
        p = [float(x) for x in vps[v]]
        g = [(p[0] - float(K[0][2]) * p[2]) / float(K[0][0]), (p[1] - float(K[1][2]) * p[2]) / float(K[1][1]), p[2]]
        nrm = math.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
        cosang = abs((g[0] * float(R[0][d]) + g[1] * float(R[1][d])) + g[2] * float(R[2][d])) / nrm
        out.append(dict(vp=v, angle_deg=math.degrees(math.acos(min(1.0, cosang))),
                        share=float(int((mine == v).sum())) / float(mine.size)))
    return out
