"""NumPy restatement of the global point-line association: limap's own part -- the four
association residuals of GlobalAssociator with their weights, losses and SetUp switches, in upstream's operation order,
on any dtype -- and the project's linear solve as a straight loop.  Paths relative to src/limap:

    optimize/global_pl_association/cost_functions.h:105-199    edge_residual()
    ceresbase/line_dists.h:40-78                               sine(), cosine()
    optimize/global_pl_association/global_associator.cc:176-305   setup(): switches, weights, edge order
    optimize/global_pl_association/global_associator.cc:452-504   vp_pairs()

R1.1 and R1.2 are ba_oracle's blocks with the camera a constant.  Derivatives come from refine_oracle's dual-number class
along the project's charts: p + dp, section 19's line chart, and the vanishing point's tangent basis (vp_basis).
"""
import numpy as np

import ba_oracle as bo
import refine_oracle as ro
from refine_oracle import Dual, EPS, CAUCHY_B

HUBER_A = 0.01
PL, VL, ORTH, COLL = 0, 1, 2, 3


def cross(x, y):
    return [x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0]]


def _unit2(a, b, dtype):
    n1 = ro._sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2] + dtype(EPS))
    n2 = ro._sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2] + dtype(EPS))
    return [x / n1 for x in a], [x / n2 for x in b]


def _clamp1(x, dtype):
    if isinstance(x, Dual):
        return Dual(1, None, dtype) if x.v > 1 else x
    return np.minimum(x, 1)


def sine(a, b, dtype):
    an, bn = _unit2(a, b, dtype)
    c = cross(an, bn)
    return _clamp1(ro._sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2] + dtype(EPS)), dtype)


def cosine(a, b, dtype):
    an, bn = _unit2(a, b, dtype)
    c = dtype(0) + an[0] * bn[0] + an[1] * bn[1] + an[2] * bn[2]
    return _clamp1(ro._abs(c), dtype)


def edge_residual(kind, pa, pb, dtype):
    """the residuals of an edge (a list of 3 or 1) at the parameters of its two unknowns: lists of scalars or Duals"""
    if kind == PL:
        d, m = ro.plucker(pb[:4], pb[4:], dtype)
        bp = cross(d, pa)
        bp = [bp[i] + m[i] for i in range(3)]
        disp = cross(d, bp)
        return [disp[i] + dtype(EPS) for i in range(3)]
    if kind == VL:
        d, _ = ro.plucker(pb[:4], pb[4:], dtype)
        return [sine(d, pa, dtype)]
    if kind == ORTH:
        return [cosine(pa, pb, dtype)]
    return [sine(pa, pb, dtype)]


def edge_rho(kind, w, sq, dtype=np.float64):
    """ScaledLoss(HuberLoss(0.01) | TrivialLoss, w): rho and rho'"""
    w = dtype(w)
    if kind >= ORTH:
        return w * sq, w
    a = dtype(HUBER_A)
    b = a * a
    if sq > b:
        r = np.sqrt(sq)
        return w * (dtype(2) * a * r - b), w * (a / r)
    return w * sq, w


def vp_basis(v):
    v = np.asarray(v)
    k = int(np.argmin(np.abs(v)))  # the first among equals
    e = np.zeros(3, v.dtype)
    e[k] = 1
    c = np.cross(v, e)
    c[k] = 0
    b1 = c / np.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2])
    return b1, np.array(cross(v, b1), v.dtype)


def vp_retract(v, dl):
    b1, b2 = vp_basis(v)
    t = v + dl[0] * b1 + dl[1] * b2
    return t / np.sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2])


def retract(kind, p, dl):
    """kind 0 point, 1 line, 2 VP"""
    if kind == 1:
        return ro.retract(p, dl)
    if kind == 2:
        return vp_retract(np.asarray(p[:3], float), dl)
    return np.asarray(p[:3], float) + np.asarray(dl[:3], float)


def seeds(kind, p, dtype):
    if kind == 1:
        u, w = ro.seeds(p, dtype)
        return u + w
    if kind == 2:
        v = np.array([dtype(x) for x in p[:3]], dtype)
        b1, b2 = vp_basis(v)
        z = dtype(0)
        return [Dual(v[i], [b1[i], b2[i], z, z], dtype) for i in range(3)]
    return [Dual(p[i], np.eye(4)[i], dtype) for i in range(3)]


def consts(p, dtype):
    return [Dual(x, None, dtype) for x in p]


# ---- SetUp ----
DEFAULTS = dict(lw_point=0.1, lw_pointline_association=10.0, lw_vpline_association=1.0, lw_vp_orthogonality=1.0,
                lw_vp_collinearity=0.0, min_num_images=4, constant_point=False, constant_line=False, constant_vp=False,
                enable_pointline=True, enable_vpline=True, geometric_alpha=10.0)


def setup(s, **kw):
    """the problem SetUp builds from the scene: R1 blocks (ba_oracle's dicts), edges (kind, a, b as unknown indices, w the
    ScaledLoss weight), and nd per unknown (0: constant); unknowns in the order points, lines, VPs"""
    c = dict(DEFAULTS, **kw)
    NP, NL, NV = len(s["poff"]) - 1, len(s["loff"]) - 1, len(s["vp3"])
    row = {int(i): n for n, i in enumerate(s["img_ids"])}
    cpt, cln, cvp = c["constant_point"], c["constant_line"], c["constant_vp"]
    blks, few = [], []
    if not cpt and c["lw_point"] > 0:
        for n in range(NP):
            for i in range(int(s["poff"][n]), int(s["poff"][n + 1])):
                blks.append(dict(kind=0, row=row[int(s["pimg"][i])], s=n, obs=s["pxy"][i], w=c["lw_point"]))
    for n in range(NL):
        a, b = int(s["loff"][n]), int(s["loff"][n + 1])
        few.append(len(set(int(x) for x in s["limg"][a:b])) < c["min_num_images"])
        if cln:
            continue
        for i in np.argsort(s["limg"][a:b], kind="stable") + a:
            sg = s["l2d"][i]
            blks.append(dict(kind=1, row=row[int(s["limg"][i])], s=NP + n, obs=sg,
                             w=np.sqrt((sg[2] - sg[0]) * (sg[2] - sg[0]) + (sg[3] - sg[1]) * (sg[3] - sg[1])) / 30.0))
    on = {PL: c["enable_pointline"] and (not cpt or not cln) and c["lw_pointline_association"] > 0,
          VL: c["enable_vpline"] and (not cvp or not cln) and c["lw_vpline_association"] > 0,
          ORTH: c["enable_vpline"] and not cvp and c["lw_vp_orthogonality"] > 0,
          COLL: c["enable_vpline"] and not cvp and c["lw_vp_collinearity"] > 0}
    edges = []
    for kind, a, b, w in zip(s["edge_kind"], s["edge_a"], s["edge_b"], s["edge_w"]):
        kind, a, b = int(kind), int(a), int(b)
        if not on[kind]:
            continue
        ua = a if kind == PL else NP + NL + a
        ub = NP + b if kind <= VL else NP + NL + b
        if kind == PL:
            we = w * c["lw_pointline_association"]
        elif kind == VL:
            we = w * 1e2 * c["lw_vpline_association"]
        else:
            we = 1e2 * (c["lw_vp_orthogonality"] if kind == ORTH else c["lw_vp_collinearity"])
        edges.append((kind, ua, ub, float(we)))
    touched = set(b["s"] for b in blks) | set(e[1] for e in edges) | set(e[2] for e in edges)
    nd = []
    for u in range(NP + NL + NV):
        if u < NP:
            nd.append(3 if (not cpt and u in touched) else 0)
        elif u < NP + NL:
            nd.append(4 if (not cln and not few[u - NP] and u in touched) else 0)
        else:
            nd.append(2 if (not cvp and u in touched) else 0)
    return blks, edges, nd


def start_params(s, nd):
    """6 per unknown: the points, the lines' minimal parameters, the VPs (a free one normalised)"""
    NP, NL = len(s["poff"]) - 1, len(s["loff"]) - 1
    sp = np.zeros((len(nd), 6))
    for n in range(NP):
        sp[n, :3] = s["p3"][n]
    for n in range(NL):
        sp[NP + n] = ro.minimal(s["line6"][n])
    for n, v in enumerate(s["vp3"]):
        u = NP + NL + n
        v = np.asarray(v, float)
        sp[u, :3] = v / np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) if nd[u] else v
    return sp


def kinds_of(s):
    NP, NL, NV = len(s["poff"]) - 1, len(s["loff"]) - 1, len(s["vp3"])
    return [0] * NP + [1] * NL + [2] * NV


def evaluate(s, sp=None, dtype=np.float64, **kw):
    """at the point sp (start_params where None): dict of res_blk (NB, 2), res_edge (NE, 3), cost, g4 (NU, 4),
    diag (NU, 4, 4), off (NE, 4, 4), and the dense H, g over the unknowns' 4 slots (4 NU)"""
    c = dict(DEFAULTS, **kw)
    blks, edges, nd = setup(s, **kw)
    kinds = kinds_of(s)
    sp = start_params(s, nd) if sp is None else np.asarray(sp, float)
    NU = len(nd)
    poses = [np.concatenate([ro.normalise_q(s["q"][n], np.float64), s["t"][n]]) for n in range(len(s["img_ids"]))]
    g4, diag = np.zeros((NU, 4), dtype), np.zeros((NU, 4, 4), dtype)
    off = np.zeros((len(edges), 4, 4), dtype)
    res_blk, res_edge = np.zeros((len(blks), 2), dtype), np.zeros((len(edges), 3), dtype)
    cost = dtype(0)
    bb = dtype(CAUCHY_B)
    H = np.zeros((4 * NU, 4 * NU), dtype)
    for i, b in enumerate(blks):
        u = b["s"]
        r, _, Js = bo.block_jets(b, s["k"][b["row"]], poses[b["row"]], sp[u][:6 if b["kind"] else 3], c["geometric_alpha"], dtype)
        sq = r[0] * r[0] + r[1] * r[1]
        w = dtype(b["w"])
        if b["kind"]:
            cost = cost + w * bb * np.log(dtype(1) + sq / bb)
            rho1 = w / (dtype(1) + sq / bb)
        else:
            cost = cost + w * sq
            rho1 = w
        res_blk[i] = r
        if nd[u]:
            J = np.zeros((2, 4), dtype)
            J[:, :Js.shape[1]] = Js
            diag[u] += rho1 * (J.T @ J)
            g4[u] += rho1 * (J.T @ r)
    for i, (kind, a, b, w) in enumerate(edges):
        pa = [dtype(x) for x in sp[a]]
        pb = [dtype(x) for x in sp[b]]
        ca, cb = consts(pa, dtype), consts(pb, dtype)
        rv = edge_residual(kind, ca, cb, dtype)
        r = np.zeros(3, dtype)
        r[:len(rv)] = [x.v for x in rv]
        Ja, Jb = np.zeros((3, 4), dtype), np.zeros((3, 4), dtype)
        if nd[a]:
            for m, x in enumerate(edge_residual(kind, seeds(kinds[a], pa, dtype), cb, dtype)):
                Ja[m] = x.d
        if nd[b]:
            for m, x in enumerate(edge_residual(kind, ca, seeds(kinds[b], pb, dtype), dtype)):
                Jb[m] = x.d
        sq = r[0] * r[0] + r[1] * r[1] + r[2] * r[2]
        rho, rho1 = edge_rho(kind, w, sq, dtype)
        cost = cost + rho
        res_edge[i] = r
        diag[a] += rho1 * (Ja.T @ Ja)
        g4[a] += rho1 * (Ja.T @ r)
        diag[b] += rho1 * (Jb.T @ Jb)
        g4[b] += rho1 * (Jb.T @ r)
        off[i] = rho1 * (Ja.T @ Jb)
        H[4 * a:4 * a + 4, 4 * b:4 * b + 4] += off[i]
        H[4 * b:4 * b + 4, 4 * a:4 * a + 4] += off[i].T
    for u in range(NU):
        H[4 * u:4 * u + 4, 4 * u:4 * u + 4] += diag[u]
    return dict(res_blk=res_blk, res_edge=res_edge, cost=cost / dtype(2), g4=g4, diag=diag, off=off, H=H, g=g4.reshape(-1),
                nd=nd, edges=edges, sp=sp)


def free_slots(nd):
    return np.array([4 * u + i for u, n in enumerate(nd) for i in range(n)], int)


def damp(h, mu):
    """lm_damp: h + clamp(sqrt h, 1e-6, 1e32)^2 / mu"""
    d = np.clip(np.sqrt(h), 1e-6, 1e32)
    return h + d * d / mu


# ---- the cost on a packed point, for scipy ----
class Packed:
    """x = the free unknowns' local steps from the point sp0, through the project's charts"""

    def __init__(self, s, **kw):
        self.s, self.kw = s, kw
        self.c = dict(DEFAULTS, **kw)
        self.blks, self.edges, self.nd = setup(s, **kw)
        self.kinds = kinds_of(s)
        self.poses = [np.concatenate([ro.normalise_q(s["q"][n], np.float64), s["t"][n]]) for n in range(len(s["img_ids"]))]
        self.off = np.concatenate([[0], np.cumsum(self.nd)])

    def point(self, sp0, x):
        sp = np.array(sp0, float)
        for u, n in enumerate(self.nd):
            if n:
                dl = np.zeros(4)
                dl[:n] = x[self.off[u]:self.off[u + 1]]
                r = retract(self.kinds[u], sp0[u], dl)
                sp[u, :len(r)] = r
        return sp

    def residuals(self, sp):
        """the blocks' residuals scaled by sqrt(rho(s) / s): half their squared norm is the cost"""
        f64 = np.float64
        out = []
        for b in self.blks:
            k, pose, x = [f64(v) for v in self.s["k"][b["row"]]], self.poses[b["row"]], sp[b["s"]]
            obs = [f64(v) for v in b["obs"]]
            if b["kind"]:
                r = bo.line_residual(k, list(pose[:4]), list(pose[4:]), list(x[:4]), list(x[4:6]), obs, self.c["geometric_alpha"], f64)
                sq = r[0] * r[0] + r[1] * r[1]
                rho = b["w"] * CAUCHY_B * np.log1p(sq / CAUCHY_B)
            else:
                r = bo.point_residual(k, list(pose[:4]), list(pose[4:]), list(x[:3]), obs)
                sq = r[0] * r[0] + r[1] * r[1]
                rho = b["w"] * sq
            sc = np.sqrt(rho / sq) if sq > 0 else 0.0
            out += [r[0] * sc, r[1] * sc]
        for kind, a, b, w in self.edges:
            r = edge_residual(kind, [f64(v) for v in sp[a]], [f64(v) for v in sp[b]], f64)
            sq = sum(v * v for v in r)
            rho, _ = edge_rho(kind, w, sq)
            sc = np.sqrt(rho / sq) if sq > 0 else 0.0
            out += [v * sc for v in r]
        return np.array(out, float)

    def cost(self, sp):
        f = self.residuals(sp)
        return 0.5 * float(f @ f)


# ---- the linear solve as a straight loop in the defined orders ----
def _tree_sum(v):
    """per chunk of 256 items: lane stride (l, l + 64, ...) in ascending order, then the xor tree over the 64 lanes"""
    n = len(v)
    nch = max(1, (n + 255) // 256)
    pad = np.zeros(nch * 256)
    pad[:n] = v
    lanes = pad.reshape(nch, 4, 64)
    acc = np.zeros((nch, 64))
    for k in range(4):
        acc = acc + lanes[:, k, :]
    idx = np.arange(64)
    m = 32
    while m >= 1:
        acc = acc + acc[:, idx ^ m]
        m //= 2
    return acc[:, 0]


def _totals(chunks):
    """one wave over the chunk results: lane stride, then the xor tree"""
    n = len(chunks)
    rows = (n + 63) // 64
    pad = np.zeros(rows * 64)
    pad[:n] = chunks
    acc = np.zeros(64)
    for k in range(rows):
        acc = acc + pad[64 * k:64 * k + 64]
    idx = np.arange(64)
    m = 32
    while m >= 1:
        acc = acc + acc[idx ^ m]
        m //= 2
    return acc[0]


def reduce_dot(per_unknown):
    return _totals(_tree_sum(per_unknown))


def _mul4(M, v):
    """(n, 4, 4) x (n, 4): every row from 0.0 in ascending column order"""
    out = np.zeros_like(v)
    for j in range(4):
        out = out + M[:, :, j] * v[:, j:j + 1]
    return out


def _dot4(a, b):
    s = np.zeros(len(a))
    for j in range(4):
        s = s + a[:, j] * b[:, j]
    return s


def block_inverse(A, nd):
    """the inverse of the leading nd x nd block by the recurrence of lm_step, column by column; None: a bad pivot"""
    L = np.zeros((4, 4))
    for i in range(nd):
        for j in range(i + 1):
            sm = A[i, j]
            for k in range(j):
                sm = sm - L[i, k] * L[j, k]
            if i == j:
                if not (sm > 0 and sm < 1.7976931348623157e308):
                    return None
                L[i, i] = np.sqrt(sm)
            else:
                L[i, j] = sm / L[j, j]
    M = np.zeros((4, 4))
    for c in range(nd):
        y, x = np.zeros(4), np.zeros(4)
        for i in range(nd):
            sm = 1.0 if i == c else 0.0
            for k in range(i):
                sm = sm - L[i, k] * y[k]
            y[i] = sm / L[i, i]
        for i in range(nd - 1, -1, -1):
            sm = y[i]
            for k in range(i + 1, nd):
                sm = sm - L[k, i] * x[k]
            x[i] = sm / L[i, i]
        M[:nd, c] = x[:nd]
    return M


# error-free transformations (Knuth's TwoSum, Dekker's TwoProduct by Veltkamp's split): the same IEEE operations as
# lt_assoc.h's as_two_sum / as_two_prod, on arrays
def two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = 134217729.0 * a
    hi = c - (c - a)
    return hi, a - hi


def two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, (((ah * bh - p) + ah * bl) + al * bh) + al * bl


def dd_acc(h, l, a, b):
    """(h, l) += a b: the product and the sum exact, their errors collected in l"""
    p, e = two_prod(a, b)
    s, t = two_sum(h, p)
    return s, l + (t + e)


def dd_norm(h, l):
    s = h + l
    return s, l - (s - h)


def pcg_loop(nd, diag, edge_a, edge_b, off, rhs, eta, cap):
    """preconditioned CG from x = 0 -> (x (n, 4), iterations, end: 0 converged, 1 cap, 2 breakdown, 3 pivot).  x, r and
    A p are carried as double-double pairs (section 29); p, z and the scalars are plain doubles"""
    n = len(nd)
    A, E, b = np.zeros((n, 4, 4)), np.zeros((len(edge_a), 4, 4)), np.zeros((n, 4))
    for u in range(n):
        A[u, :nd[u], :nd[u]] = diag[u][:nd[u], :nd[u]]
        b[u, :nd[u]] = rhs[u][:nd[u]]
    for e in range(len(edge_a)):
        E[e, :nd[edge_a[e]], :nd[edge_b[e]]] = off[e][:nd[edge_a[e]], :nd[edge_b[e]]]
    Minv = np.zeros((n, 4, 4))
    bad = False
    for u in range(n):
        M = block_inverse(A[u], nd[u])
        bad = bad or M is None
        if M is not None:
            Minv[u] = M
    xh, xl = np.zeros((n, 4)), np.zeros((n, 4))
    if bad:
        return xh, 0, 3
    rh, rl = b.copy(), np.zeros((n, 4))
    z = _mul4(Minv, rh)
    p = z.copy()
    rz0 = rz = reduce_dot(_dot4(rh, z))
    if not (rz0 > 0 and rz0 < 1.7976931348623157e308):
        return xh, 0, 2
    free = np.array(nd) > 0
    it = 0
    while True:
        ah, al = np.zeros((n, 4)), np.zeros((n, 4))
        for j in range(4):
            ah, al = dd_acc(ah, al, A[:, :, j], p[:, j:j + 1])
        for e in range(len(edge_a)):
            ua, ub = edge_a[e], edge_b[e]
            if free[ua]:
                for c in range(4):
                    ah[ua], al[ua] = dd_acc(ah[ua], al[ua], E[e][:, c], p[ub, c])
            if free[ub]:
                for c in range(4):
                    ah[ub], al[ub] = dd_acc(ah[ub], al[ub], E[e][c, :], p[ua, c])
        ah, al = dd_norm(ah, al)
        pap = reduce_dot(_dot4(p, ah))
        if not (pap > 0 and pap < 1.7976931348623157e308):
            return xh, it, 2
        alpha = rz / pap
        xh, xl = dd_norm(*dd_acc(xh, xl, alpha, p))
        rh, rl = dd_acc(rh, rl, -alpha, ah)
        s, t = two_sum(rh, (-alpha) * al)
        rh, rl = dd_norm(s, rl + t)
        z = _mul4(Minv, rh)
        rzn = reduce_dot(_dot4(rh, z))
        it += 1
        if np.sqrt(rzn) <= eta * np.sqrt(rz0):
            return xh, it, 0
        if it >= cap:
            return xh, it, 1
        beta = rzn / rz
        rz = rzn
        p = z + beta * p
