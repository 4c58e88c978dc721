"""NumPy restatement of the feature-consistency term of limap.optimize.line_refinement, written
from upstream's files in their operation order and parameterised on the dtype (float64, longdouble); the dual numbers,
the parameterisation, the projection and the geometric term come from refine_oracle, the intersection and the bilinear
rule from refine_terms_oracle, the camera projection of a point from patch_oracle.  Paths relative to src/limap:

    base/linetrack.cc:353-454                                   samples(): ComputeFConsistencySamples (float64: the
                                                                samples are data of the problem, taken once)
    base/line_dists.h:98-119, base/infinite_line.cc:9-16        perp_oneway(), infinite_line()
    ceresbase/line_projection.h:136-200                         fundamental(), epiline(): GetEpipolarLineCoordinate
    ceresbase/line_projection.h:202-213                         ro.plucker, ro.world_to_pixel, to.intersect
    features/featurepatch.h:53-123, features/featuremap.h:77-85 to_local(), bilinear128()
    optimize/line_refinement/pixel_cost_functions.h:342-385     block(): FeatureConsisTgtFunctor
    optimize/line_refinement/refine.cc:363-543                  evaluate(): the blocks, their order and weight

The multiplication order of the fundamental matrix: relR = R_tgt R_ref^T, relT = t_tgt - relR t_ref, E = [relT]x relR,
F = (Kinv_tgt^T E) Kinv_ref, every 3x3 product summing its three terms left to right with the zero entries in place; R is
Ceres' QuaternionToRotation of the view's quaternion, normalised once by CameraPose.  The epipolar line is
(F (x, y, 1)).normalized().  A block with |p_homo[2]| < EPS at either intersection fails; an evaluation with a failed
block has cost +inf (this project's rule).
"""
import numpy as np

import patch_oracle as po
import refine_oracle as ro
import refine_terms_oracle as to
from refine_oracle import Dual, _sqrt, val

TH_PERP = 0.3
CHANNELS = 128


def unit2(v):
    z = v[0] * v[0] + v[1] * v[1]
    return v / np.sqrt(z) if z > 0 else v


def unit3(v):
    z = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
    return v / np.sqrt(z) if z > 0 else v


def length2(s, e):
    d = s - e
    return np.sqrt(d[0] * d[0] + d[1] * d[1])


def dot2(a, b):
    return a[0] * b[0] + a[1] * b[1]


def perp_oneway(s1, e1, s2, e2):
    """dist_endpoints_perpendicular_oneway(l1, l2): the ends of l1 against the line of l2"""
    v2 = unit2(e2 - s2)
    out = []
    for p in (s1, e1):
        d = p - s2
        out.append(np.sqrt(max(dot2(d, d) - dot2(d, v2) * dot2(d, v2), 0.0)))
    return max(out)


def infinite_line(p, direc):
    """InfiniteLine2d(p, direc).coords"""
    return unit3(np.array([direc[1], (-1.0) * direc[0], ((-1.0) * direc[1]) * p[0] + direc[0] * p[1]]))


def samples(line6, img_ids, segs4, cams, rmin, rmax, n):
    """ComputeFConsistencySamples: supports in the track's list order, cams {img_id: cam11}
    -> [(ref_img_id, coords (3), [target img ids])], the kept samples in order"""
    line6, segs4 = np.asarray(line6, np.float64), np.asarray(segs4, np.float64)
    ids = sorted(set(int(i) for i in img_ids))
    start, end = line6[:3], line6[3:]
    interval = (end - start) / np.float64(n - 1)
    proj_line = {i: (po.project(cams[i], start)[0], po.project(cams[i], end)[0]) for i in ids}
    out = []
    for pi in range(n):
        point = start + np.float64(pi) * interval
        proj = {i: po.project(cams[i], point)[0] for i in ids}
        supports = []
        for k, (i, sg) in enumerate(zip(img_ids, segs4)):
            s, e = sg[:2], sg[2:]
            pr = dot2(proj[int(i)] - s, unit2(e - s)) / length2(s, e)
            if pr >= rmin and pr <= rmax:
                supports.append(k)
        if len(supports) < 2:
            continue
        good = [k for k in supports
                if perp_oneway(segs4[k][:2], segs4[k][2:], *proj_line[int(img_ids[k])]) < TH_PERP]
        if not good:
            continue
        max_length, max_id = -1.0, -1
        for k in good:
            ln = length2(segs4[k][:2], segs4[k][2:])
            if ln > max_length:
                max_length, max_id = ln, k
        ref = int(img_ids[max_id])
        d = unit2(segs4[max_id][2:] - segs4[max_id][:2])
        coor = infinite_line(proj[ref], np.array([d[1], -d[0]]))
        tgts = [i for i in sorted(set(int(img_ids[k]) for k in supports)) if i != ref]
        out.append((ref, coor, tgts))
    return out


def view(cam11, dtype):
    """-> kvec, Ceres' rotation (3x3 lists) of the once-normalised quaternion, tvec, the normalised quaternion"""
    q = ro.normalise_q(cam11[4:8], dtype)
    return [dtype(x) for x in cam11[:4]], ro._mat3(ro.quat_to_rot_ceres(list(q))), [dtype(x) for x in cam11[8:11]], q


def fundamental(cam_ref, cam_tgt, dtype):
    kr, Rr, tr, _ = view(cam_ref, dtype)
    kt, Rt, tt, _ = view(cam_tgt, dtype)
    zero, one = dtype(0), dtype(1)
    relR = ro._mm(Rt, ro._T(Rr))
    rt = [relR[i][0] * tr[0] + relR[i][1] * tr[1] + relR[i][2] * tr[2] for i in range(3)]
    relT = [tt[i] - rt[i] for i in range(3)]
    E = ro._mm(ro._skew(relT, zero), relR)
    kinv = lambda k: [[one / k[0], zero, -k[2] / k[0]], [zero, one / k[1], -k[3] / k[1]], [zero, zero, one]]  # noqa: E731
    return ro._mm(ro._mm(ro._T(kinv(kt)), E), kinv(kr))


def epiline(F, x, y):
    e = [F[i][0] * x + F[i][1] * y + F[i][2] for i in range(3)]
    z = e[0] * e[0] + e[1] * e[1] + e[2] * e[2]
    if val(z) > 0:
        n = _sqrt(z)
        e = [c / n for c in e]
    return e


def to_local(grid, x, y, dtype):
    """FeaturePatch::GlobalToLocal; grid = (array (h, w, 128), R (2, 2), tvec (2,)); a map: R = I, tvec = 0"""
    _, R, t = grid
    ax, ay = x - dtype(t[0]), y - dtype(t[1])
    return dtype(R[0][0]) * ax + dtype(R[0][1]) * ay, dtype(R[1][0]) * ax + dtype(R[1][1]) * ay


def bilinear128(arr, r, c, dtype):
    """BiLinearInterpolator::Evaluate over the 128 channels at (r, c) -> f, dfdr, dfdc (forward differences)"""
    h, w = arr.shape[:2]
    rv, cv = dtype(val(r)), dtype(val(c))
    row, col = int(np.floor(rv)), int(np.floor(cv))
    dy, dx = rv - dtype(row), cv - dtype(col)
    t = lambda a, b: arr[min(max(row + a, 0), h - 1), min(max(col + b, 0), w - 1)].astype(dtype)  # noqa: E731
    ll, lr, ul, ur = t(0, 0), t(0, 1), t(1, 0), t(1, 1)
    f = to._interp(dx, dy, ll, lr, ul, ur)
    dfdr = to._interp(dx, dy, ul, ur, t(2, 0), t(2, 1)) - f
    dfdc = to._interp(dx, dy, lr, t(0, 2), ur, t(1, 2)) - f
    return f, dfdr, dfdc


def _jet(arr, ly, lx, dtype):
    f, fr, fc = bilinear128(arr, ly, lx, dtype)
    return f, fr[:, None] * ly.d[None, :] + fc[:, None] * lx.d[None, :]


def block(cam_ref, cam_tgt, grid_ref, grid_tgt, coor, u, w, dtype):
    """FeatureConsisTgtFunctor::operator() -> (ok, residuals (128), jacobian (128, 4), xy_ref, xy_tgt values)"""
    cr, ct = ro.cams_normalised([cam_ref, cam_tgt], dtype)
    d, m = ro.plucker(u, w, dtype)
    c_ref = ro.world_to_pixel(cr[:4], cr[4:8], cr[8:11], d, m, dtype)
    ok, xy = to.intersect(c_ref, [dtype(x) for x in coor], dtype)
    if not ok:
        return False, None, None, None, None
    lx, ly = to_local(grid_ref, xy[0], xy[1], dtype)
    f_ref, j_ref = _jet(grid_ref[0], ly, lx, dtype)
    epi = epiline(fundamental(cam_ref, cam_tgt, dtype), xy[0], xy[1])
    c_tgt = ro.world_to_pixel(ct[:4], ct[4:8], ct[8:11], d, m, dtype)
    ok, xt = to.intersect(c_tgt, epi, dtype)
    if not ok:
        return False, None, None, None, None
    lx, ly = to_local(grid_tgt, xt[0], xt[1], dtype)
    f_tgt, j_tgt = _jet(grid_tgt[0], ly, lx, dtype)
    return True, f_tgt - f_ref, j_tgt - j_ref, [float(val(v)) for v in xy], [float(val(v)) for v in xt]


def evaluate(line6, img_ids, segs4, cams, grids, p, n_samples=100, fconsis_multiplier=1.0, rmin=0.05, rmax=0.95,
             use_geometric=True, alpha=10.0, dtype=np.float64, smps=None):
    """One track at the minimal parameters p.  img_ids, segs4: the supports in list order; cams {img_id: cam11};
    grids {img_id: (array, R, tvec)}.  -> dict(samples, r (n_blocks, 128), failed (n_blocks), cost, g, H, weights,
    xy_ref, xy_tgt)"""
    if smps is None:
        smps = samples(line6, img_ids, segs4, cams, rmin, rmax, n_samples)
    u, w = ro.seeds(p, dtype)
    b = dtype(ro.CAUCHY_B)
    cost, g, H = dtype(0), np.zeros(4, dtype), np.zeros((4, 4), dtype)
    if use_geometric:
        order = ro.residual_order(img_ids)
        cam_rows = ro.cams_normalised([cams[int(img_ids[k])] for k in order], dtype)
        for row, k in zip(cam_rows, order):
            s = [dtype(x) for x in segs4[k]]
            rr = ro.residual(row, s, u, w, alpha, dtype)
            wk = np.sqrt((s[0] - s[2]) ** 2 + (s[1] - s[3]) ** 2) / dtype(30)
            sq = rr[0].v * rr[0].v + rr[1].v * rr[1].v
            cost = cost + wk * b * np.log(dtype(1) + sq / b)
            J = np.stack([rr[0].d, rr[1].d])
            rho1 = wk / (dtype(1) + sq / b)
            H += rho1 * (J.T @ J)
            g += rho1 * (J.T @ np.array([rr[0].v, rr[1].v], dtype))
    res, failed, weights, xr, xt = [], [], [], [], []
    for ref, coor, tgts in smps:
        for tg in tgts:
            wgt = dtype(fconsis_multiplier) / ((dtype(len(smps)) / dtype(100)) * (dtype(len(tgts)) / dtype(5)))
            ok, r, J, a, c = block(cams[ref], cams[tg], grids[ref], grids[tg], coor, u, w, dtype)
            failed.append(not ok)
            weights.append(wgt)
            if not ok:
                res.append(np.full(CHANNELS, np.nan, dtype))
                xr.append([np.nan, np.nan]); xt.append([np.nan, np.nan])
                continue
            sq = (r * r).sum()
            cost = cost + wgt * b * np.log(dtype(1) + sq / b)
            rho1 = wgt / (dtype(1) + sq / b)
            H += rho1 * (J.T @ J)
            g += rho1 * (J.T @ r)
            res.append(r); xr.append(a); xt.append(c)
    cost = dtype(np.inf) if any(failed) else cost / dtype(2)
    return dict(samples=smps, r=np.array(res, dtype).reshape(-1, CHANNELS), failed=np.array(failed, bool), cost=cost, g=g,
                H=H, weights=np.array(weights, dtype), xy_ref=np.array(xr).reshape(-1, 2), xy_tgt=np.array(xt).reshape(-1, 2))
