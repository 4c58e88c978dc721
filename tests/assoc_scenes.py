"""Scenes for the tests of the global point-line association: ba_scenes' cameras (held at the
ground truth: they are constants here), point and line tracks, plus vanishing points and association edges, as the arrays
lt_assoc_arrays takes.  Edges: kind 0 point-line, 1 VP-line, 2 VP-VP orthogonality, 3 VP-VP collinearity; a, b index the
tracks and VPs; w the count upstream's construct_weights_* would hand over."""
import ctypes as C

import numpy as np

import ba_scenes as bs

PL, VL, ORTH, COLL = 0, 1, 2, 3


def _with_edges(s, vps, edges):
    s = dict(s)
    e = np.array(edges, float).reshape(-1, 4)
    s.update(vp3=np.ascontiguousarray(np.array(vps, float).reshape(-1, 3)),
             edge_kind=np.ascontiguousarray(e[:, 0], np.int32), edge_a=np.ascontiguousarray(e[:, 1], np.int32),
             edge_b=np.ascontiguousarray(e[:, 2], np.int32), edge_w=np.ascontiguousarray(e[:, 3], np.float64))
    return s


def structured_scene(n_cams=4, lines_per_dir=2, points_per_line=2, n_free_points=2, seed=0, noise_px=0.5,
                     struct_sigma=0.02, vp_sigma=0.03, junction=True, count=4):
    """lines along three orthogonal directions, points generated on them, one VP per direction: the generated incidences
    are the point-line edges, the direction classes the VP-line edges, and the three VP pairs are orthogonality edges"""
    rng = np.random.default_rng(seed)
    base = bs.make_scene(n_cams=n_cams, n_points=0, n_lines=0, seed=seed, pose_sigma=0.0)
    k, q, t, ids = base["k"], base["q_gt"], base["t_gt"], base["img_ids"]
    # a rotated orthogonal frame
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    dirs = Q.T
    gt6, cls = [], []
    for c in range(3):
        for _ in range(lines_per_dir):
            a = rng.uniform(-1.0, 1.0, 3)
            gt6.append(np.concatenate([a, a + dirs[c] * rng.uniform(0.9, 1.6)]))
            cls.append(c)
    gt6 = np.array(gt6)
    NL = len(gt6)
    p_gt, inc = [], []
    for n in range(NL):
        for _ in range(points_per_line):
            u = rng.uniform(0.1, 0.9)
            inc.append((len(p_gt), n))
            p_gt.append(gt6[n, :3] + u * (gt6[n, 3:] - gt6[n, :3]))
    if junction and NL >= 2:  # line 1 moved to pass through the first point of line 0: a point tied to two lines
        d1 = gt6[1, 3:] - gt6[1, :3]
        gt6[1, :3] = p_gt[0] - 0.4 * d1
        gt6[1, 3:] = p_gt[0] + 0.6 * d1
        for i, (p, n) in enumerate(inc):
            if n == 1:
                p_gt[p] = gt6[1, :3] + rng.uniform(0.1, 0.9) * d1
        inc.append((0, 1))
    for _ in range(n_free_points):
        p_gt.append(rng.uniform(-1.0, 1.0, 3))
    p_gt = np.array(p_gt).reshape(-1, 3)
    poff, pimg, pxy = [0], [], []
    for X in p_gt:
        for c in range(n_cams):
            pimg.append(int(ids[c]))
            pxy.append(bs.project(k[c], q[c], t[c], X) + rng.normal(0, noise_px, 2))
        poff.append(len(pimg))
    loff, limg, l2d, l3d = [0], [], [], []
    for n in range(NL):
        a, b = gt6[n, :3], gt6[n, 3:]
        for j in range(n_cams):
            c = (2 * n + 3 * j) % n_cams if n_cams % 3 else (n + j) % n_cams
            pa, pb = a + (b - a) * 0.05, a + (b - a) * 0.95
            limg.append(int(ids[c]))
            l2d.append(np.concatenate([bs.project(k[c], q[c], t[c], pa), bs.project(k[c], q[c], t[c], pb)]) + rng.normal(0, noise_px, 4))
            l3d.append(np.concatenate([pa, pb]) + rng.normal(0, 0.01, 6))
        loff.append(len(limg))
    cc = np.ascontiguousarray
    s = dict(img_ids=cc(ids, np.int32), k=cc(k), q=cc(q), t=cc(t), p3=cc(p_gt + rng.normal(0, struct_sigma, p_gt.shape)),
             p_gt=cc(p_gt), poff=np.array(poff, np.int64), pimg=np.array(pimg, np.int32), pxy=cc(np.array(pxy, float).reshape(-1, 2)),
             line6=cc(gt6 + rng.normal(0, struct_sigma, gt6.shape)), gt6=cc(gt6), loff=np.array(loff, np.int64),
             limg=np.array(limg, np.int32), l2d=cc(np.array(l2d, float).reshape(-1, 4)), l3d=cc(np.array(l3d, float).reshape(-1, 6)),
             dirs_gt=dirs, line_class=np.array(cls), incidences=sorted(inc))
    vps = dirs + rng.normal(0, vp_sigma, dirs.shape)
    vps /= np.linalg.norm(vps, axis=1, keepdims=True)
    edges = [(PL, p, n, count) for p, n in sorted(inc)]
    edges += [(VL, cls[n], n, count) for n in sorted(range(NL), key=lambda n: (cls[n], n))]
    edges += [(ORTH, 0, 1, 1), (ORTH, 0, 2, 1), (ORTH, 1, 2, 1)]
    return _with_edges(s, vps, edges)


def small_scene(seed=0, n_cams=4, parallel=False, orth_exact=False, identical=False):
    """8 points, 4 lines, 3 VPs (two more per clamp case): point 0 tied to lines 0 and 1 (a junction), line 1 tied to points
    0, 1 and VP 0, the last points without an edge, VP 1 tied to VP 0 only, VP 2 without any edge.  parallel: VP 0 exactly along line 0 (the
    sine's EPS term).  orth_exact: VPs 2, 3 exactly orthogonal under an orthogonality edge; identical: VPs 2, 3 identical
    under a collinearity edge (enable with lw_vp_collinearity > 0)"""
    s = structured_scene(n_cams=n_cams, lines_per_dir=2, points_per_line=1, n_free_points=2, seed=seed)
    # keep lines 0..3 (directions 0, 0, 1, 1) and their tracks' supports
    s = dict(s, **{k: v for k, v in bs.without_lines(s, keep=[0, 1, 2, 3]).items()})
    NP = len(s["poff"]) - 1
    assert NP == 8
    vps = [s["vp3"][0].copy(), s["vp3"][2].copy(), s["vp3"][1].copy()]  # VP 2 keeps no edge at all
    edges = [(PL, 0, 0, 4), (PL, 0, 1, 4), (PL, 1, 1, 3), (PL, 2, 2, 5), (PL, 3, 3, 4), (VL, 0, 0, 4), (VL, 0, 1, 3)]
    if parallel:
        d = s["line6"][0, 3:] - s["line6"][0, :3]
        vps[0] = d / np.linalg.norm(d)
    if orth_exact:
        vps += [np.array([1.0, 0.0, 0.0]), np.array([0.0, 0.6, 0.8])]
        edges.append((ORTH, len(vps) - 2, len(vps) - 1, 1))
    if identical:
        v = np.array([0.36, 0.48, 0.8])
        vps += [v, v.copy()]
        edges.append((COLL, len(vps) - 2, len(vps) - 1, 1))
    edges.append((ORTH, 0, 1, 1))
    return _with_edges(s, vps, edges)


def stationary_vp_scene(seed=5):
    """only orthogonality edges between the three coordinate axes, everything else constant or off (use cfg STATIONARY):
    every residual and with it the gradient is exactly zero -- the zero-gradient end"""
    s = structured_scene(n_cams=4, seed=seed)
    return dict(s, vp3=np.eye(3))


STATIONARY = dict(constant_point=1, constant_line=1, enable_pointline=0, lw_vpline_association=0.0)


# a linear solve that fails inside the loop, with finite input (use with the configurations below)
BREAKDOWN = dict(lw_vp_orthogonality=1e300)  # on structured_scene: r0.z0 is finite, the products of A p are not: k_as_alpha
PIVOT = dict(STATIONARY, lw_vp_orthogonality=1e306)


def pivot_scene(seed=5):
    """stationary_vp_scene with a fourth VP equal to the second and an orthogonality edge to the first: with PIVOT the two
    edges' sums of the first VP's block overflow (the cost and the gradient stay exactly zero): a bad pivot"""
    s = stationary_vp_scene(seed)
    return dict(s, vp3=np.ascontiguousarray(np.vstack([s["vp3"], s["vp3"][1:2]])),
                edge_kind=np.append(s["edge_kind"], np.int32(ORTH)), edge_a=np.append(s["edge_a"], np.int32(0)),
                edge_b=np.append(s["edge_b"], np.int32(3)), edge_w=np.append(s["edge_w"], 1.0))


def depth_zero_scene(seed=5):
    """a point of depth exactly 0 in the first camera: the cost at the start is not finite"""
    s = structured_scene(n_cams=4, seed=seed)
    s = dict(s, q=s["q"].copy(), t=s["t"].copy(), p3=s["p3"].copy())
    s["q"][0] = [1.0, 0.0, 0.0, 0.0]
    s["t"][0] = [0.0, 0.0, 5.0]
    s["p3"][0] = [0.3, 0.2, -5.0]
    return s


def graph_scene(n_points, n_lines, n_vps, pl, vl, seed=0, n_cams=3, orth=()):
    """ba_scenes' unstructured points and lines with a given graph: pl = [(point, line)], vl = [(vp, line)]; the geometry
    does not agree with the edges (the robust losses bound them): for the bit-identity tests of the orders"""
    rng = np.random.default_rng(seed + 77)
    s = bs.make_scene(n_cams=n_cams, n_points=n_points, n_lines=n_lines, seed=seed, pose_sigma=0.0)
    vps = rng.normal(size=(n_vps, 3))
    vps /= np.linalg.norm(vps, axis=1, keepdims=True)
    edges = [(PL, p, n, 3 + (p + n) % 3) for p, n in sorted(pl)] + [(VL, v, n, 3 + n % 4) for v, n in sorted(vl)]
    edges += [(ORTH, a, b, 1) for a, b in orth]
    return _with_edges(s, vps, edges)


# ---- the native calls on a scene ----
def cfg_of(**kw):
    from limap_amd import _capi
    c = _capi.LtAssocConfig()
    _capi.load_library().lt_assoc_config_default(C.byref(c))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def input_of(s):
    """lt_assoc_input over the scene's arrays (which the returned structure keeps alive)"""
    from limap_amd import _capi
    p = _capi.ptr
    a = _capi.LtAssocInput()
    a.n_img = len(s["img_ids"])
    a.img_ids, a.kvec4, a.qvec4, a.tvec3 = p(s["img_ids"], C.c_int32), p(s["k"]), p(s["q"]), p(s["t"])
    a.n_pt = len(s["poff"]) - 1
    a.pt3, a.pt_off, a.pt_img, a.pt_xy2 = p(s["p3"]), p(s["poff"], C.c_int64), p(s["pimg"], C.c_int32), p(s["pxy"])
    a.n_ln = len(s["loff"]) - 1
    a.line6, a.ln_off, a.ln_img, a.l2d4 = p(s["line6"]), p(s["loff"], C.c_int64), p(s["limg"], C.c_int32), p(s["l2d"])
    a.n_vp = len(s["vp3"])
    a.vp3 = p(s["vp3"])
    a.n_edge = len(s["edge_kind"])
    a.edge_kind, a.edge_a, a.edge_b = p(s["edge_kind"], C.c_int32), p(s["edge_a"], C.c_int32), p(s["edge_b"], C.c_int32)
    a.edge_w = p(s["edge_w"])
    a._keep = s
    return a


def _outs(s):
    NP, NL, NV = len(s["poff"]) - 1, len(s["loff"]) - 1, len(s["vp3"])
    return dict(points=np.zeros((NP, 3)), params=np.zeros((NL, 6)), vps=np.zeros((NV, 3)), cost=np.zeros(2),
                iterations=np.zeros(1, np.int32), cg_iterations=np.zeros(1, np.int64), code=np.zeros(1, np.int32))


def _out_ptrs(o):
    from limap_amd import _capi
    p = _capi.ptr
    return (p(o["points"]), p(o["params"]), p(o["vps"]), p(o["cost"]), p(o["iterations"], C.c_int32),
            p(o["cg_iterations"], C.c_int64), p(o["code"], C.c_int32))


def run_host(s, cfg, threads=4, trace=0):
    """lt_fn_assoc_host -> (return code, outputs[, trace dict])"""
    from limap_amd import _capi
    o = _outs(s)
    n, total0, rec = np.zeros(1, np.int64), np.zeros(1), np.zeros((max(trace, 1), 6))
    p = _capi.ptr
    rc = _capi.load_library().lt_fn_assoc_host(C.byref(input_of(s)), C.byref(cfg), int(threads), *_out_ptrs(o), int(trace),
                                               p(n, C.c_int64), p(total0), p(rec))
    if trace:
        return rc, o, dict(n=int(n[0]), total0=float(total0[0]), rec=rec[:min(int(n[0]), trace)])
    return rc, o


def run_device(ctx, s, cfg):
    """lt_assoc_arrays + lt_assoc_get -> (return code, outputs)"""
    o = _outs(s)
    rc = ctx.L.lt_assoc_arrays(ctx.h, C.byref(input_of(s)), C.byref(cfg))
    if rc == 0:
        ctx.chk(ctx.L.lt_assoc_get(ctx.h, *_out_ptrs(o)))
    return rc, o


def host_error():
    from limap_amd import _capi
    return _capi.load_library().lt_fn_assoc_host_error().decode(errors="replace")


def evaluate(s, cfg, sp=None):
    """lt_fn_assoc_eval -> dict (the arrays of the header's comment)"""
    from limap_amd import _capi
    L, p = _capi.load_library(), _capi.ptr
    inp = input_of(s)
    dims = np.zeros(8, np.int64)
    none = [None] * 11
    rc = L.lt_fn_assoc_eval(C.byref(inp), C.byref(cfg), None, p(dims, C.c_int64), *none)
    if rc:
        raise ValueError(host_error())
    NU, NB, NE = int(dims[0]), int(dims[4]), int(dims[5])
    o = dict(nd=np.zeros(max(NU, 1), np.int32), blk_unk=np.zeros(max(NB, 1), np.int32), edge_info=np.zeros((max(NE, 1), 3), np.int32),
             edge_w=np.zeros(max(NE, 1)), sp=np.zeros((max(NU, 1), 6)), res_blk=np.zeros((max(NB, 1), 2)),
             res_edge=np.zeros((max(NE, 1), 3)), cost=np.zeros(1), g4=np.zeros((max(NU, 1), 4)), diag=np.zeros((max(NU, 1), 4, 4)),
             off=np.zeros((max(NE, 1), 4, 4)))
    spp = None if sp is None else p(np.ascontiguousarray(sp, np.float64))
    rc = L.lt_fn_assoc_eval(C.byref(inp), C.byref(cfg), spp, p(dims, C.c_int64), p(o["nd"], C.c_int32), p(o["blk_unk"], C.c_int32),
                            p(o["edge_info"], C.c_int32), p(o["edge_w"]), p(o["sp"]), p(o["res_blk"]), p(o["res_edge"]),
                            p(o["cost"]), p(o["g4"]), p(o["diag"]), p(o["off"]))
    if rc:
        raise ValueError(host_error())
    cut = dict(nd=NU, sp=NU, g4=NU, diag=NU, blk_unk=NB, res_blk=NB, edge_info=NE, edge_w=NE, res_edge=NE, off=NE)
    o = {k: (v[:cut[k]] if k in cut else v) for k, v in o.items()}
    o["dims"] = dims
    o["cost"] = float(o["cost"][0])
    return o


def pcg(nd, diag, edge_a, edge_b, off, rhs, eta, cap):
    """lt_fn_assoc_pcg -> (return code, x (n, 4), iterations, end, (r0.z0, last r.z))"""
    from limap_amd import _capi
    L, p = _capi.load_library(), _capi.ptr
    n, ne = len(nd), len(edge_a)
    nd = np.ascontiguousarray(nd, np.int32)
    diag = np.ascontiguousarray(diag, np.float64).reshape(n, 16)
    ea, eb = np.ascontiguousarray(edge_a, np.int32), np.ascontiguousarray(edge_b, np.int32)
    off = np.ascontiguousarray(off, np.float64).reshape(max(ne, 0), 16) if ne else np.zeros((1, 16))
    if not ne:
        ea, eb = np.zeros(1, np.int32), np.zeros(1, np.int32)
    rhs = np.ascontiguousarray(rhs, np.float64).reshape(n, 4)
    x, it, end, rz = np.zeros((n, 4)), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(2)
    rc = L.lt_fn_assoc_pcg(n, p(nd, C.c_int32), p(diag), ne, p(ea, C.c_int32), p(eb, C.c_int32), p(off), p(rhs), float(eta),
                           int(cap), p(x), p(it, C.c_int32), p(end, C.c_int32), p(rz))
    return rc, x, int(it[0]), int(end[0]), rz


def same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)
