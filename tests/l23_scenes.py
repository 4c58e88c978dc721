"""Small planted scenes for the 2D-3D line matching: a handful of 3D lines, database views with
known poses whose segments are projections of the tracks plus clutter (track -1), queries with a coarse pose a few
degrees and centimetres off.  A scene is the dict tests/l23_oracle.py reads; `limap_amd.localization.scene_arrays(*args(sc))`
takes the same."""
import numpy as np

import est_oracle as eo
import est_scenes as _es

KVEC = np.array([600.0, 590.0, 400.0, 300.0])
DB_LINES = (0, 1, 63, 64, 65, 130)


def rot_y(a):
    return np.array([np.cos(a / 2), 0.0, np.sin(a / 2), 0.0])


def cam11(q, t):
    return np.concatenate([KVEC, np.asarray(q, float), np.asarray(t, float)])


def project(cam, X):
    R = eo.rotation(cam[4:8])
    pc = R @ np.asarray(X, float) + cam[8:11]
    return np.array([KVEC[0] * pc[0] / pc[2] + KVEC[2], KVEC[1] * pc[1] / pc[2] + KVEC[3]])


def seg_of(cam, l6, rng=None, noise=0.0):
    s = np.concatenate([project(cam, l6[:3]), project(cam, l6[3:])])
    return s + (rng.normal(0, noise, 4) if noise else 0.0)


def world_lines(rng, n):
    a = np.column_stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(5, 8, n)])
    b = a + rng.normal(0, 0.6, (n, 3))
    return np.concatenate([a, b], 1)


def clutter(rng, n):
    a = np.column_stack([rng.uniform(50, 750, n), rng.uniform(50, 550, n)])
    return np.concatenate([a, a + rng.normal(0, 60, (n, 2))], 1)


def args(sc):
    """the arguments of limap_amd.localization.scene_arrays"""
    return (sc["db_cams"], sc["db_segs"], sc["db_tracks"], sc["q_cams"], sc["q_segs"], sc["tasks"], sc.get("pairs"), sc["tracks6"])


def db_view(rng, cam, tracks6, n_lines, share=0.6):
    """n_lines segments: projections of randomly chosen tracks, the rest clutter without a track"""
    n_t = min(int(round(share * n_lines)), len(tracks6)) if n_lines > 1 else n_lines
    ids = rng.permutation(len(tracks6))[:n_t]
    segs = [seg_of(cam, tracks6[t], rng, 0.3) for t in ids]
    segs = np.array(segs).reshape(-1, 4)
    segs = np.concatenate([segs, clutter(rng, n_lines - n_t)], 0)
    trk = np.concatenate([ids, -np.ones(n_lines - n_t, int)]).astype(int)
    p = rng.permutation(n_lines)
    return segs[p], trk[p]


def sizes_scene(seed=0):
    """Database images with 0, 1, 63, 64, 65 and 130 lines; queries with 5, 0, 1, 5, 5 lines (one without lines between two
    that have some) and 3, 1, 1, 0, 3 tasks, one image listed twice; a zero-length segment on either side."""
    rng = np.random.default_rng(seed)
    tracks6 = world_lines(rng, 130)
    db_cams = [cam11(rot_y(0.02 * (d - 2)), [0.4 * (d - 2.5), 0.05 * d, 0.1]) for d in range(len(DB_LINES))]
    views = [db_view(rng, db_cams[d], tracks6, n) for d, n in enumerate(DB_LINES)]
    db_segs, db_tracks = [v[0] for v in views], [v[1] for v in views]
    db_segs[5][7, 2:] = db_segs[5][7, :2]  # a database segment of zero length
    q_true = [cam11(rot_y(0.01 * q), [0.1 * q, -0.05, 0.0]) for q in range(5)]
    q_cams = [cam11(rot_y(0.01 * q + 0.03), [0.1 * q + 0.05, -0.02, 0.03]) for q in range(5)]  # some 2 degrees, 5 cm off
    q_lines = (5, 0, 1, 5, 5)
    q_segs = []
    for q, n in enumerate(q_lines):
        ids = rng.permutation(130)[:n]
        q_segs.append(np.array([seg_of(q_true[q], tracks6[t], rng, 0.5) for t in ids]).reshape(-1, 4))
    q_segs[4][2, 2:] = q_segs[4][2, :2]  # a query segment of zero length
    tasks = [[5, 0, 5], [2], [3], [], [1, 2, 4]]
    return dict(db_cams=db_cams, db_segs=db_segs, db_tracks=db_tracks, q_cams=q_cams, q_segs=q_segs, tasks=tasks, tracks6=tracks6)


def with_pairs(sc, seed=1, per_task=40):
    """listed pairs for every task of a scene: random pairs, some twice, in no order"""
    rng = np.random.default_rng(seed)
    pairs = []
    for q, t in enumerate(sc["tasks"]):
        pq = []
        for img in t:
            nq, nd = len(sc["q_segs"][q]), len(sc["db_segs"][img])
            n = per_task if nq and nd else 0
            m = np.column_stack([rng.integers(0, max(nq, 1), n), rng.integers(0, max(nd, 1), n)]).reshape(-1, 2)
            pq.append(np.concatenate([m, m[:3]], 0))
        pairs.append(pq)
    return dict(sc, pairs=pairs)


def order_scene():
    """Query line 0 first survives in the second task, query line 1 in the first: the rows of line 1 come first.  The
    baseline is along x, so epipolar lines are horizontal; the two tracks are vertical and lie in disjoint bands of y."""
    tracks6 = np.array([[0.5, -1.5, 6.0, 0.5, -0.5, 6.0], [-0.5, 0.5, 6.0, -0.5, 1.5, 6.0]])
    ident = [1.0, 0.0, 0.0, 0.0]
    db_cams = [cam11(ident, [0.5, 0.0, 0.0]), cam11(ident, [-0.5, 0.0, 0.0])]
    db_segs = [seg_of(db_cams[0], tracks6[1]).reshape(1, 4), seg_of(db_cams[1], tracks6[0]).reshape(1, 4)]
    q_cam = cam11(ident, [0.0, 0.0, 0.0])
    q_segs = [np.array([seg_of(q_cam, tracks6[0]), seg_of(q_cam, tracks6[1])])]
    return dict(db_cams=db_cams, db_segs=db_segs, db_tracks=[[1], [0]], q_cams=[q_cam], q_segs=q_segs, tasks=[[0, 1]],
                tracks6=tracks6)


def degenerate_scene(seed=3):
    """A query whose coarse pose equals the database pose (F is zero) and a query with a segment through the epipole"""
    rng = np.random.default_rng(seed)
    tracks6 = world_lines(rng, 12)
    db_cam = cam11(rot_y(0.05), [0.3, 0.0, 0.2])
    segs, trk = db_view(rng, db_cam, tracks6, 10)
    q_same = db_cam.copy()
    q_other = cam11(rot_y(0.0), [0.0, 0.0, 0.0])
    centre = -eo.rotation(db_cam[4:8]).T @ db_cam[8:11]  # the database camera's centre, seen from the second query
    e = project(q_other, centre)  # the epipole
    through = np.concatenate([e - [30.0, 10.0], e + [30.0, 10.0]])
    qs = np.array([seg_of(q_other, tracks6[t], rng, 0.5) for t in range(4)] + [through])
    return dict(db_cams=[db_cam], db_segs=[segs], db_tracks=[trk], q_cams=[q_same, q_other], q_segs=[qs[:4], qs], tasks=[[0], [0]],
                tracks6=tracks6)


FILTER_COUNTS = (1, 63, 64, 65, 130)
T_BEHIND, T_TURNED, T_TWIN_LO, T_TWIN_HI = 130, 131, 1, 6


def filter_scene(seed=5):
    """One query, one stand-in database image whose line t belongs to track t, listed pairs.  Tracks 0 .. 129 are the
    five base lines shifted by (t // 5) steps of about half a pixel; query line i is the image of base line i and has
    1, 63, 64, 65, 130 candidates (listed in descending order, some twice).  Track 6 equals track 1 (equal losses: the
    smaller id wins); track 130 lies behind the camera; track 131 is base line 0 turned by 45 degrees about its midpoint
    (its sine is above the threshold under Midpoint).  Query line 5 has only far candidates (dropped under Perpendicular
    and Midpoint); query line 6 is line 0 again with the candidates 131, 130 and 5; query line 7 is line 2 moved by five
    pixels across itself: dropped at dist_thres 2, kept at 10."""
    rng = np.random.default_rng(seed)
    base = world_lines(rng, 6)
    tracks6 = np.zeros((132, 6))
    for t in range(130):
        tracks6[t] = base[t % 5] + 0.004 * (t // 5) * np.array([1.0, 0.0, 0.0, 1.0, 0.0, 0.0])
    tracks6[T_TWIN_HI] = tracks6[T_TWIN_LO]
    tracks6[T_BEHIND] = base[0] * np.array([1, 1, -1, 1, 1, -1.0])
    m, h = 0.5 * (base[0][:3] + base[0][3:]), 0.5 * (base[0][3:] - base[0][:3])
    c, s = np.cos(np.pi / 4), np.sin(np.pi / 4)
    ht = np.array([c * h[0] - s * h[1], s * h[0] + c * h[1], h[2]])
    tracks6[T_TURNED] = np.concatenate([m - ht, m + ht])
    cam = cam11(rot_y(0.01), [0.02, -0.01, 0.0])
    q_segs = np.array([seg_of(cam, base[i], rng, 0.2) for i in range(6)] + [seg_of(cam, base[0], rng, 0.2)])
    q_segs[5] += 300.0  # far from every candidate
    d = q_segs[2, 2:] - q_segs[2, :2]
    nrm = np.array([-d[1], d[0]]) / np.linalg.norm(d)
    q_segs = np.concatenate([q_segs, (q_segs[2] + 5.0 * np.concatenate([nrm, nrm])).reshape(1, 4)], 0)
    m = []
    for i, n in enumerate(FILTER_COUNTS):
        ids = list(range(n - 1, -1, -1))
        m += [(i, t) for t in ids + ids[:2]]
    m += [(5, 0), (5, 1), (5, 2), (6, T_TURNED), (6, T_BEHIND), (6, 5), (7, 12), (7, 2), (7, 7)]
    return dict(db_cams=[cam], db_segs=[np.zeros((132, 4))], db_tracks=[np.arange(132)], q_cams=[cam], q_segs=[q_segs], tasks=[[0]],
                pairs=[[np.array(m)]], tracks6=tracks6)


def loc_scene(seed=0, n_tracks=24, n_db=4, n_query=2, clutter_share=0.25, noise=0.5, n_pts=40, outliers=0.4):
    """The runner's planted scene: every database view sees every track (plus clutter), every query sees every track from
    its true pose (plus clutter) and carries a coarse pose about two degrees and five centimetres off; point
    correspondences as est_scenes.planted_scene draws them.  -> dict with the scene, the name maps and the true poses."""
    rng = np.random.default_rng(seed)
    tracks6 = world_lines(rng, n_tracks)
    db_cams = [cam11(rot_y(0.04 * (d - 1.5)), [0.5 * (d - 1.5), 0.05 * d, 0.1]) for d in range(n_db)]
    n_cl = int(round(clutter_share * n_tracks))
    db_segs, db_tracks = [], []
    for d in range(n_db):
        segs = np.array([seg_of(db_cams[d], l, rng, 0.3) for l in tracks6])
        db_segs.append(np.concatenate([segs, clutter(rng, n_cl)], 0))
        db_tracks.append(np.concatenate([np.arange(n_tracks), -np.ones(n_cl, int)]).astype(int))
    truth, q_cams, q_segs, points = [], [], [], []
    for q in range(n_query):
        qv = eo.normalise_q(np.array([1.0, 0.01 * q, 0.02 * (q + 1), -0.01]))
        t = np.array([0.2 * q - 0.1, 0.05, 0.05 * q])
        true = cam11(qv, t)
        truth.append(true)
        dq = eo.normalise_q(np.array([1.0, 0.012, -0.01, 0.008]))  # about two degrees
        w0, v0, w1, v1 = dq[0], dq[1:], qv[0], qv[1:]
        qc = np.concatenate([[w0 * w1 - v0 @ v1], w0 * v1 + w1 * v0 + np.cross(v0, v1)])
        q_cams.append(cam11(qc, t + np.array([0.03, -0.03, 0.03])))
        segs = np.array([seg_of(true, l, rng, noise) for l in tracks6])
        q_segs.append(np.concatenate([segs, clutter(rng, n_cl)], 0))
        R = eo.rotation(qv)
        n_out = int(round(outliers * n_pts))
        p3, p2 = [], []
        for i in range(n_pts):
            pc = np.array([rng.uniform(-1.2, 1.2), rng.uniform(-0.9, 0.9), 1.0]) * rng.uniform(2, 6)
            p3.append(R.T @ (pc - t))
            wrong = np.array([rng.uniform(0, 800), rng.uniform(0, 600)])
            p2.append(wrong if i < n_out else project(true, p3[-1]) + rng.normal(0, noise, 2))
        points.append(dict(p3ds=np.array(p3), p2ds=np.array(p2)))
    tasks = [[(q + k) % n_db for k in range(3)] for q in range(n_query)]
    return dict(db_cams=db_cams, db_segs=db_segs, db_tracks=db_tracks, q_cams=q_cams, q_segs=q_segs, tasks=tasks, tracks6=tracks6,
                truth=truth, points=points)


FILTER_NAMES = (None, "Perpendicular", "Midpoint", "Midpoint_Perpendicular")


def order_pairs_scene():
    """the order scene in the listed modes: the pair of query line 1 is listed in the first task, that of line 0 in the second"""
    return dict(order_scene(), pairs=[[np.array([[1, 0]]), np.array([[0, 0]])]])


_CASES = []


def cases():
    """Every scene, mode and filter the twin (test_l23_host.py) and the device (test_gpu_l23.py) are compared on: dicts with
    name, scene, mode, filt and kw (thresholds)."""
    if _CASES:
        return _CASES

    def add(name, sc, mode, filt, **kw):
        _CASES.append(dict(name=f"{name}-{mode}-{filt}" + "".join(f"-{k}{v}" for k, v in kw.items()), scene=sc, mode=mode, filt=filt, kw=kw))

    sizes = sizes_scene()
    listed = with_pairs(sizes)
    for filt in FILTER_NAMES:
        add("sizes", sizes, "all_pairs", filt)
        add("sizes", listed, "listed", filt)
        add("sizes", listed, "listed_filtered", filt)
        add("order", order_scene(), "all_pairs", filt)
        add("degenerate", degenerate_scene(), "all_pairs", filt)
        for dist_thres in (2.0, 10.0):
            add("filter", filter_scene(), "listed", filt, dist_thres=dist_thres)
    add("order", order_pairs_scene(), "listed", None)
    add("order", order_pairs_scene(), "listed_filtered", None)
    add("all-fail", sizes, "all_pairs", None, thr=2.0)
    add("all-fail", sizes, "all_pairs", "Perpendicular", thr=2.0)
    add("wide", sizes, "all_pairs", "Midpoint", dist_thres=400.0, sine_thres=2.0, angle_scale=0.5)
    return _CASES


_REFERENCE = {}


def reference(ora, case):
    """the restatement's (q_off, rows, loss) of a case, computed once"""
    import l23_oracle as lo
    if case["name"] not in _REFERENCE:
        _REFERENCE[case["name"]] = lo.match_scene(ora, case["scene"], case["mode"], case["filt"], **case["kw"])
    return _REFERENCE[case["name"]]


def product(loc, case, **how):
    """the same case through limap_amd.localization (`loc`), on the host twin (host=True) or the device"""
    kw = dict(case["kw"])
    if "thr" in kw:
        kw["IoU_threshold"] = kw.pop("thr")
    return loc.match_lines_arrays(loc.scene_arrays(*args(case["scene"])), case["mode"], dist_func=case["filt"], **kw, **how)


def collections(sc):
    """a loc_scene as the runner's arguments: image collections with names, segment dicts, line tracks, retrieval by name, points"""
    from limap_amd import base
    n_db = len(sc["db_cams"])
    db = base.ImageCollection({10 + d: base.CameraView(c[:4], c[4:8], c[8:], image_name=f"db/{d}.png") for d, c in enumerate(sc["db_cams"])})
    qr = base.ImageCollection({100 + q: base.CameraView(c[:4], c[4:8], c[8:], image_name=f"query/{q}.png") for q, c in enumerate(sc["q_cams"])})
    db_segs = {10 + d: sc["db_segs"][d] for d in range(n_db)}
    q_segs = {100 + q: s for q, s in enumerate(sc["q_segs"])}
    T = len(sc["tracks6"])
    members = [([], []) for _ in range(T)]
    for d in range(n_db):
        for j, t in enumerate(sc["db_tracks"][d]):
            if t >= 0:
                members[t][0].append(10 + d)
                members[t][1].append(j)
    linemap = [base.LineTrack(base.Line3d(sc["tracks6"][t][:3], sc["tracks6"][t][3:]), *members[t]) for t in range(T)]
    retrieval = {f"query/{q}.png": [f"db/{d}.png" for d in sc["tasks"][q]] for q in range(len(sc["q_cams"]))}
    corresp = {100 + q: p for q, p in enumerate(sc["points"])}
    return db, qr, db_segs, q_segs, linemap, retrieval, corresp


def cfg(matcher="epipolar", method="hybrid", skip=False, filt=None):
    block = _es.loc_cfg(method=method)
    block.update({"2d_matcher": matcher, "epipolar_filter": False, "IoU_threshold": 0.2, "reprojection_filter": filt, "skip_exists": skip})
    return {"localization": block}
