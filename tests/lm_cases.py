"""Named cases for the minimisers' shared loop (lt_lm.h; tests/lm_oracle.py restates it): every case is a deterministic
one-track or one-problem scene for one kernel, its configuration, the termination code it must end with and the set of
branches of the loop it must take (lm_oracle.branches).  The cases were found on the host twin: rescaling the pixel unit
(kvec and the 2D observations) of a line track, a pose problem or a point track moves the sums of the
linearisation through the ranges where the gradient underflows to zero, the model decrease underflows, the step is
rejected until the radius ends the solve, and H overflows.

run_host / run_device / replay give, per track or problem, the compared fields: p (the final point), cost0, cost1,
iterations, code."""
import ctypes as C
from collections import namedtuple

import numpy as np

import ba_scenes as bs
import lm_oracle as lo
import loc_scenes as ls
import refine_scenes as rs
from limap_amd import _capi
from limap_amd import hybrid_localization as hl

p_ = _capi.ptr
Case = namedtuple("Case", "name kernel build cfg code branches")
FIELDS = ("p", "cost0", "cost1", "iterations", "code")


# ---- k_refine_lm: one line track ----
def line_track(n, scale=1.0, seed=3, n_tracks=12, id_offset=0):
    """track n of make_tracks(n_tracks, seed) alone, the pixel unit rescaled; id_offset: image ids of its own"""
    s = rs.make_tracks(n_tracks, seed=seed)
    a, b = int(s["off"][n]), int(s["off"][n + 1])
    c = np.ascontiguousarray
    return dict(img_ids=c(s["img_ids"] + id_offset, np.int32), k=c(s["k"] * scale), q=s["q"], t=s["t"],
                line6=c(s["line6"][n:n + 1]), off=np.array([0, b - a], np.int64), img=c(s["img"][a:b] + id_offset, np.int32),
                l2d=c(s["l2d"][a:b] * scale), l3d=c(s["l3d"][a:b]))


def edge_track(name, id_offset=0):
    """one of refine_scenes' edge fixtures alone"""
    s = rs.edge_scene()
    n = [x[0] for x in rs.edge_tracks()].index(name)
    a, b = int(s["off"][n]), int(s["off"][n + 1])
    c = np.ascontiguousarray
    return dict(s, img_ids=c(s["img_ids"] + id_offset, np.int32), line6=c(s["line6"][n:n + 1]), off=np.array([0, b - a], np.int64),
                img=c(s["img"][a:b] + id_offset, np.int32), l2d=c(s["l2d"][a:b]), l3d=c(s["l3d"][a:b]))


def concat_lines(scenes):
    """one-track scenes with disjoint image ids as one scene, the tracks in the given order"""
    c = np.ascontiguousarray
    order = np.argsort(np.concatenate([s["img_ids"] for s in scenes]), kind="stable")
    cat = lambda k: c(np.concatenate([s[k] for s in scenes]))  # noqa: E731
    ids = cat("img_ids")
    assert len(set(ids.tolist())) == len(ids)
    off = np.concatenate([[0], np.cumsum([int(s["off"][-1]) for s in scenes])]).astype(np.int64)
    return dict(img_ids=c(ids[order]), k=c(cat("k")[order]), q=c(cat("q")[order]), t=c(cat("t")[order]), line6=cat("line6"),
                off=off, img=cat("img"), l2d=cat("l2d"), l3d=cat("l3d"))


def refine_cfg(**kw):
    c = _capi.LtRefineConfig()
    _capi.load_library().lt_refine_config_default(C.byref(c))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _refine_out(r):
    return [dict(p=r["params"][n], cost0=r["cost"][n, 0], cost1=r["cost"][n, 1], iterations=int(r["iterations"][n]),
                 code=int(r["codes"][n])) for n in range(len(r["codes"]))]


def _refine_run(s, cfg, **kw):
    from limap_amd import optimize
    return _refine_out(optimize.refine_arrays((s["img_ids"], s["k"], s["q"], s["t"]),
                                              (s["line6"], s["off"], s["img"], s["l2d"], s["l3d"]), refine_cfg(**cfg), **kw))


def _refine_replay(s, cfg):
    L = _capi.load_library()
    c = refine_cfg(**cfg)
    out = []
    for n in range(len(s["off"]) - 1):
        cam, sg = rs.track_supports(s, n)
        K = len(sg)

        def ev(p, cam=cam, sg=sg, K=K):
            cost, g, H = C.c_double(), np.zeros(4), np.zeros(16)
            assert L.lt_fn_refine_eval(K, p_(cam, C.c_double), p_(sg, C.c_double), p_(np.ascontiguousarray(p), C.c_double),
                                       c.geometric_alpha, None, C.byref(cost), p_(g, C.c_double), p_(H, C.c_double)) == 0
            return np.float64(cost.value), g, H.reshape(4, 4)
        p0 = np.zeros(6)
        assert L.lt_fn_refine_minimal(p_(np.ascontiguousarray(s["line6"][n]), C.c_double), p_(p0, C.c_double)) == 0
        n_img = len(set(s["img"][s["off"][n]:s["off"][n + 1]].tolist()))
        out.append(lo.solve("rf_lm", ev, p0, c.max_num_iterations, constant=bool(c.constant_line) or n_img < c.min_num_images))
    return out


# ---- k_refine_lm_terms: one line track with the VP and heatmap terms ----
TERMS_COUNTS = (1, 4, 5, 15, 16, 17, 33)
ALL_TERMS = dict(use_vp=1, use_heatmap=1, n_samples_heatmap=11, heatmap_multiplier=0.5)


def terms_track(n, long=False, terms=ALL_TERMS):
    """track n of refine_terms_scenes' scene (supports as TERMS_COUNTS; n = 7: the track whose start cannot be
    evaluated) alone, under the given terms.  long: the supports stretched, so that steps lead into failing samples"""
    import refine_terms_scenes as ts
    s = ts.make_scene(TERMS_COUNTS, seed=1)
    if long:
        s = ts.long_supports(s)
    s = ts.subset(ts.merge(s, ts.failing_track()), [n])
    s["_terms"] = dict(terms)
    return s


def terms_band_track(n, init_sigma=0.3, d=4.5):
    """track n of the same scene started init_sigma off its line, under the geometric and the heatmap term, every heatmap
    +inf further than d pixels from the projection of the start: the start evaluates, a step that crosses the band reads an
    infinite texel and its cost is +inf"""
    import refine_terms_scenes as ts
    s = ts.subset(ts.make_scene(TERMS_COUNTS, seed=1, init_sigma=init_sigma), [n])
    heat = dict(s["heatmaps"])
    row = {int(i): k for k, i in enumerate(s["img_ids"])}
    for i in sorted(set(int(x) for x in s["img"])):
        v = row[i]
        a, b = (ts._project(s["k"][v], s["q"][v], s["t"][v], s["line6"][0, e:e + 3]) for e in (0, 3))
        nrm = np.array([-(b - a)[1], (b - a)[0]]) / np.linalg.norm(b - a)
        yy, xx = np.mgrid[0:heat[i].shape[0], 0:heat[i].shape[1]]
        heat[i] = np.where(np.abs((xx - a[0]) * nrm[0] + (yy - a[1]) * nrm[1]) <= d, heat[i], np.inf)
    s["heatmaps"] = heat
    s["_terms"] = dict(use_heatmap=1)
    return s


def _terms_structs(s, cfg):
    import refine_terms_scenes as ts
    L = _capi.load_library()
    return ts, L, ts.cfg_struct(L, **cfg), ts.terms_struct(L, texel_type=_capi.TEXEL_F16, **s["_terms"])


def _terms_run(s, cfg, ctx=None):
    ts, L, c, t = _terms_structs(s, cfg)
    tex = ts.texels(s, np.float16)
    if ctx is None:
        rc, r = ts.run_host(L, s, c, t, tex, threads=1)
        assert rc == 0, L.lt_fn_refine_host_error()
    else:
        assert ctx.L.lt_refine_set_heatmaps(ctx.h, *ts.heatmap_args(tex), _capi.TEXEL_F16) == 0
        rc, r = ts.run_device(ctx, s, c, t)
        assert rc == 0, ctx.L.lt_last_error(ctx.h)
    return _refine_out(r)


def _terms_replay(s, cfg):
    ts, L, c, t = _terms_structs(s, cfg)
    ids, _, _, arrs = ts.texels(s, np.float16)
    by_id = {int(i): a for i, a in zip(ids, arrs)}
    out = []
    for n in range(len(s["off"]) - 1):
        cam, sg, flag, vp3, hms = ts.track_inputs(s, n, by_id)

        def ev(p, a=(cam, sg), b=(flag, vp3, hms)):
            e = ts.eval_ours(L, a[0], a[1], p, t, *b, alpha=c.geometric_alpha)
            return np.float64(e["cost"]), e["g"], e["H"]
        p0 = np.zeros(6)
        assert L.lt_fn_refine_minimal(p_(np.ascontiguousarray(s["line6"][n]), C.c_double), p_(p0, C.c_double)) == 0
        n_img = len(set(s["img"][s["off"][n]:s["off"][n + 1]].tolist()))
        out.append(lo.solve("rf_lm_terms", ev, p0, c.max_num_iterations, constant=bool(c.constant_line) or n_img < c.min_num_images))
    return out


# ---- k_refine_lm_feat: four tracks, one workgroup ----
FEAT_ITERATIONS = 100


def feat_mix():
    """-> (maps, [four one-track scenes over one image collection], their codes): a start whose reference intersection
    fails (6), a track of three images (5: constant under min_num_images 4), an ordinary track, and a track whose every
    sample is dropped (it runs without the term).  refine_feature_scenes' edge builders, 8 samples"""
    import refine_feature_scenes as fs
    base = fs.make_scene(counts=(5, 4, 6, 4, 5), seed=2)
    fail = fs.failing_scene(8)
    shift = int(base["img_ids"].max()) + 100
    c = np.ascontiguousarray
    cams = {k: c(np.concatenate([base[k], fail[k]])) for k in ("k", "q", "t")}
    cams["img_ids"] = c(np.concatenate([base["img_ids"], fail["img_ids"] + shift]), np.int32)
    maps = {int(i): m.astype(np.float16) for i, m in base["maps"].items()}
    maps.update({int(i) + shift: m.astype(np.float16) for i, m in fail["maps"].items()})
    fail = dict(fail, img=c(fail["img"] + shift, np.int32))
    three = fs.subset(base, [1])
    assert len(set(three["img"].tolist())) == 4
    keep = three["img"] != three["img"][0]
    three = dict(three, img=three["img"][keep], l2d=three["l2d"][keep], l3d=three["l3d"][keep],
                 off=np.array([0, int(keep.sum())], np.int64))
    none_kept = fs.shifted(fs.projected_supports(base, 0), 0.3 + 1e-9)
    scenes = [dict(x, **cams) for x in (fail, three, fs.subset(base, [2]), none_kept)]
    return maps, scenes, [6, 5, None, None]


# ---- k_loc_lm: one pose problem ----
def loc_cfg(**kw):
    c = _capi.LtLocConfig()
    _capi.load_library().lt_loc_config_default(C.byref(c))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def pose_problem(n_lines=6, n_points=8, seed=4, scale=1.0, **kw):
    """loc_scenes.make_problem with the pixel unit rescaled"""
    pr = ls.make_problem(n_lines, n_points, seed=seed, **kw)
    pr = dict(pr, kvec=pr["kvec"] * scale, p2ds=pr["p2ds"] * scale, l2ds=[[sg * scale for sg in g] for g in pr["l2ds"]])
    return pr


def empty_problem(seed=4):
    pr = ls.make_problem(1, 1, seed=seed)
    return dict(pr, l3ds=np.zeros((0, 2, 3)), l2ds=[], p3ds=np.zeros((0, 3)), p2ds=np.zeros((0, 2)))


def _loc_out(r):
    return [dict(p=np.concatenate([r["qvec"][n], r["tvec"][n]]), cost0=r["cost"][n, 0], cost1=r["cost"][n, 1],
                 iterations=int(r["iterations"][n]), code=int(r["codes"][n])) for n in range(len(r["codes"]))]


def _loc_run(problems, cfg, **kw):
    return _loc_out(hl.loc_arrays(hl._problem_arrays(problems), loc_cfg(**cfg), **kw))


def loc_eval_at(cfg_struct, problem, p7):
    """lt_fn_loc_eval_at: the problem at the pose p7 as given -> (cost, g, H)"""
    P, k, q, t, line_off, l3, seg_off, sg, pt_off, p3, p2 = hl._problem_arrays([problem])
    q = np.ascontiguousarray(p7[:4], np.float64)
    t = np.ascontiguousarray(p7[4:], np.float64)
    cost, g, H = np.zeros(1), np.zeros(6), np.zeros((6, 6))
    L = _capi.load_library()
    rc = L.lt_fn_loc_eval_at(p_(k, C.c_double), p_(q, C.c_double), p_(t, C.c_double), int(line_off[-1]), p_(l3, C.c_double),
                             p_(seg_off, C.c_int64), p_(sg, C.c_double), int(pt_off[-1]), p_(p3, C.c_double),
                             p_(p2, C.c_double), C.byref(cfg_struct), None, p_(cost, C.c_double), p_(g, C.c_double),
                             p_(H, C.c_double))
    assert rc == 0, L.lt_fn_loc_host_error()
    return np.float64(cost[0]), g, H


def _loc_replay(problems, cfg):
    c = loc_cfg(**cfg)
    out = []
    for pr in problems:
        nb = sum(len(g) for g in pr["l2ds"]) + len(pr["p3ds"])
        p0 = np.concatenate([lo.normalise_q(pr["qvec"]), np.asarray(pr["tvec"], float)])
        ev = (lambda p, pr=pr: loc_eval_at(c, pr, p)) if nb else None
        out.append(lo.solve("lc_lm", ev, p0, c.max_num_iterations, n_blocks=nb))
    return out


# ---- k_ba_point_lm: one point track under constant poses ----
def point_track(n, scale=1.0, seed=7, obs=(1, 15, 16, 17, 33, 2), id_offset=0):
    """point track n of a six-camera scene alone (obs: the first tracks' observation counts), the pixel unit rescaled"""
    s = bs.without_lines(bs.make_scene(n_cams=6, n_points=9, n_lines=0, seed=seed, point_obs=list(obs)), [])
    a, b = int(s["poff"][n]), int(s["poff"][n + 1])
    c = np.ascontiguousarray
    g = dict(s)
    g.update(img_ids=c(s["img_ids"] + id_offset, np.int32), k=c(s["k"] * scale), p3=c(s["p3"][n:n + 1]),
             poff=np.array([0, b - a], np.int64), pimg=c(s["pimg"][a:b] + id_offset, np.int32), pxy=c(s["pxy"][a:b] * scale))
    return g


def concat_points(scenes):
    c = np.ascontiguousarray
    cat = lambda k: c(np.concatenate([s[k] for s in scenes]))  # noqa: E731
    ids = cat("img_ids")
    assert len(set(ids.tolist())) == len(ids)
    order = np.argsort(ids, kind="stable")
    g = dict(scenes[0])
    g.update(img_ids=c(ids[order]), k=c(cat("k")[order]), q=c(cat("q")[order]), t=c(cat("t")[order]), p3=cat("p3"),
             poff=np.concatenate([[0], np.cumsum([int(s["poff"][-1]) for s in scenes])]).astype(np.int64),
             pimg=cat("pimg"), pxy=cat("pxy"))
    return g


def point_cfg(cfg):
    return bs.cfg_of(constant_pose=1, **cfg)


def _point_out(o):
    """a one-track solve: the separated solve's summary is the track's own"""
    assert len(o["points"]) == 1
    return [dict(p=o["points"][0], cost0=o["cost"][0], cost1=o["cost"][1], iterations=int(o["iterations"][0]), code=int(o["code"][0]))]


def point_eval(s, cfg_struct, track, p3):
    cost, g, H = np.zeros(1), np.zeros(4), np.zeros((4, 4))
    L = _capi.load_library()
    rc = L.lt_fn_ba_point_eval(*bs.args_of(s, cfg_struct), int(track), p_(np.ascontiguousarray(p3, np.float64), C.c_double),
                               p_(cost, C.c_double), p_(g, C.c_double), p_(H, C.c_double))
    assert rc == 0, L.lt_fn_ba_host_error()
    return np.float64(cost[0]), g, H


def _point_replay(s, cfg):
    c = point_cfg(cfg)
    return [lo.solve("ba_point_lm", lambda p, n=n: point_eval(s, c, n, p), s["p3"][n], c.max_num_iterations,
                     constant=bool(c.constant_point)) for n in range(len(s["p3"]))]


# ---- the free-pose bundle adjustment: ba_decide_step ----
def ba_scene(scale, n_cams=3, n_points=6, seed=2):
    """three cameras and six points, no lines, the pixel unit rescaled"""
    s = dict(bs.without_lines(bs.make_scene(n_cams=n_cams, n_points=n_points, n_lines=0, seed=seed), []))
    s["k"], s["pxy"] = np.ascontiguousarray(s["k"] * scale), np.ascontiguousarray(s["pxy"] * scale)
    return s


# at 1e40 the factorisation fails at the radius 1e4 (H overflows) and succeeds at smaller radii: failed attempts, accepted
# and rejected steps in turn, the radius after 55 attempts; at 1e-170 every gradient sum underflows to zero
BA_SCENES = {"failed_factorisations_then_radius": (1e40, 1), "zero_gradient": (1e-170, 2)}
BA_CFG = dict(max_num_iterations=60)


def ba_trace(s, cfg_struct, cap=256):
    """lt_fn_ba_host_trace -> (total0, records (attempts, 5), cost2, iterations, code)"""
    L = _capi.load_library()
    n, t0, rec, cost = np.zeros(1, np.int64), np.zeros(1), np.zeros((cap, 5)), np.zeros(2)
    it, code = np.zeros(1, np.int32), np.zeros(1, np.int32)
    rc = L.lt_fn_ba_host_trace(*bs.args_of(s, cfg_struct), cap, p_(n, C.c_int64), p_(t0, C.c_double), p_(rec, C.c_double),
                               p_(cost, C.c_double), p_(it, C.c_int32), p_(code, C.c_int32))
    assert rc == 0 and n[0] <= cap, L.lt_fn_ba_host_error()
    return np.float64(t0[0]), rec[:int(n[0])], cost, int(it[0]), int(code[0])


def ba_step_is_nan(s, cfg_struct, mu):
    """lt_fn_ba_eval reports a NaN step at the radius mu: a factorisation failed"""
    L = _capi.load_library()
    dims = np.zeros(4, np.int64)
    assert L.lt_fn_ba_eval(*bs.args_of(s, cfg_struct), None, p_(dims, C.c_int64), None, None, None, None, None, float(mu), None) == 0
    st = np.zeros(int(dims[2]))
    assert L.lt_fn_ba_eval(*bs.args_of(s, cfg_struct), None, p_(dims, C.c_int64), None, None, None, None, None, float(mu),
                           p_(st, C.c_double)) == 0
    return bool(np.all(np.isnan(st)))


# ---- the three kernels under one surface ----
def run_host(case):
    s = case.build()
    if case.kernel == "refine":
        return _refine_run(s, case.cfg, host_threads=1)
    if case.kernel == "refine_terms":
        return _terms_run(s, case.cfg)
    if case.kernel == "loc":
        return _loc_run([s], case.cfg, host_threads=1)
    rc, o = bs.run_host(s, point_cfg(case.cfg), 1)
    assert rc == 0
    return _point_out(o)


def run_device(case, ctx):
    s = case.build()
    if case.kernel == "refine":
        return _refine_run(s, case.cfg, ctx=ctx)
    if case.kernel == "refine_terms":
        return _terms_run(s, case.cfg, ctx=ctx)
    if case.kernel == "loc":
        return _loc_run([s], case.cfg, ctx=ctx)
    rc, o = bs.run_device(ctx, s, point_cfg(case.cfg))
    assert rc == 0
    return _point_out(o)


def replay(case):
    s = case.build()
    if case.kernel == "refine":
        return _refine_replay(s, case.cfg)
    if case.kernel == "refine_terms":
        return _terms_replay(s, case.cfg)
    if case.kernel == "loc":
        return _loc_replay([s], case.cfg)
    return _point_replay(s, case.cfg)


def same(a, b):
    """two results agree bit for bit in every compared field (a NaN equals a NaN)"""
    return (np.array_equal(np.asarray(a["p"]), np.asarray(b["p"]), equal_nan=True) and a["iterations"] == b["iterations"] and
            a["code"] == b["code"] and all(np.array_equal(np.float64(a[k]), np.float64(b[k]), equal_nan=True) for k in ("cost0", "cost1")))


def points_only(scale):
    pr = pose_problem(n_lines=1, n_points=8, scale=scale)
    return dict(pr, l3ds=np.zeros((0, 2, 3)), l2ds=[])


EDGE = dict(min_num_images=1, num_outliers_aggregator=0, max_num_iterations=200)
IT = lambda n: dict(max_num_iterations=n)  # noqa: E731
_SPECS = [
    # ---- the line chart through rf_lm (k_refine_lm) ----
    ("line_ordinary", "refine", lambda **kw: line_track(2, **kw), IT(200)),
    ("line_ordinary_17_supports", "refine", lambda **kw: line_track(0, **kw), IT(200)),
    ("line_max_iter_0", "refine", lambda **kw: line_track(2, **kw), IT(0)),
    ("line_max_iter_1", "refine", lambda **kw: line_track(2, **kw), IT(1)),
    ("line_cap_after_accept", "refine", lambda **kw: line_track(2, **kw), IT(3)),
    ("line_constant", "refine", lambda **kw: line_track(3, **kw), IT(200)),
    ("line_zero_gradient", "refine", lambda **kw: line_track(0, 1e-100, **kw), IT(200)),
    ("line_zero_gradient_origin_parallel", "refine", lambda **kw: edge_track("origin_parallel", **kw), EDGE),
    ("line_bad_model_at_0", "refine", lambda **kw: line_track(0, 1e-60, **kw), IT(200)),
    ("line_bad_model_after_rejections", "refine", lambda **kw: line_track(0, 1e-40, **kw), IT(200)),
    ("line_radius_without_accept", "refine", lambda **kw: line_track(0, 1e-36, **kw), IT(200)),
    ("line_radius_cap_14", "refine", lambda **kw: line_track(0, 1e-36, **kw), IT(14)),
    ("line_radius_cap_15", "refine", lambda **kw: line_track(0, 1e-36, **kw), IT(15)),
    ("line_radius_cap_16", "refine", lambda **kw: line_track(0, 1e-36, **kw), IT(16)),
    ("line_bad_pivot_after_accept_26_supports", "refine", lambda **kw: line_track(6, 1e44, **kw), IT(200)),
    ("line_bad_pivot_at_0", "refine", lambda **kw: line_track(0, 1e80, **kw), IT(200)),
    ("line_start_not_finite", "refine", lambda **kw: edge_track("origin_perpendicular", **kw), dict(EDGE, geometric_alpha=500.0)),
    # ---- the line chart through rf_lm_terms (k_refine_lm_terms) ----
    ("terms_ordinary_33_supports", "refine_terms", lambda: terms_track(6), EDGE),
    ("terms_ordinary_17_supports", "refine_terms", lambda: terms_track(5), EDGE),
    ("terms_long_supports_radius_cap", "refine_terms", lambda: terms_track(3, long=True), EDGE),
    ("terms_step_into_infinite_texels", "refine_terms", lambda: terms_band_track(5), EDGE),
    ("terms_bad_pivot_after_infinite_step", "refine_terms", lambda: terms_band_track(6), EDGE),
    ("terms_one_support_constant", "refine_terms", lambda: terms_track(0), dict(EDGE, min_num_images=2)),
    ("terms_start_not_finite", "refine_terms", lambda: terms_track(7), EDGE),
    ("terms_constant_before_start_not_finite", "refine_terms", lambda: terms_track(7), dict(EDGE, min_num_images=5)),
    # ---- the pose chart through lc_lm (k_loc_lm) ----
    ("pose_ordinary", "loc", lambda: pose_problem(), IT(200)),
    ("pose_cap", "loc", lambda: pose_problem(), IT(5)),
    ("pose_max_iter_0", "loc", lambda: pose_problem(), IT(0)),
    ("pose_zero_gradient", "loc", lambda: points_only(1e-170), IT(200)),
    ("pose_bad_model_at_0", "loc", lambda: pose_problem(scale=1e-100), IT(200)),
    ("pose_radius_without_accept", "loc", lambda: pose_problem(scale=1e-60), IT(200)),
    ("pose_bad_pivot_finite_start", "loc", lambda: pose_problem(scale=1e151), IT(200)),
    ("pose_start_not_finite", "loc", lambda: pose_problem(scale=1e153), IT(200)),
    ("pose_no_residuals", "loc", lambda: empty_problem(), IT(200)),
    # ---- the point chart through ba_point_lm (k_ba_point_lm) ----
    ("point_zero_gradient_after_accept", "ba_point", lambda **kw: point_track(0, **kw), IT(200)),
    ("point_ordinary", "ba_point", lambda **kw: point_track(5, **kw), IT(200)),
    ("point_ordinary_33_blocks", "ba_point", lambda **kw: point_track(4, **kw), IT(200)),
    ("point_max_iter_1", "ba_point", lambda **kw: point_track(5, **kw), IT(1)),
    ("point_bad_model_at_0", "ba_point", lambda **kw: point_track(0, 1e-100, **kw), IT(200)),
    ("point_radius_without_accept", "ba_point", lambda **kw: point_track(1, 1e-60, **kw), IT(200)),
    ("point_bad_pivot_finite_start", "ba_point", lambda **kw: point_track(0, 1e44, **kw), IT(200)),
    ("point_bad_pivot_after_accept", "ba_point", lambda **kw: point_track(0, 1e62, **kw), IT(200)),
    ("point_start_not_finite", "ba_point", lambda **kw: point_track(1, 1e160, **kw), IT(200)),
]

# name: (code, branches); recorded from the replay, which equals the host twin bit for bit on every case
EXPECT = {
    "line_ordinary": (1, {'accept', 'grow_above_floor', 'grow_floor', 'radius_cap', 'radius_exit', 'radius_exit_early', 'reject_then_accept', 'three_rejections'}),  # 62 iterations
    "line_ordinary_17_supports": (1, {'accept', 'grow_floor', 'radius_exit', 'radius_exit_early', 'reject_then_accept', 'three_rejections'}),  # 35 iterations
    "line_max_iter_0": (0, {'max_iter_0'}),  # 0 iterations
    "line_max_iter_1": (0, {'accept', 'cap_after_accept', 'grow_above_floor', 'max_iter_1'}),  # 1 iterations
    "line_cap_after_accept": (0, {'accept', 'cap_after_accept', 'grow_above_floor', 'grow_floor'}),  # 3 iterations
    "line_constant": (5, {'code5'}),  # 0 iterations
    "line_zero_gradient": (2, {'zero_gradient_at_0'}),  # 0 iterations
    "line_zero_gradient_origin_parallel": (2, {'zero_gradient_at_0'}),  # 0 iterations
    "line_bad_model_at_0": (4, {'bad_model_at_0'}),  # 0 iterations
    "line_bad_model_after_rejections": (4, {'bad_model_after_rejections', 'three_rejections'}),  # 14 iterations
    "line_radius_without_accept": (1, {'radius_exit', 'radius_exit_early', 'three_rejections'}),  # 15 iterations
    "line_radius_cap_14": (0, {'cap_after_reject', 'three_rejections'}),  # 14 iterations
    "line_radius_cap_15": (1, {'radius_exit', 'radius_exit_on_cap', 'three_rejections'}),  # 15 iterations
    "line_radius_cap_16": (1, {'radius_exit', 'radius_exit_one_before_cap', 'three_rejections'}),  # 15 iterations
    "line_bad_pivot_after_accept_26_supports": (3, {'accept', 'bad_pivot_after_accept', 'grow_floor'}),  # 7 iterations
    "line_bad_pivot_at_0": (3, {'bad_pivot_at_0_finite_start'}),  # 0 iterations
    "line_start_not_finite": (3, {'bad_pivot_at_0_start_not_finite'}),  # 0 iterations
    "terms_ordinary_33_supports": (1, {'accept', 'grow_floor', 'radius_exit', 'radius_exit_early', 'reject_then_accept', 'three_rejections'}),  # 32 iterations
    "terms_ordinary_17_supports": (1, {'accept', 'grow_floor', 'radius_exit', 'radius_exit_early', 'three_rejections'}),  # 21 iterations
    "terms_long_supports_radius_cap": (1, {'accept', 'grow_floor', 'radius_cap', 'radius_exit', 'radius_exit_early', 'reject_then_accept', 'three_rejections'}),  # 83 iterations
    "terms_step_into_infinite_texels": (1, {'accept', 'grow_floor', 'radius_exit', 'radius_exit_early', 'reject_cost_not_finite', 'reject_then_accept', 'three_rejections'}),  # 82 iterations
    "terms_bad_pivot_after_infinite_step": (3, {'accept', 'bad_pivot_after_accept', 'grow_floor', 'reject_cost_not_finite', 'reject_then_accept', 'three_rejections'}),  # 7 iterations
    "terms_one_support_constant": (5, {'code5'}),  # 0 iterations
    "terms_start_not_finite": (6, {'code6'}),  # 0 iterations
    "terms_constant_before_start_not_finite": (5, {'code5'}),  # 0 iterations
    "pose_ordinary": (1, {'accept', 'grow_floor', 'radius_exit', 'radius_exit_early', 'reject_then_accept', 'three_rejections'}),  # 28 iterations
    "pose_cap": (0, {'accept', 'cap_after_reject', 'grow_floor'}),  # 5 iterations
    "pose_max_iter_0": (0, {'max_iter_0'}),  # 0 iterations
    "pose_zero_gradient": (2, {'zero_gradient_at_0'}),  # 0 iterations
    "pose_bad_model_at_0": (4, {'bad_model_at_0'}),  # 0 iterations
    "pose_radius_without_accept": (1, {'radius_exit', 'radius_exit_early', 'three_rejections'}),  # 15 iterations
    "pose_bad_pivot_finite_start": (3, {'bad_pivot_at_0_finite_start'}),  # 0 iterations
    "pose_start_not_finite": (6, {'code6'}),  # 0 iterations
    "pose_no_residuals": (7, {'code7'}),  # 0 iterations
    "point_zero_gradient_after_accept": (2, {'accept', 'grow_floor', 'zero_gradient_after_accept'}),  # 4 iterations
    "point_ordinary": (1, {'accept', 'grow_above_floor', 'grow_floor', 'radius_exit', 'radius_exit_early', 'reject_then_accept', 'three_rejections'}),  # 24 iterations
    "point_ordinary_33_blocks": (1, {'accept', 'grow_floor', 'radius_exit', 'radius_exit_early', 'reject_then_accept', 'three_rejections'}),  # 22 iterations
    "point_max_iter_1": (0, {'accept', 'cap_after_accept', 'grow_floor', 'max_iter_1'}),  # 1 iterations
    "point_bad_model_at_0": (4, {'bad_model_at_0'}),  # 0 iterations
    "point_radius_without_accept": (1, {'radius_exit', 'radius_exit_early', 'three_rejections'}),  # 15 iterations
    "point_bad_pivot_finite_start": (3, {'bad_pivot_at_0_finite_start'}),  # 0 iterations
    "point_bad_pivot_after_accept": (3, {'accept', 'bad_pivot_after_accept', 'grow_floor'}),  # 1 iterations
    "point_start_not_finite": (6, {'code6'}),  # 0 iterations
}

CASES = [Case(n, k, b, c, *EXPECT.get(n, (None, None))) for n, k, b, c in _SPECS]
BY_NAME = {c.name: c for c in CASES}

# every branch of the loop some case must take (test_lm_host.py checks the union)
BRANCHES = {
    "zero_gradient_at_0", "zero_gradient_after_accept", "bad_pivot_at_0_start_not_finite", "bad_pivot_at_0_finite_start",
    "bad_pivot_after_accept", "bad_model_at_0", "bad_model_after_rejections", "accept", "reject_then_accept", "three_rejections", "radius_exit",
    "radius_exit_on_cap", "radius_exit_one_before_cap", "radius_cap", "grow_floor", "grow_above_floor", "max_iter_0",
    "max_iter_1", "cap_after_accept", "cap_after_reject", "reject_cost_not_finite", "code5", "code6", "code7",
}
# not reached through a kernel by any case found (rescaling the pixel unit of line tracks, pose problems and point tracks
# over 1e-170 .. 1e160): a model decrease that is not positive after accepted steps -- where the sums are small enough
# for it, the first step already has it.  test_lm_host.py reaches it through lt_fn_lm_loop_script
UNREACHED = {"bad_model_after_accept"}
