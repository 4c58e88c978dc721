"""The feature-consistency term of the line refinement on the host path: lt_fn_refine_eval_feature
and lt_fn_refine_host_feature against the NumPy restatement of tests/refine_feature_oracle.py, the edges of the sample
selection and of the sampling, and the Python surface.  No GPU."""
import glob
import os

import numpy as np
import pytest

import refine_feature_oracle as fo
import refine_feature_scenes as fs
import refine_oracle as ro
from limap_amd import features, optimize

# |cost_f64 - cost_longdouble| / cost_longdouble of the restatement on the scene below, both forms, all tracks: measured
# 3.1e-13 at most (the sums of 128 squares and the logarithm in float64).  The bound is 8 times that; the float64
# restatement alone stays inside it, which test_cost_agrees_with_the_longdouble_restatement asserts too.
COST_DISTANCE = 3.1e-13
COST_RTOL = 8 * COST_DISTANCE
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refine_feature")
GOLDEN_IN = ("img_ids", "k", "q", "t", "line6", "off", "img", "l2d", "l3d")


@pytest.fixture(scope="module")
def scene():
    return fs.make_scene()


@pytest.fixture(scope="module")
def sources(scene):
    """{(form, dtype): the patches or maps in that texel type}"""
    out = {}
    for dt in ("float16", "float32"):
        out[("patch", dt)] = fs.patches_of(scene, dt)
        out[("map", dt)] = fs.texel_maps(scene, dt)
    return out


def oracle(s, n, grids, p=None, dtype=np.float64, smps=None, **kw):
    a, b = int(s["off"][n]), int(s["off"][n + 1])
    p = ro.minimal(s["line6"][n]) if p is None else p
    return fo.evaluate(s["line6"][n], s["img"][a:b], s["l2d"][a:b], fs.cams_of(s), grids, p, n_samples=kw.pop("n_samples", 8),
                       dtype=dtype, smps=smps, **kw)


def same_samples(a, b):
    return len(a) == len(b) and all(x[0] == y[0] and np.array_equal(x[1], y[1]) and x[2] == y[2] for x, y in zip(a, b))


# ---- 1. against the restatement ----
@pytest.mark.parametrize("form", ["patch", "map"])
@pytest.mark.parametrize("dt", ["float16", "float32"])
def test_samples_and_residuals_equal_the_restatement_bit_for_bit(scene, sources, form, dt):
    rf = fs.refine_cfg(dtype=dt)
    for n in range(len(scene["line6"])):
        g = fs.oracle_grids(scene, n, form, sources[(form, dt)])
        ours, e = fs.eval_ours(scene, n, rf, g), oracle(scene, n, g)
        assert len(e["samples"]) > 0 and e["r"].shape[0] > 0
        assert same_samples(ours["samples"], e["samples"]), "kept samples, reference choices, target lists"
        assert ours["r"].tobytes() == e["r"].astype(np.float64).tobytes(), "the 128 residuals of every block"
        assert not ours["failed"].any() and not e["failed"].any()
        assert np.allclose(ours["g"], e["g"], rtol=1e-9, atol=1e-12) and np.allclose(ours["H"], e["H"], rtol=1e-9, atol=1e-12)
    if form == "patch":
        assert any(not np.allclose(g[i][1], np.eye(2)) for i in g), "a rotated patch (R is not the identity)"


def test_cost_agrees_with_the_longdouble_restatement(scene, sources):
    """The host's cost against the longdouble restatement within COST_RTOL = 8 x COST_DISTANCE; the distance between the
    float64 and the longdouble restatement, measured on these scenes (3.1e-13 at most), is printed and held to the same
    bound."""
    worst_o = worst_h = 0.0
    for form in ("patch", "map"):
        for n in range(len(scene["line6"])):
            g = fs.oracle_grids(scene, n, form, sources[(form, "float16")])
            e = oracle(scene, n, g)
            el = oracle(scene, n, g, dtype=np.longdouble, smps=e["samples"])
            ours = fs.eval_ours(scene, n, fs.refine_cfg(), g)
            worst_o = max(worst_o, float(abs(e["cost"] - el["cost"]) / el["cost"]))
            worst_h = max(worst_h, float(abs(np.longdouble(ours["cost"]) - el["cost"]) / el["cost"]))
    print(f"float64 restatement to longdouble {worst_o:.3g}, host to longdouble {worst_h:.3g}, bound {COST_RTOL:.3g}")
    assert worst_o <= COST_RTOL and worst_h <= COST_RTOL


def test_feature_only_cost_and_other_parameters(scene, sources):
    """use_geometric off, and parameters away from the initial line: the samples stay those of the initial line"""
    g = fs.oracle_grids(scene, 1, "patch", sources[("patch", "float16")])
    p = ro.retract(ro.minimal(scene["line6"][1]), np.array([0.002, -0.001, 0.0015, 0.003]))
    rf = fs.refine_cfg(use_geometric=False)
    ours, e = fs.eval_ours(scene, 1, rf, g, p=p), oracle(scene, 1, g, p=p, use_geometric=False)
    assert same_samples(ours["samples"], e["samples"]) and ours["r"].tobytes() == e["r"].tobytes()
    assert np.isclose(ours["cost"], float(e["cost"]), rtol=COST_RTOL)


# ---- 2. the minimiser ----
@pytest.mark.parametrize("form", ["patch", "map"])
def test_minimiser(scene, sources, form):
    """The final cost is not above the initial one, the line ends nearer the true line than it began (initial ends off
    by N(0, 0.004)), the returned cost is the restatement's at the returned line (rtol 1e-9, the bound
    test_refine_terms_host.py holds the heatmap term to -- it has no gradient bound to borrow), and the projected
    gradient there is smaller than at the start."""
    rf = fs.refine_cfg(max_num_iterations=30)
    r = fs.run(scene, rf, form, sources[(form, "float16")], host_threads=4)
    assert np.all(r["cost"][:, 1] <= r["cost"][:, 0]) and np.all(r["iterations"] > 0)
    for n in range(len(scene["line6"])):
        assert fs.line_distance(r["segments"][n], scene["gt6"][n]) < fs.line_distance(scene["line6"][n], scene["gt6"][n])
        g = fs.oracle_grids(scene, n, form, sources[(form, "float16")])
        e0, e1 = oracle(scene, n, g), oracle(scene, n, g, p=r["params"][n])
        assert np.isclose(float(e1["cost"]), r["cost"][n, 1], rtol=1e-9) and np.isclose(float(e0["cost"]), r["cost"][n, 0], rtol=1e-9)
        assert np.linalg.norm(e1["g"]) < np.linalg.norm(e0["g"])


# ---- 3. sample selection edges ----
@pytest.fixture(scope="module")
def exact(scene):
    """track 0 with one support per image, each exactly the projection of the initial line"""
    return fs.projected_supports(scene, 0)


def _eval(o, maps, **kw):
    g = fs.oracle_grids(o, 0, "map", maps)
    rf = fs.refine_cfg(**kw)
    ours, e = fs.eval_ours(o, 0, rf, g), oracle(o, 0, g)
    assert same_samples(ours["samples"], e["samples"]) and ours["r"].tobytes() == e["r"].tobytes()
    assert (np.isinf(ours["cost"]) and np.isinf(e["cost"])) or np.isclose(ours["cost"], float(e["cost"]), rtol=COST_RTOL)
    return ours


def test_good_support_threshold(exact, sources):
    """all supports 0.3 -+ 1e-9 px beside the projection: just below every sample is kept, just above none is"""
    maps = sources[("map", "float16")]
    below, above = _eval(fs.shifted(exact, 0.3 - 1e-9), maps), _eval(fs.shifted(exact, 0.3 + 1e-9), maps)
    assert len(below["samples"]) > 0 and len(above["samples"]) == 0 and above["r"].shape[0] == 0


def test_one_support_points_are_dropped_and_the_weight_counts_the_kept(exact, sources):
    """the first support covers the first half, the others the rest: points with one support drop, so n_kept (2) is not
    n_samples_feature (8) and the cost -- equal to the restatement's, which divides by n_kept / 100 -- says so"""
    K = len(exact["img"])
    o = fs.trimmed(exact, [(0.0, 0.5)] + [(0.6, 1.0)] * (K - 1))
    ours = _eval(o, sources[("map", "float16")])
    assert 0 < len(ours["samples"]) < 8
    e = oracle(o, 0, fs.oracle_grids(o, 0, "map", sources[("map", "float16")]))
    n_kept, n_tgt = len(e["samples"]), len(e["samples"][0][2])
    assert e["weights"][0] == 1.0 / ((n_kept / 100.0) * (n_tgt / 5.0)) != 1.0 / ((8 / 100.0) * (n_tgt / 5.0))


def test_all_supports_of_a_point_in_one_image_leave_no_target(exact, sources):
    """two supports of the first image cover the first half alone: those samples are kept without targets, add no block
    and still count in n_kept"""
    K = len(exact["img"])
    o = dict(exact)
    for key in ("img", "l2d", "l3d"):
        o[key] = np.concatenate([exact[key][:1], exact[key]])
    o["off"] = np.array([0, K + 1], np.int64)
    o = fs.trimmed(o, [(0.0, 0.5), (0.0, 0.45)] + [(0.6, 1.0)] * (K - 1))
    ours = _eval(o, sources[("map", "float16")])
    n_tgt = [len(x[2]) for x in ours["samples"]]
    assert 0 in n_tgt and max(n_tgt) > 0 and ours["r"].shape[0] == sum(n_tgt)


def test_length_tie_goes_to_the_first_support(exact, sources):
    t = fs.length_tie(exact, 0, 1)
    assert t is not None, "no end within 400 ulps gives the same length"
    K = len(exact["img"])
    t = fs.trimmed(t, [(0, 1), (0, 1)] + [(0.1, 0.8)] * (K - 2))
    a, b = _eval(t, sources[("map", "float16")]), _eval(fs.swapped(t, 0, 1), sources[("map", "float16")])
    assert {x[0] for x in a["samples"]} == {int(t["img"][0])} and {x[0] for x in b["samples"]} == {int(t["img"][1])}


def test_every_sample_dropped_is_the_run_without_the_term(exact, sources):
    o = fs.shifted(exact, 0.3 + 1e-9)
    maps = sources[("map", "float16")]
    with_f = fs.run(o, fs.refine_cfg(), "map", maps, host_threads=2)
    without = fs.run(o, fs.refine_cfg(use_feature=False), None, None, host_threads=2)
    fs.same_bits(with_f, without, "no kept sample")
    assert with_f["iterations"][0] > 0


# ---- 4. sampling edges ----
def test_clamp_on_and_beyond_a_patch_border(scene):
    """patches one pixel wide on either side of the line and without stretch: intersections fall on and beyond their
    border, where Grid2D's clamp applies on both sides"""
    cfg = dict(fs.PATCH_CFG, patch=dict(k_stretch=1.0, t_stretch=0, range_perp=1))
    pat = features.extract_track_patches(cfg, fs.tracks_of(scene), fs.imagecols(scene), scene["maps"], host=True, dtype="float16")
    beyond = 0
    for n in range(len(scene["line6"])):
        g = fs.oracle_grids(scene, n, "patch", pat)
        ours, e = fs.eval_ours(scene, n, fs.refine_cfg(), g), oracle(scene, n, g)
        assert same_samples(ours["samples"], e["samples"]) and ours["r"].tobytes() == e["r"].tobytes()
        b = 0
        for ref, _, tgts in e["samples"]:
            for tg in tgts:
                arr, R, tv = g[tg]
                lx, ly = fo.to_local(g[tg], e["xy_tgt"][b][0], e["xy_tgt"][b][1], np.float64)
                beyond += not (0 <= lx <= arr.shape[1] - 2 and 0 <= ly <= arr.shape[0] - 2)
                b += 1
    assert beyond > 0


def test_map_form_at_the_image_border(scene, sources):
    """maps cut to their left 30 columns and top 20 rows: intersections beyond the border read the clamped texels"""
    maps = {i: np.ascontiguousarray(m[:20, :30]) for i, m in sources[("map", "float16")].items()}
    out = 0
    for n in range(len(scene["line6"])):
        g = fs.oracle_grids(scene, n, "map", maps)
        ours, e = fs.eval_ours(scene, n, fs.refine_cfg(), g), oracle(scene, n, g)
        assert ours["r"].tobytes() == e["r"].tobytes()
        out += int(((e["xy_ref"][:, 0] > 29) | (e["xy_ref"][:, 1] > 19)).sum())
    assert out > 0


def test_failed_intersection_at_the_initial_line_is_code_6():
    f = fs.failing_scene()
    maps = {i: m.astype(np.float16) for i, m in f["maps"].items()}
    g = {i: (maps[i], np.eye(2), np.zeros(2)) for i in maps}
    ours, e = fs.eval_ours(f, 0, fs.refine_cfg(), g), oracle(f, 0, g)
    assert same_samples(ours["samples"], e["samples"]) and len(ours["samples"]) == 1
    assert ours["failed"].all() and e["failed"].all() and np.isinf(ours["cost"])
    r = fs.run(f, fs.refine_cfg(), "map", maps, host_threads=1)
    assert r["codes"][0] == 6 and r["iterations"][0] == 0 and np.all(np.isinf(r["cost"]))
    assert np.array_equal(r["params"][0], ro.minimal(f["line6"][0])), "the line is kept"


# ---- goldens (tests/golden/make_refine_feature_golden.py) ----
def golden_maps(z, dtype):
    """the texel maps of a golden from their recipe: make_scene's arguments, or the zero maps of failing_scene"""
    if "maps_seed" in z:
        src = fs.make_scene(counts=tuple(int(c) for c in z["maps_counts"]), seed=int(z["maps_seed"]))["maps"]
    else:
        src = fs.failing_scene()["maps"]
    return {i: m.astype(dtype) for i, m in src.items()}


def run_golden(z, maps, host_threads=None):
    """the solve of a golden's inputs on the host (host_threads) or on the device"""
    s = {k: np.ascontiguousarray(z[k]) for k in GOLDEN_IN}
    s["gt6"] = s["line6"]
    cfg = {k[4:]: np.asarray(z[k]).item() for k in z if k.startswith("cfg_")}
    rf = fs.refine_cfg(**cfg)
    on_host = host_threads is not None
    vp = (np.ascontiguousarray(z["vp_flag"]), np.ascontiguousarray(z["vp3"])) if "vp_flag" in z else None
    heat = None
    if rf.use_heatmap:  # some_heatmaps of the regenerated float64 maps: the texel type rounds them once
        f64 = fs.make_scene(counts=tuple(int(c) for c in z["maps_counts"]), seed=int(z["maps_seed"]))
        heat = optimize.Heatmaps(fs.some_heatmaps(f64), cfg["dtype"])
    return fs.run(s, rf, "map", maps, host_threads=host_threads, vp=vp, heatmaps=heat) if on_host else \
        fs.run(s, rf, "map", maps, vp=vp, heatmaps=heat)


def load_golden(path):
    """-> the file's arrays, the regenerated maps (their digests checked), the recorded outputs"""
    z = dict(np.load(path))
    maps = golden_maps(z, str(z["cfg_dtype"]))
    got = [fs.texel_digest(maps[int(i)]) for i in z["img_ids"]]
    assert got == list(z["maps_sha256"]), "the regenerated feature maps are not the recorded ones"
    return z, maps, {k: z["out_" + k] for k in fs.RESULT_KEYS}


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "*.npz"))))
def test_goldens_reproduce(path):
    z, maps, want = load_golden(path)
    r = run_golden(z, maps, host_threads=4)
    for k in fs.RESULT_KEYS:
        assert np.array_equal(r[k], want[k]), (os.path.basename(path), k)


def test_goldens_exist():
    assert len(glob.glob(os.path.join(GOLDEN, "*.npz"))) >= 4


# ---- 5. forms and texel types ----
def test_texel_types(scene, sources):
    """float64 input with dtype float16 is one astype; float32 texels keep what binary16 rounds away"""
    rf = fs.refine_cfg()
    from_f64 = fs.run(scene, rf, "map", scene["maps"], host_threads=2)
    from_f16 = fs.run(scene, rf, "map", sources[("map", "float16")], host_threads=2)
    fs.same_bits(from_f64, from_f16, "one astype(np.float16)")
    f32 = fs.run(scene, fs.refine_cfg(dtype="float32"), "map", scene["maps"], host_threads=2)
    assert not np.array_equal(f32["params"], from_f16["params"])
    h = optimize.FeatureMaps(scene["maps"], "float16", host=True)
    assert all(a.dtype == np.float16 and np.array_equal(a, scene["maps"][int(i)].astype(np.float16)) for i, a in zip(h.ids, h.keep))


# ---- 6. the Python surface ----
CFG = dict(min_num_images=4, use_geometric=True, use_feature=True, n_samples_feature=8, dtype="float16")


def _lines(tracks):
    return np.array([np.concatenate([t.line.start, t.line.end]) for t in tracks])


def test_value_errors(scene, sources):
    tracks, ic = fs.tracks_of(scene), fs.imagecols(scene)
    pat, maps = sources[("patch", "float16")], sources[("map", "float16")]
    ids = tracks[0].GetSortedImageIds()
    views = [ic.camview(i) for i in ids]
    pp, pf = [pat[(0, i)] for i in ids], [maps[i] for i in ids]
    with pytest.raises(ValueError, match="use_ref_descriptor"):
        optimize.line_refinement(dict(CFG, use_ref_descriptor=True), tracks, ic, featuremaps=maps, host_threads=1)
    optimize.RefinementConfig(dict(CFG, use_ref_descriptor=False, ref_multiplier=3.0))._check()
    with pytest.raises(ValueError, match="channels"):
        optimize.line_refinement(dict(CFG, channels=64), tracks, ic, featuremaps=maps, host_threads=1)
    with pytest.raises(ValueError, match="dtype"):
        optimize.line_refinement(dict(CFG, dtype="float64"), tracks, ic, featuremaps=maps, host_threads=1)
    with pytest.raises(ValueError, match="use_feature"):
        optimize.line_refinement(dict(CFG), tracks, ic, host_threads=1)
    with pytest.raises(ValueError, match="use_feature"):
        optimize.solve_line_bundle_adjustment(dict(CFG, constant_intrinsics=True, constant_pose=True), ic, tracks, host_threads=1)
    with pytest.raises(ValueError, match="use_feature"):
        optimize.solve_line_refinement(dict(CFG), tracks[0], views, host_threads=1)
    with pytest.raises(ValueError, match="p_patches"):
        optimize.solve_line_refinement(dict(CFG), tracks[0], views, p_patches=pp[:-1], host_threads=1)
    with pytest.raises(ValueError, match="p_features"):
        optimize.solve_line_refinement(dict(CFG), tracks[0], views, p_features=pf[:-1], host_threads=1)
    with pytest.raises(ValueError, match="p_patches and p_features"):
        optimize.solve_line_refinement(dict(CFG), tracks[0], views, p_patches=pp, p_features=pf, host_threads=1)
    with pytest.raises(ValueError, match="p_features"):
        optimize.solve_line_refinement(dict(CFG, use_feature=False), tracks[0], views, p_features=pf, host_threads=1)
    with pytest.raises(ValueError, match="track 1, image"):
        optimize.line_refinement(dict(CFG), tracks, ic, patches={k: v for k, v in pat.items() if k[0] != 1}, host_threads=1)
    with pytest.raises(ValueError, match="track 0, image"):
        optimize.line_refinement(dict(CFG), tracks, ic, featuremaps={i: m for i, m in maps.items() if i != ids[0]}, host_threads=1)
    with pytest.raises(ValueError, match="128"):
        optimize.solve_line_refinement(dict(CFG), tracks[0], views, p_features=[m[:, :, :64] for m in pf], host_threads=1)
    with pytest.raises(ValueError, match="PatchInfo"):
        optimize.solve_line_refinement(dict(CFG), tracks[0], views, p_patches=[1] * len(ids), host_threads=1)


def test_python_surface(scene, sources, tmp_path):
    """per track is the scene call; patch_dir is patches, featuremap_dir is featuremaps; a budget of one byte -- one
    track per native call -- is one call"""
    tracks, ic = fs.tracks_of(scene), fs.imagecols(scene)
    short = fs.tracks_of(fs.subset(fs.make_scene(counts=(3,), seed=3), [0]))[0]  # below min_num_images: passes through
    tracks = tracks + [short]
    pat, maps = sources[("patch", "float16")], sources[("map", "float16")]
    by_p = optimize.line_refinement(dict(CFG), tracks, ic, patches=pat, host_threads=2)
    by_m = optimize.line_refinement(dict(CFG), tracks, ic, featuremaps=maps, host_threads=2)
    assert by_p[-1] is short and by_m[-1] is short
    assert not np.array_equal(_lines(by_p[:-1]), _lines(tracks[:-1])) and not np.array_equal(_lines(by_p[:-1]), _lines(by_m[:-1]))
    one = optimize.line_refinement(dict(CFG), tracks, ic, patches=pat, host_threads=2, patch_bytes=1)
    assert np.array_equal(_lines(one), _lines(by_p)), "one track per native call"
    for n, t in enumerate(tracks[:-1]):
        ids = t.GetSortedImageIds()
        views = [ic.camview(i) for i in ids]
        e = optimize.solve_line_refinement(dict(CFG), t, views, p_patches=[pat[(n, i)] for i in ids], host_threads=1)
        assert np.array_equal(np.concatenate([e.GetLine3d().start, e.GetLine3d().end]), _lines(by_p)[n])
        e = optimize.solve_line_refinement(dict(CFG), t, views, p_features=[maps[i] for i in ids], host_threads=1)
        assert np.array_equal(np.concatenate([e.GetLine3d().start, e.GetLine3d().end]), _lines(by_m)[n])
    assert optimize.solve_line_refinement(dict(CFG), short, [ic.camview(i) for i in short.GetSortedImageIds()],
                                          p_features=[maps[i] for i in short.GetSortedImageIds()], host_threads=1) is None
    pdir, fdir = str(tmp_path / "patches"), str(tmp_path / "maps")
    features.extract_track_patches(dict(fs.PATCH_CFG), tracks, ic, scene["maps"], output_dir=pdir, host=True)
    os.makedirs(fdir)
    for i, m in maps.items():
        np.save(os.path.join(fdir, f"feature_{i}.npy"), np.ascontiguousarray(m.transpose(2, 0, 1)))
    assert np.array_equal(_lines(optimize.line_refinement(dict(CFG), tracks, ic, patch_dir=pdir, host_threads=2)), _lines(by_p))
    assert np.array_equal(_lines(optimize.line_refinement(dict(CFG), tracks, ic, featuremap_dir=fdir, host_threads=2)), _lines(by_m))


def test_sanitizer_program_of_the_host_twin():
    """tools/refine_feature_host_asan.cpp + lt_refine.cpp (host-only) under AddressSanitizer and UBSan, a program of its own"""
    from helpers import run_host_asan
    run_host_asan("refine_feature_asan", "refine_feature_host_asan")
