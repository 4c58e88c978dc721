"""limap_amd.line2d, host side (no GPU): the restatement lt_fn_sold2_detect_host against what limap's own
LineSegmentDetectionModule made of every fixture of tests/golden/sold2_detect (written by
tests/golden/make_sold2_detect_golden.py), stage by stage: every stage is fed the reference's output of the stage before
it, so that differences do not compound.

Elementwise pieces (sample positions, bilinear and local-max values) must equal the reference bit for bit.  Reductions
(the top-share mean of a refinement block, the mean over the samples) and the point-to-line distance are definitions of
ours: they are compared under derived bounds, and a candidate or a segment whose float64
re-evaluation lies within the derived margin of a threshold is UNDECIDED -- at most 10 % of a fixture's items."""
import importlib.util
import json
import os

import numpy as np
import pytest

from limap_amd import line2d, matching

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gen = _load("make_sold2_detect_golden")
U, F = gen.U, np.float32
EXPECTED = ["bilinear_global_83x101", "edge_border", "edge_j0_plain", "edge_j0_refine", "edge_j1_plain", "edge_j1_refine",
            "edge_j2_plain", "edge_j2_refine", "edge_no_detection", "edge_point", "edge_same_endpoints",
            "plateau_96x128", "radius1_blocks5_80x96", "shipped_96x128"]
BIG = ["bilinear_global_83x101", "radius1_blocks5_80x96", "shipped_96x128"]
REF_TIME = json.load(open(os.path.join(gen.OUT, "ref_time.json")))
_cache = {}


def fixture(name):
    if name not in _cache:
        _cache[name] = gen.load_fixture(name)
    return _cache[name]


def stage_cfg(cfg, **kw):
    c = json.loads(json.dumps(cfg))
    c.update(kw)
    return c


def perturb_vec(cfg):
    j = cfg["junction_refine_cfg"]
    return line2d._perturb_vec(j["num_perturbs"], j["perturb_interval"])


def test_every_fixture_is_there():
    assert gen.fixture_names() == EXPECTED


# ---- sampler, positions, elementwise values ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 5, 64])
def test_sampler_is_torch_linspace(n):
    import torch
    ref = torch.linspace(0, 1, n).numpy()
    assert np.array_equal(line2d.linspace_sampler(n), ref)
    module = line2d.LineSegmentDetectionModule(0.5, num_samples=n)
    assert np.array_equal(module.torch_sampler, ref)


def test_stored_samplers_are_torch_linspace():
    import torch
    for name in EXPECTED:
        s = fixture(name)["sampler"]
        assert np.array_equal(s, torch.linspace(0, 1, len(s)).numpy()), name


@pytest.mark.parametrize("name", BIG + ["plateau_96x128", "edge_border"])
def test_positions_and_sample_values_equal_the_reference_bit_for_bit(name):
    fx = fixture(name)
    cfg, junc, heat, pairs = fx["cfg"], fx["junctions"], fx["ref_refined_heat"], fx["ref_pairs"]
    assert len(pairs) > 0
    H, W = heat.shape
    for method, key in (("local_max", "ref_val_local_max"), ("bilinear", "ref_val_bilinear")):
        c = stage_cfg(cfg, sampling_method=method, use_heatmap_refinement=False, heatmap_refine_cfg=None)
        pos, val = line2d.samples_host(c, junc, heat, pairs)
        assert np.array_equal(pos.view(np.uint32), fx["ref_pos"].view(np.uint32))
        assert np.array_equal(val, fx[key]), f"{method}: {np.abs(val - fx[key]).max()}"
    # the NumPy restatement the analysis below rests on gives the same bits
    js, je = junc[pairs[:, 0]], junc[pairs[:, 1]]
    h = gen.sample_positions(js[:, 0], je[:, 0], fx["sampler"], H - 1)
    w = gen.sample_positions(js[:, 1], je[:, 1], fx["sampler"], W - 1)
    assert np.array_equal(h, fx["ref_pos"][..., 0]) and np.array_equal(w, fx["ref_pos"][..., 1])
    assert np.array_equal(gen.bilinear_values(heat, h, w), fx["ref_val_bilinear"])
    lm = gen.local_max_values(heat, h, w, int(cfg.get("max_local_patch_radius", 3)),
                              gen.dist_thresholds(js, je, H, W, cfg.get("lambda_radius", 2.0)))
    assert np.array_equal(lm, fx["ref_val_local_max"])


# ---- refined heatmap ------------------------------------------------------------------------------------------------------
REFINED = [n for n in EXPECTED if n not in ("edge_same_endpoints", "edge_point")]


@pytest.mark.parametrize("name", REFINED)
def test_block_scales_and_refined_pixels_within_the_derived_bound(name):
    """ours: the exact sum of the k largest values, divided in FP64, rounded once (relative error u).  torch: an FP32 sum
    of k positive values in some order (relative error below (k - 1) u / (1 - (k - 1) u)) and an FP32 division (u).  So
    the two scales differ relatively by less than (k + 3) u.  A pixel is the clamped mean of at most four clamped
    quotients h / scale <= 1: a quotient moves by its scale's relative difference and the two division roundings, the
    sum of c <= 4 terms by 2 (c - 1) u c and the division by the count by 2 u more: (k_max + 16) u in all."""
    fx = fixture(name)
    cfg, heat = fx["cfg"], fx["heatmap"]
    scales, bounds = line2d.block_scales_host(cfg, heat)
    assert np.array_equal(bounds, fx["ref_bounds"])
    ref, k = fx["ref_scales"], fx["ref_scale_counts"]
    assert np.array_equal(scales < 0, ref < 0)
    on = ref > 0
    assert (np.abs(scales - ref)[on] <= (k[on] + 3) * U * ref[on]).all()
    _, st = line2d.detect_scene(stage_cfg(cfg, use_junction_refinement=False, junction_refine_cfg=None),
                                [fx["junctions"]], [heat], host=True, return_stages=True)
    kmax = np.zeros(heat.shape)
    for a in range(len(bounds)):
        for b in range(len(bounds)):
            sl = (slice(bounds[a, 0], bounds[a, 1]), slice(bounds[b, 2], bounds[b, 3]))
            kmax[sl] = np.maximum(kmax[sl], k[a, b])
    diff = np.abs(st[0]["heatmap"].astype(np.float64) - fx["ref_refined_heat"])
    assert (diff <= (kmax + 16) * U).all(), diff.max()
    rec = REF_TIME["fixtures"][name]["max_rel_scale_difference"]
    assert rec <= (k.max() + 3) * U


def test_refined_pixels_equal_torch_given_equal_scales():
    """the per-pixel pass is elementwise: on a heatmap whose block scales come out the same bits on both sides (a
    block's top share is a single value, so no sum is rounded) the refined heatmap equals the reference's exactly"""
    fx = fixture("edge_no_detection")
    _, st = line2d.detect_scene(fx["cfg"], [fx["junctions"]], [fx["heatmap"]], host=True, return_stages=True)
    assert np.array_equal(st[0]["heatmap"], fx["ref_refined_heat"])
    import torch
    rng = np.random.default_rng(3)
    heat = rng.random((41, 37)).astype(F)
    cfg = stage_cfg(gen.SHIPPED, heatmap_refine_cfg={"mode": "local", "ratio": 1e-6, "valid_thresh": 0.3, "num_blocks": 4,
                                                     "overlap_ratio": 0.5},
                    use_junction_refinement=False, junction_refine_cfg=None)
    scales, bounds = line2d.block_scales_host(cfg, heat)
    out = torch.zeros(heat.shape)
    cnt = torch.zeros(heat.shape, dtype=torch.int)
    ht = torch.tensor(heat)
    for a in range(4):
        for b in range(4):
            sl = (slice(bounds[a, 0], bounds[a, 1]), slice(bounds[b, 2], bounds[b, 3]))
            assert scales[a, b] == heat[sl].max()
            out[sl] += torch.clamp(ht[sl] / float(scales[a, b]), min=0.0, max=1.0)
            cnt[sl] += 1
    want = torch.clamp(out / cnt, max=1.0, min=0.0).numpy()
    _, st = line2d.detect_scene(cfg, [np.zeros((0, 2), F)], [heat], host=True, return_stages=True)
    assert np.array_equal(st[0]["heatmap"], want)


# ---- candidate mask and line map ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BIG + ["plateau_96x128", "edge_border", "edge_no_detection"])
def test_candidate_mask_equals_the_reference_where_decided(name):
    fx = fixture(name)
    cfg, junc = fx["cfg"], fx["junctions"]
    c = stage_cfg(cfg, use_heatmap_refinement=False, heatmap_refine_cfg=None, use_junction_refinement=False,
                  junction_refine_cfg=None)
    _, st = line2d.detect_scene(c, [junc], [fx["ref_refined_heat"]], host=True, return_stages=True)
    ours, ref = st[0]["candidates"], fx["ref_cand"]
    keep, decided = gen.suppression_analysis(junc, cfg["nms_dist_tolerance"])
    iu = np.triu_indices(len(junc), 1)
    assert (~decided[iu]).mean() <= gen.MAX_UNDECIDED
    assert (~decided[iu]).mean() == pytest.approx(REF_TIME["fixtures"][name]["undecided_share"]["suppression"])
    d = decided[iu]
    assert np.array_equal(ours[iu][d], ref[iu][d])
    assert np.array_equal(ours[iu][d] != 0, keep[iu][d])
    assert not np.tril(ours).any()


@pytest.mark.parametrize("name", BIG + ["plateau_96x128", "edge_border", "edge_same_endpoints", "edge_point"])
def test_line_map_equals_the_reference_where_decided(name):
    fx = fixture(name)
    cfg, junc, heat = fx["cfg"], fx["junctions"], fx["ref_refined_heat"]
    c = stage_cfg(cfg, use_heatmap_refinement=False, heatmap_refine_cfg=None, use_junction_refinement=False,
                  junction_refine_cfg=None)
    segs, st = line2d.detect_scene(c, [junc], [heat], host=True, return_stages=True, cand_in=[fx["ref_cand"]])
    pairs = fx["ref_pairs"]
    ok, decided, *_ = gen.scoring_analysis(heat, junc, pairs, cfg, fx["sampler"])
    assert (~decided).mean() <= gen.MAX_UNDECIDED
    ours, ref = st[0]["line_map"], fx["ref_line_map"]
    assert np.array_equal(ours, ours.T) and ours.dtype == np.int32
    p = pairs[decided]
    assert np.array_equal(ours[p[:, 0], p[:, 1]], ref[p[:, 0], p[:, 1]])
    assert np.array_equal(ours[p[:, 0], p[:, 1]] != 0, ok[decided])
    off = np.ones_like(ours, bool)
    off[pairs[:, 0], pairs[:, 1]] = off[pairs[:, 1], pairs[:, 0]] = False
    assert not ours[off].any()
    # without junction refinement the segments are the detected pairs in candidate order
    det = np.argwhere(np.triu(ours, 1))
    assert np.array_equal(segs[0], np.stack([junc[det[:, 0]], junc[det[:, 1]]], 1).astype(np.float64).reshape(-1, 2, 2))


# ---- junction refinement ----------------------------------------------------------------------------------------------------
WITH_REFINEMENT = [n for n in EXPECTED if not n.endswith(("_refine", "_plain")) and n != "edge_no_detection"]


@pytest.mark.parametrize("name", WITH_REFINEMENT + ["edge_j2_refine"])
def test_junction_refinement_against_the_reference(name):
    fx = fixture(name)
    cfg, junc, heat = fx["cfg"], fx["junctions"], fx["ref_refined_heat"]
    c = stage_cfg(cfg, use_heatmap_refinement=False, heatmap_refine_cfg=None)
    segs, st = line2d.detect_scene(c, [junc], [heat], host=True, return_stages=True, det_in=[fx["ref_line_map"]])
    det = np.argwhere(np.triu(fx["ref_line_map"], 1))
    assert np.array_equal(st[0]["pairs"], det)
    ours, ref = st[0]["perturb"], fx["ref_perturb"]
    assert len(ours) == len(ref) == len(det) > 0
    vec = perturb_vec(cfg)
    start = np.concatenate([junc[det[:, 0]], junc[det[:, 1]]], 1)
    ana = gen.refinement_analysis(heat, start, vec, fx["sampler"])
    decided = np.array([a[1] for a in ana])
    plateau = "flag_plateau" in fx
    if not plateau:
        assert (~decided).mean() <= gen.MAX_UNDECIDED
        assert np.array_equal(ours[decided], ref[decided])
        assert np.array_equal(ours[decided], np.array([a[0] for a in ana])[decided])
    for s, (best, _, margin, obj) in enumerate(ana):
        # every evaluation is within margin / 2 of the float64 objective, so the arg-max of any of them is within
        # margin of the best
        assert obj[ours[s]] >= obj[ref[s]] - margin
        assert obj[ours[s]] >= obj[best] - margin
        H, W = heat.shape
        assert np.array_equal(st[0]["segments_refined"][s].reshape(4), gen.perturbed_segments(start[s], vec, H, W)[ours[s]])
    if not plateau and decided.all():
        assert np.array_equal(st[0]["junctions_refined"], fx["ref_junctions_out"])
        assert np.array_equal(st[0]["line_map_refined"], fx["ref_line_map_out"])
        assert np.array_equal(segs[0], fx["ref_segments"])


# ---- the whole chain --------------------------------------------------------------------------------------------------------
def _no_undecided(name):
    return max(REF_TIME["fixtures"][name]["undecided_share"].values()) == 0.0


def test_the_generator_verified_the_whole_chain_fixture():
    assert "flag_whole_chain" in fixture("shipped_96x128") and _no_undecided("shipped_96x128")
    assert fixture("shipped_96x128")["cfg"] == line2d.SHIPPED_CFG
    assert len(fixture("shipped_96x128")["ref_segments"]) >= 8


@pytest.mark.parametrize("name", [n for n in EXPECTED if n == "shipped_96x128" or n.startswith("edge_")])
def test_whole_chain_equals_the_reference_exactly(name):
    assert _no_undecided(name)
    fx = fixture(name)
    segs = line2d.detect_scene(fx["cfg"], [fx["junctions"]], [fx["heatmap"]], host=True)
    assert segs[0].dtype == np.float64 and segs[0].shape == fx["ref_segments"].shape
    assert np.array_equal(segs[0], fx["ref_segments"])
    module = line2d.LineSegmentDetectionModule(**fx["cfg"])
    line_map, junctions, heat = module.detect(fx["junctions"], fx["heatmap"], host=True)
    assert np.array_equal(junctions, fx["ref_junctions_out"])
    assert np.array_equal(line_map, fx["ref_line_map_out"])
    assert np.array_equal(line2d.line_map_to_segments(junctions, line_map), fx["ref_segments"])


def test_edge_fixtures_hold_what_they_are_named_for():
    for n in (0, 1, 2):
        assert len(fixture(f"edge_j{n}_refine")["junctions"]) == n
        # with junction refinement on and no detected segment the result has zero junctions
        if n < 2:
            assert fixture(f"edge_j{n}_refine")["ref_junctions_out"].shape == (0, 2)
            assert fixture(f"edge_j{n}_plain")["ref_junctions_out"].shape == (n, 2)
    assert len(fixture("edge_j2_refine")["ref_segments"]) == 1
    assert len(fixture("edge_no_detection")["ref_segments"]) == 0
    assert fixture("edge_no_detection")["ref_junctions_out"].shape == (0, 2)
    assert (fixture("edge_no_detection")["ref_scales"] < 0).all()
    j = fixture("edge_border")["junctions"]
    assert {0.0, 31.0} <= set(j[:, 0]) and {0.0, 39.0} <= set(j[:, 1]) and len(fixture("edge_border")["ref_segments"]) == 4
    same = fixture("edge_same_endpoints")
    assert len(same["ref_perturb"]) > len(same["ref_segments"])  # two detections refined to the same end points
    pt = fixture("edge_point")["ref_segments"]
    assert len(pt) == 1 and np.array_equal(pt[0, 0], pt[0, 1])


def test_coordinate_flips():
    s = np.arange(24, dtype=np.float64).reshape(6, 2, 2)
    flat = line2d.sold2segstosegs(s)
    assert flat.shape == (6, 4) and np.array_equal(flat[:, 0], s[:, 0, 1]) and np.array_equal(flat[:, 3], s[:, 1, 0])
    assert np.array_equal(line2d.segstosold2segs(flat), s)


# ---- compute_descinfo ---------------------------------------------------------------------------------------------------------
def _desc_truth(segs, desc, valid_pts, grid=4):
    """float64 evaluation of grid_sample + normalize and the magnitudes its bound needs"""
    _, C, Hd, Wd = desc.shape
    p = valid_pts.reshape(-1, 2).astype(F)
    coords = []
    for col, size in ((0, Hd), (1, Wd)):
        g = p[:, col] * F(2) / F(size * grid) - F(1)
        coords.append(((g + F(1)) * F(size) - F(1)) / F(2))
    iy, ix = (c.astype(np.float64) for c in coords)
    y0, x0 = np.floor(iy), np.floor(ix)
    val = np.zeros((C, len(p)))
    mag = np.zeros((C, len(p)))
    d64 = desc[0].astype(np.float64)
    for dy in (0, 1):
        for dx in (0, 1):
            wy = (iy - y0) if dy else (y0 + 1 - iy)
            wx = (ix - x0) if dx else (x0 + 1 - ix)
            yy, xx = (y0 + dy).astype(int), (x0 + dx).astype(int)
            inside = (yy >= 0) & (yy < Hd) & (xx >= 0) & (xx < Wd)
            tap = np.where(inside, d64[:, np.clip(yy, 0, Hd - 1), np.clip(xx, 0, Wd - 1)], 0.0)
            val += tap * (wy * wx)
            mag += np.abs(tap) * (wy * wx)
    norm = np.maximum(np.sqrt((val * val).sum(0)), 1e-12)
    return val / norm, mag / norm


@pytest.mark.parametrize("name", ["descinfo_a", "descinfo_b", "descinfo_small"])
def test_descinfo_against_the_reference(name):
    """a sampled value is a 4-term sum of products with weights that are themselves products: below 6 u sum |w v| from
    the truth in any order; the norm of C such values adds (C / 2 + 2) u relatively, the division u"""
    z = np.load(os.path.join(gen.OUT, name + ".npz"))
    segs, desc = z["segs"], z["descriptor"]
    pts, valid = line2d.sample_line_points(segs)
    assert np.array_equal(valid, z["ref_valid"]) and np.array_equal(pts, z["ref_points"])
    d, v = line2d.compute_descinfo(segs, desc, host=True)
    assert d.dtype == np.float32 and d.shape == z["ref_desc"].shape and np.array_equal(v, valid)
    truth, mag = _desc_truth(segs, desc, pts)
    C = desc.shape[1]
    bound = 6 * U * mag * (1 + (C + 6) * U) + np.abs(truth) * (C / 2 + 6) * U + 6 * U * np.sqrt((mag * mag).sum(0)) * np.abs(truth)
    assert (np.abs(d - truth) <= bound).all()
    assert (np.abs(z["ref_desc"] - truth) <= bound).all()


def test_descinfo_matches_like_the_reference_descinfo():
    wgen = _load("make_match_wunsch_golden")
    za, zb = (np.load(os.path.join(gen.OUT, n + ".npz")) for n in ("descinfo_a", "descinfo_b"))
    ref = [[z["ref_desc"], z["ref_valid"]] for z in (za, zb)]
    assert wgen.undecided_share(ref, [(0, 1), (1, 0)], 0, 5, 10) == 0.0
    ours = [line2d.compute_descinfo(z["segs"], z["descriptor"], host=True) for z in (za, zb)]
    for a, b in ((0, 1), (1, 0)):
        want = matching.match_pair_host(ref[a], ref[b], "sold2", topk=0)
        got = matching.match_pair_host(ours[a], ours[b], "sold2", topk=0)
        assert len(want) >= 10 and np.array_equal(got, want)


def test_descinfo_of_no_segments_and_other_modes():
    d = line2d.compute_descinfo(np.zeros((0, 2, 2)), np.zeros((1, 8, 5, 5), F), host=True)
    assert isinstance(d, np.ndarray) and d.shape == (0,) and d.dtype == np.empty((0), dtype=int).dtype
    for mode in ("d2_net", "asl_feat"):
        with pytest.raises(NotImplementedError):
            line2d.compute_descinfo(np.zeros((1, 2, 2)), np.zeros((1, 8, 5, 5), F), sampling_mode=mode, host=True)


# ---- rejections -------------------------------------------------------------------------------------------------------------------
def test_rejections_name_the_key():
    M = line2d.LineSegmentDetectionModule
    with pytest.raises(ValueError, match="Missing heatmap refinement config"):
        M(0.5, use_heatmap_refinement=True)
    with pytest.raises(ValueError, match="Missing junction refinement config"):
        M(0.5, use_junction_refinement=True)
    for bad in (1, 65):
        with pytest.raises(ValueError, match="num_samples"):
            M(0.5, num_samples=bad)
    for bad in (4, 11):
        with pytest.raises(ValueError, match="num_perturbs"):
            M(0.5, use_junction_refinement=True, junction_refine_cfg={"num_perturbs": bad, "perturb_interval": 0.25})
    with pytest.raises(ValueError, match="max_local_patch_radius"):
        M(0.5, max_local_patch_radius=5)
    with pytest.raises(ValueError, match="sampling_method"):
        M(0.5, sampling_method="nearest")
    with pytest.raises(ValueError, match="mode"):
        M(0.5, use_heatmap_refinement=True, heatmap_refine_cfg={"mode": "median", "ratio": 0.2, "valid_thresh": 0.01})
    m = M(0.5)
    heat = np.zeros((20, 20), F)
    with pytest.raises(ValueError, match=r"junctions must be \(n, 2\)"):
        m.detect(np.zeros((4, 3), F), heat, host=True)
    with pytest.raises(ValueError, match="2-D"):
        m.detect(np.zeros((4, 2), F), np.zeros((20, 20, 1), F), host=True)
    with pytest.raises(ValueError, match="num_blocks"):
        line2d.detect_scene(stage_cfg(gen.SHIPPED, heatmap_refine_cfg={"mode": "local", "ratio": 0.2, "valid_thresh": 0.01,
                                                                       "num_blocks": 33, "overlap_ratio": 0.5}),
                            [np.zeros((0, 2), F)], [heat], host=True)
    # the library rejects what the Python layer lets through when its attributes are changed after construction
    m.num_samples = 70
    with pytest.raises(ValueError, match="num_samples"):
        m.detect(np.zeros((4, 2), F), heat, host=True)
