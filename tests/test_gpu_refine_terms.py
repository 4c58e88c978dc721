"""-m gpu: the line refinement with the VP and the heatmap term on the device (k_refine_prep_terms, k_refine_lm_terms)
equals the host path (lt_fn_refine_host_terms) bit for bit -- parameters, segments, costs, iterations, termination codes --
at the group width's edges, for every term combination, both texel types and the branch fixtures of
tests/test_refine_terms_host.py; the goldens; the call without a term; determinism; the heatmaps as context state
(DESIGN.md section 19)."""
import glob
import os

import numpy as np
import pytest

import refine_scenes as rs
import refine_terms_scenes as ts
from limap_amd import _capi
from test_refine_terms_host import CFG, COUNTS, GOLDEN, KEYS, VP_CFG, _imagecols, _linetracks, load_golden, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    return _capi.Context()


@pytest.fixture(scope="module")
def scene():
    """tracks of 1, 4, 5, 15, 16, 17 and 33 supports in images of 17x23 and 24x32, two images without a track, and the
    track whose evaluation fails at the start"""
    return ts.merge(ts.make_scene(COUNTS, seed=1), ts.failing_track())


def set_heatmaps(ctx, tex, texel_type=_capi.TEXEL_F16):
    return ctx.L.lt_refine_set_heatmaps(ctx.h, *ts.heatmap_args(tex), texel_type)


def both(ctx, s, cfg_kw, terms_kw, dtype=np.float16):
    """(host, device) results of one configuration"""
    L = ctx.L
    ttype = _capi.TEXEL_F32 if dtype == np.float32 else _capi.TEXEL_F16
    tex = ts.texels(s, dtype)
    cfg, terms = ts.cfg_struct(L, **cfg_kw), ts.terms_struct(L, texel_type=ttype, **terms_kw)
    rc, h = ts.run_host(L, s, cfg, terms, tex, threads=8)
    assert rc == 0, L.lt_fn_refine_host_error()
    assert set_heatmaps(ctx, tex, ttype) == 0
    rc, d = ts.run_device(ctx, s, cfg, terms)
    assert rc == 0, L.lt_last_error(ctx.h)
    return h, d


TERMS = {
    "vp": dict(use_vp=1),
    "vp_alone": dict(use_geometric=0, use_vp=1, vp_multiplier=0.1),
    "heatmap": dict(use_heatmap=1),
    "heatmap_alone_2": dict(use_geometric=0, use_heatmap=1, n_samples_heatmap=2),
    "all_10": dict(use_vp=1, use_heatmap=1),
    "all_11": dict(use_vp=1, use_heatmap=1, n_samples_heatmap=11, heatmap_multiplier=0.5),
    "no_geometric": dict(use_geometric=0, use_vp=1, use_heatmap=1),
}


@pytest.mark.parametrize("name,dtype", [(n, t) for n in sorted(TERMS) for t in (np.float16, np.float32)
                                        if t == np.float16 or TERMS[n].get("use_heatmap")])
def test_device_equals_host_bit_for_bit(ctx, scene, name, dtype):
    h, d = both(ctx, scene, dict(num_outliers_aggregator=0), TERMS[name], dtype)
    same(h, d, name)
    if TERMS[name].get("use_heatmap"):
        assert h["codes"][-1] == 6 and np.array_equal(h["params"][-1], d["params"][-1])
    assert np.any(h["iterations"] > 0)


@pytest.mark.parametrize("tracks", [[3], [1, 2, 4, 6], [0, 1, 2, 3, 5]], ids=["one_group", "one_wave", "one_over"])
def test_track_counts_around_a_wave(ctx, scene, tracks):
    h, d = both(ctx, ts.subset(scene, tracks), dict(num_outliers_aggregator=0, min_num_images=1), TERMS["all_10"])
    same(h, d, tracks)


@pytest.mark.parametrize("fixture,terms", [("long_supports", "all_11"), ("checker_heatmaps", "heatmap_alone_2"),
                                           ("perpendicular_vps", "vp_alone")])
def test_branch_fixtures(ctx, fixture, terms):
    s = getattr(ts, fixture)(ts.make_scene(COUNTS, seed=1))
    h, d = both(ctx, s, dict(num_outliers_aggregator=0, min_num_images=1), TERMS[terms])
    same(h, d, fixture)


@pytest.mark.parametrize("terms", ["vp", "all_10"])
def test_tracks_without_a_labelled_support(ctx, terms):
    """use_vp on and no label anywhere: k_refine_lm_terms gives the host's bits, which are those of the call without
    use_vp (for the geometric term alone that call is k_refine_lm)"""
    s = ts.make_scene(COUNTS, seed=1)
    s["vp_flag"] = np.zeros_like(s["vp_flag"])
    cfg = dict(num_outliers_aggregator=0, min_num_images=1)
    h, d = both(ctx, s, cfg, TERMS[terms])
    same(h, d, terms)
    _, d0 = both(ctx, s, cfg, dict(TERMS[terms], use_vp=0))
    same(d, d0, "without use_vp")


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "*.npz"))))
def test_device_reproduces_the_goldens(ctx, path):
    s, tex, cfg, terms, want = load_golden(path)
    t = ts.terms_struct(ctx.L, **terms)
    assert set_heatmaps(ctx, tex, t.texel_type) == 0
    rc, d = ts.run_device(ctx, s, ts.cfg_struct(ctx.L, **cfg), t)
    assert rc == 0, ctx.L.lt_last_error(ctx.h)
    same(d, want, os.path.basename(path))


def test_no_term_is_lt_refine_arrays(ctx):
    from limap_amd import optimize
    s = rs.make_tracks(40, seed=7)
    cfg = ts.cfg_struct(ctx.L, max_num_iterations=200)
    old = optimize.refine_arrays((s["img_ids"], s["k"], s["q"], s["t"]), (s["line6"], s["off"], s["img"], s["l2d"], s["l3d"]), cfg,
                                 ctx=ctx)
    rc, new = ts.run_device(ctx, s, cfg, ts.terms_struct(ctx.L))
    assert rc == 0
    same(old, new, "no term")


def test_two_runs_and_a_permuted_track_order(ctx, scene):
    cfg, terms = dict(num_outliers_aggregator=0), TERMS["all_10"]
    _, a = both(ctx, scene, cfg, terms)
    _, b = both(ctx, scene, cfg, terms)
    same(a, b, "second run")
    perm = np.random.default_rng(0).permutation(len(scene["line6"]))
    _, c = both(ctx, ts.subset(scene, perm), cfg, terms)
    same({k: a[k][perm] for k in KEYS}, c, "permuted")


def test_heatmaps_are_context_state(ctx, scene):
    L = ctx.L
    tex = ts.texels(scene)
    cfg, terms = ts.cfg_struct(L, num_outliers_aggregator=0), ts.terms_struct(L, use_heatmap=1)
    assert set_heatmaps(ctx, tex) == 0
    rc, a = ts.run_device(ctx, scene, cfg, terms)
    part = ts.subset(scene, [2, 5])
    rc2, b = ts.run_device(ctx, part, cfg, terms)  # the same heatmaps serve a second call
    assert rc == 0 and rc2 == 0
    same({k: a[k][[2, 5]] for k in KEYS}, b, "second call")
    assert ts.run_device(ctx, scene, cfg, ts.terms_struct(L, use_heatmap=1, texel_type=_capi.TEXEL_F32))[0] == -2
    assert L.lt_refine_clear_heatmaps(ctx.h) == 0
    assert ts.run_device(ctx, scene, cfg, terms)[0] == -2
    assert ts.run_device(ctx, scene, cfg, ts.terms_struct(L, use_vp=1))[0] == 0  # the VP term needs none


def test_runner_sequence_on_the_device(gpu_lib, tmp_path):
    from limap_amd import optimize, vplib
    s = ts.make_scene([8, 8, 8, 3] + [8] * 21, seed=21, direction=(0.6, -0.3, 0.74), sizes=((48, 64), (60, 80)))
    tracks, imagecols = _linetracks(s), _imagecols(s)
    all_lines = {int(i): [] for i in s["img_ids"]}
    for t in tracks:
        for k, i in enumerate(t.image_id_list):
            t.line_id_list[k] = len(all_lines[i])
            all_lines[i].append(t.line2d_list[k])
    vpresults = vplib.get_vp_detector(VP_CFG).detect_vp_all_images(all_lines, {i: imagecols.camview(i) for i in all_lines})
    for i, a in s["heatmaps"].items():
        np.save(os.path.join(tmp_path, f"heatmap_{i}.npy"), a)
    dev = optimize.line_refinement(dict(CFG), tracks, imagecols, heatmap_dir=str(tmp_path), vpresults=vpresults)
    host = optimize.line_refinement(dict(CFG), tracks, imagecols, heatmap_dir=str(tmp_path), vpresults=vpresults, host_threads=4)
    for a, b in zip(dev, host):
        assert np.array_equal(a.line.start, b.line.start) and np.array_equal(a.line.end, b.line.end)
    t = tracks[0]
    ids = t.GetSortedImageIds()
    e = optimize.solve_line_refinement(dict(CFG), t, [imagecols.camview(i) for i in ids], p_vpresults=[vpresults[i] for i in ids],
                                       p_heatmaps=[s["heatmaps"][i] for i in ids])
    assert np.array_equal(e.GetLine3d().start, dev[0].line.start)


def test_python_heatmap_cache_follows_the_context(ctx):
    """optimize.Heatmaps uploads once per context and again after anyone changed the context's heatmaps"""
    from limap_amd import optimize
    L = ctx.L
    s = ts.make_scene([5, 6], seed=22)
    hm = optimize.Heatmaps(s["heatmaps"], "float16")
    cams = (s["img_ids"], s["k"], s["q"], s["t"])
    csr = (s["line6"], s["off"], s["img"], s["l2d"], s["l3d"])
    cfg, terms = ts.cfg_struct(L), ts.terms_struct(L, use_heatmap=1)

    def run():
        return optimize.refine_arrays(cams, csr, cfg, ctx=ctx, terms=terms, heatmaps=hm)
    a = run()
    gen = L.lt_refine_heatmaps_generation(ctx.h)
    b = run()
    assert L.lt_refine_heatmaps_generation(ctx.h) == gen, "the second call uploaded again"
    assert L.lt_refine_clear_heatmaps(ctx.h) == 0  # behind Python's back
    c = run()
    assert L.lt_refine_heatmaps_generation(ctx.h) > gen + 1
    for r in (b, c):
        same(a, r, "cache")
