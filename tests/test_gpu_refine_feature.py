"""-m gpu: the line refinement with the feature-consistency term on the device (k_refine_lm_feat) equals the host twin
(lt_fn_refine_host_feature) bit for bit -- parameters, segments, both costs, iterations, termination codes -- for every
combination with the other terms, both forms and texel types, at the edges of the tracks-per-workgroup count, for device
inputs, the edge scenes of tests/test_refine_feature_host.py and the maps as context state."""
import glob
import itertools
import os

import numpy as np
import pytest

import refine_feature_scenes as fs
from limap_amd import features, optimize
from test_refine_feature_host import GOLDEN, load_golden, run_golden

pytestmark = pytest.mark.gpu

TRACKS_PER_WORKGROUP = 4  # kRfFeatTracks of lt_refine.h


@pytest.fixture(scope="module")
def scene(gpu_lib):
    return fs.make_scene(counts=(5, 4, 6, 4, 5), seed=2)


@pytest.fixture(scope="module")
def sources(scene):
    out = {}
    for dt in ("float16", "float32"):
        out[("patch", dt)] = fs.patches_of(scene, dt)
        out[("map", dt)] = fs.texel_maps(scene, dt)
    return out


def both(s, rf, form, src, **kw):
    h = fs.run(s, rf, form, src, host_threads=8, **kw)
    d = fs.run(s, rf, form, src, **kw)
    fs.same_bits(h, d, (form, kw.get("tracks")))
    return h, d


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "*.npz"))))
def test_device_reproduces_the_goldens(gpu_lib, path):
    """against the recorded bytes, not against the twin"""
    z, maps, want = load_golden(path)
    d = run_golden(z, maps)
    for k in fs.RESULT_KEYS:
        x, y = np.ascontiguousarray(d[k]), np.ascontiguousarray(want[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), (os.path.basename(path), k)


@pytest.mark.parametrize("geo,vp,hm", list(itertools.product([1, 0], [0, 1], [0, 1])))
def test_every_term_combination_both_forms_and_texel_types(scene, sources, geo, vp, hm):
    moved = 0
    for dt in ("float16", "float32"):
        rf = fs.refine_cfg(use_geometric=bool(geo), use_vp=bool(vp), use_heatmap=bool(hm), dtype=dt, vp_multiplier=0.1,
                           n_samples_heatmap=5)
        heat = optimize.Heatmaps(fs.some_heatmaps(scene), dt) if hm else None
        for form in ("patch", "map"):
            h, _ = both(scene, rf, form, sources[(form, dt)], vp=fs.some_vps(scene) if vp else None, heatmaps=heat)
            moved += int((h["iterations"] > 0).sum())
    assert moved > 0


def test_track_counts_order_and_repetition(scene, sources):
    rf = fs.refine_cfg()
    n = TRACKS_PER_WORKGROUP
    assert len(scene["line6"]) == n + 1
    src = sources[("patch", "float16")]
    full, _ = both(scene, rf, "patch", src)
    for cnt in (1, n - 1, n, n + 1):
        h, d = both(scene, rf, "patch", src, tracks=list(range(cnt)))
        assert np.array_equal(d["params"], full["params"][:cnt]), "a track does not see its neighbours"
    perm = [3, 0, 4, 2, 1]
    _, d = both(scene, rf, "patch", src, tracks=perm)
    assert np.array_equal(d["params"], full["params"][perm])
    fs.same_bits(fs.run(scene, rf, "patch", src), fs.run(scene, rf, "patch", src), "two runs in a row")
    _, dm = both(scene, rf, "map", sources[("map", "float16")], tracks=perm)
    assert dm["params"].shape == (n + 1, 6)


CFG = dict(min_num_images=4, use_geometric=True, use_feature=True, n_samples_feature=8, dtype="float16")


def _lines(tracks):
    return np.array([np.concatenate([t.line.start, t.line.end]) for t in tracks])


def test_one_track_per_native_call_and_device_inputs(scene, sources):
    import torch
    tracks, ic = fs.tracks_of(scene), fs.imagecols(scene)
    pat, maps = sources[("patch", "float16")], sources[("map", "float16")]
    host = optimize.line_refinement(dict(CFG), tracks, ic, patches=pat, host_threads=8)
    dev = optimize.line_refinement(dict(CFG), tracks, ic, patches=pat)
    one = optimize.line_refinement(dict(CFG), tracks, ic, patches=pat, patch_bytes=1)
    assert np.array_equal(_lines(host), _lines(dev)) and np.array_equal(_lines(one), _lines(dev))
    on_dev = features.extract_track_patches(dict(fs.PATCH_CFG), tracks, ic, scene["maps"], dtype="float16", device_out=True)
    assert all(p.array.is_cuda for p in on_dev.values())
    assert all(np.array_equal(on_dev[k].array.cpu().numpy(), np.asarray(pat[k].array)) for k in pat), "the same patches"
    left = optimize.line_refinement(dict(CFG), tracks, ic, patches=on_dev)
    assert np.array_equal(_lines(left), _lines(dev)), "patches left on the device"
    hm = optimize.line_refinement(dict(CFG), tracks, ic, featuremaps=maps, host_threads=8)
    tens = {i: torch.from_numpy(m).cuda() for i, m in maps.items()}
    assert np.array_equal(_lines(optimize.line_refinement(dict(CFG), tracks, ic, featuremaps=tens)), _lines(hm)), "GPU tensors"
    assert np.array_equal(_lines(optimize.line_refinement(dict(CFG), tracks, ic, featuremaps=maps)), _lines(hm)), "host arrays"


def test_edge_scenes_and_a_mixed_call(scene, sources):
    """the edge scenes of the host test, and tracks with and without kept samples in one call"""
    maps = sources[("map", "float16")]
    rf = fs.refine_cfg()
    exact = fs.projected_supports(scene, 0)
    K = len(exact["img"])
    none_kept = fs.shifted(exact, 0.3 + 1e-9)
    tie = fs.length_tie(exact, 0, 1)
    assert tie is not None
    edges = [fs.shifted(exact, 0.3 - 1e-9), none_kept, fs.trimmed(exact, [(0.0, 0.5)] + [(0.6, 1.0)] * (K - 1)),
             fs.trimmed(tie, [(0, 1), (0, 1)] + [(0.1, 0.8)] * (K - 2))]
    for o in edges:
        both(o, rf, "map", maps)
    mixed = fs.merge(fs.subset(scene, [1]), none_kept, fs.subset(scene, [2]), edges[2])
    h, d = both(mixed, rf, "map", maps)
    alone = fs.run(none_kept, fs.refine_cfg(use_feature=False), None, None)
    assert np.array_equal(d["params"][1], alone["params"][0]), "no kept sample: the run without the term"
    cut = {i: np.ascontiguousarray(m[:20, :30]) for i, m in maps.items()}
    both(scene, rf, "map", cut)
    small = features.extract_track_patches(dict(fs.PATCH_CFG, patch=dict(k_stretch=1.0, t_stretch=0, range_perp=1)),
                                           fs.tracks_of(scene), fs.imagecols(scene), scene["maps"], host=True, dtype="float16")
    both(scene, rf, "patch", small)
    f = fs.failing_scene()
    h, d = both(f, rf, "map", {i: m.astype(np.float16) for i, m in f["maps"].items()})
    assert d["codes"][0] == 6 and d["iterations"][0] == 0


def test_feature_maps_and_heatmaps_do_not_disturb_each_other(scene, sources):
    maps = optimize.FeatureMaps(sources[("map", "float16")], "float16")
    heat = optimize.Heatmaps(fs.some_heatmaps(scene), "float16")
    rf_f = fs.refine_cfg()
    rf_h = fs.refine_cfg(use_feature=False, use_heatmap=True, n_samples_heatmap=5)
    want_f = fs.run(scene, rf_f, "map", sources[("map", "float16")], host_threads=8)
    want_h = fs.run(scene, rf_h, None, None, host_threads=8, heatmaps=heat)
    for _ in range(2):
        fs.same_bits(fs.run(scene, rf_f, "map", maps), want_f, "the feature term after a heatmap run")
        fs.same_bits(fs.run(scene, rf_h, None, None, heatmaps=heat), want_h, "the heatmap term after a feature run")
