"""limap_amd.line2d on the device: every kernel of lt_kernels_sold2.hip against the library's host restatement with
zero tolerance -- segments, every returned stage, the chosen perturbation indexes, the refined-heatmap bits and the
descinfo bits -- at the edges of the tiling: junction counts around one wave of lanes and several passes of the LDS
junction table, heatmaps that are no multiple of anything, refinement blocks down to 8 x 9 pixels and one below
valid_thresh, every sample count / patch radius / perturbation count the kernels branch on, both heatmap paths of the
junction refinement, a plateau (the lowest-index tie rule), a ragged batch, torch GPU tensors, and the way into
matching.SOLD2Matcher.  Synthetic scenes only."""
import importlib.util
import json
import os

import numpy as np
import pytest

from limap_amd import line2d, matching

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_sold2_detect_golden",
                                               os.path.join(HERE, "golden", "make_sold2_detect_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)
F = np.float32
_scenes = {}


def scene(seed, H, W, n_lines, n_junc, profile="gauss"):
    """junctions (exactly n_junc of them: the line ends first) and a heatmap; computed once per key"""
    key = (seed, H, W, n_lines, n_junc, profile)
    if key not in _scenes:
        rng = np.random.default_rng(seed)
        if n_lines:
            ends, heat = gen.random_scene(rng, H, W, n_lines, 0, profile)
        else:
            ends, heat = np.zeros((0, 2), F), (rng.random((H, W)) * 0.03).astype(F)
        extra = np.stack([rng.integers(0, H, 2 * n_junc + 8), rng.integers(0, W, 2 * n_junc + 8)], 1).astype(F)
        extra = np.unique(extra, axis=0)
        extra = rng.permutation(np.array([e for e in extra if not (ends == e).all(1).any()], F).reshape(-1, 2))
        _scenes[key] = (np.ascontiguousarray(np.concatenate([ends, extra])[:n_junc], F), heat)
    return _scenes[key]


def cfg_with(**kw):
    c = json.loads(json.dumps(gen.SHIPPED))
    c["heatmap_refine_cfg"]["num_blocks"] = 5
    c["junction_refine_cfg"]["num_perturbs"] = 3
    c.update(kw)
    return c


def assert_same(dev, host):
    (sd, td), (sh, th) = dev, host
    assert len(sd) == len(sh)
    for a, b in zip(sd, sh):
        assert a.dtype == np.float64 and a.shape == b.shape and np.array_equal(a, b)
    for a, b in zip(td, th):
        assert np.array_equal(a["heatmap"].view(np.uint32), b["heatmap"].view(np.uint32))
        for k in ("candidates", "line_map", "pairs", "perturb"):
            assert np.array_equal(a[k], b[k]), k
        assert np.array_equal(a["segments_refined"].view(np.uint32), b["segments_refined"].view(np.uint32))
        for k in ("junctions_refined", "line_map_refined"):
            assert (a[k] is None) == (b[k] is None) and (a[k] is None or np.array_equal(a[k], b[k]))


def both(cfg, juncs, heats, module=None):
    m = module if module is not None else line2d.LineSegmentDetectionModule(**cfg)
    dev = line2d.detect_scene(m, juncs, heats, return_stages=True)
    host = line2d.detect_scene(m, juncs, heats, host=True, return_stages=True)
    assert_same(dev, host)
    return dev


@pytest.mark.parametrize("n", [0, 1, 2, 3, 63, 64, 65, 130])
def test_junction_counts_around_a_wave_and_the_table_passes(n):
    junc, heat = scene(11, 80, 96, 6, n)
    assert len(junc) == n
    segs, st = both(cfg_with(), [junc], [heat])
    if n >= 63:
        assert len(segs[0]) >= 3 and 0 < st[0]["candidates"].sum() < n * (n - 1) // 2


@pytest.mark.parametrize("shape", [(80, 96), (83, 101)])
@pytest.mark.parametrize("blocks", [1, 5, 20])
def test_refinement_blocks_and_a_block_below_valid_thresh(shape, blocks):
    junc, heat = scene(12, shape[0], shape[1], 6, 30)
    heat = heat.copy()
    heat[: shape[0] // 3, : shape[1] // 3] *= F(1e-4)  # whole blocks stay below valid_thresh
    c = cfg_with()
    c["heatmap_refine_cfg"]["num_blocks"] = blocks
    segs, st = both(c, [junc], [heat])
    scales, bounds = line2d.block_scales_host(c, heat)
    assert scales.shape == (blocks, blocks)
    if blocks == 20:
        assert (scales < 0).any() and (scales > 0).any()
        if shape == (80, 96):  # round(80 / 10.5) x round(96 / 10.5)
            assert (bounds[0, 1] - bounds[0, 0], bounds[0, 3] - bounds[0, 2]) == (8, 9)
    g = cfg_with(heatmap_refine_cfg={"mode": "global", "ratio": 0.2, "valid_thresh": 0.01})
    both(g, [junc], [heat])


@pytest.mark.parametrize("samples", [2, 5, 64])
@pytest.mark.parametrize("method", ["local_max", "bilinear"])
def test_sample_counts_and_methods(samples, method):
    junc, heat = scene(13, 83, 101, 6, 40)
    segs, _ = both(cfg_with(num_samples=samples, sampling_method=method, inlier_thresh=0.6, detect_thresh=0.3), [junc], [heat])
    # (two bilinear samples sit on the integer junctions themselves, where the reference's form weighs 0)
    assert len(segs[0]) > 0 or (samples, method) == (2, "bilinear")


@pytest.mark.parametrize("radius", [1, 3, 4])
def test_patch_radius(radius):
    junc, heat = scene(14, 80, 96, 6, 40)
    segs, _ = both(cfg_with(max_local_patch_radius=radius, lambda_radius=40.0), [junc], [heat])
    assert len(segs[0]) > 0


@pytest.mark.parametrize("perturbs", [1, 3, 9])
def test_perturbation_counts(perturbs):
    junc, heat = scene(15, 83, 101, 6, 30)
    c = cfg_with()
    c["junction_refine_cfg"] = {"num_perturbs": perturbs, "perturb_interval": 0.25}
    segs, st = both(c, [junc], [heat])
    assert len(st[0]["perturb"]) > 0 and st[0]["perturb"].max() < perturbs ** 4
    if perturbs == 9:
        assert len(set(st[0]["perturb"].tolist())) > 1


def test_both_heatmap_paths_of_the_junction_refinement():
    """120 x 130 = 15 600 floats: the window of a segment across the whole image does not fit the LDS window (12 288
    floats) and is read from global memory, a short one is staged; with the window switched off every segment takes the
    global path, with a small one most do -- the same bits every time"""
    H, W = 120, 130
    rng = np.random.default_rng(16)
    lines = np.array([[[2.3, 2.6], [116.4, 126.7]], [[60.2, 20.3], [64.6, 52.1]], [[100.5, 10.2], [20.3, 100.8]]])
    heat = gen.ridge_heatmap(rng, H, W, lines)
    junc = np.round(lines.reshape(-1, 2)).astype(F)
    c = cfg_with(use_candidate_suppression=False)
    c["junction_refine_cfg"] = {"num_perturbs": 9, "perturb_interval": 0.25}
    m = line2d.LineSegmentDetectionModule(**c)
    ref = both(c, [junc], [heat], m)
    assert len(ref[1][0]["pairs"]) >= 3
    spans = [abs(junc[i] - junc[j]) + 7 for i, j in ref[1][0]["pairs"]]
    assert any(s[0] * s[1] > 12288 for s in spans) and any(s[0] * s[1] < 4000 for s in spans)
    for window in (0, 4000):
        m.lds_window_floats = window
        assert_same(line2d.detect_scene(m, [junc], [heat], return_stages=True), ref)


def test_plateau_takes_the_lowest_perturbation_index():
    junc, heat = scene(17, 80, 96, 6, 24, profile="box")
    c = cfg_with()
    c["junction_refine_cfg"] = {"num_perturbs": 9, "perturb_interval": 0.25}
    segs, st = both(c, [junc], [heat])
    assert len(st[0]["perturb"]) > 0
    # on the plateau many perturbed segments reach the same mean: the chosen one is the first of them
    heat_r, vec = st[0]["heatmap"], line2d._perturb_vec(9, 0.25)
    tied = 0
    for (i, j), p in zip(st[0]["pairs"], st[0]["perturb"]):
        obj, _, ps = gen.perturb_objectives(heat_r, np.concatenate([junc[i], junc[j]]), vec, line2d.linspace_sampler(64))
        same = np.nonzero(obj == obj[p])[0]
        tied += len(same) > 1
        if obj[p] == 1.0:  # a mean of exactly 1 is exact in every summation order
            assert p == same[0]
    assert tied > 0


def test_ragged_batch_equals_one_by_one():
    specs = [(21, 80, 96, 5, 40), (22, 83, 101, 6, 65), (23, 40, 50, 0, 0), (24, 64, 64, 3, 7), (25, 96, 80, 5, 130)]
    juncs, heats = zip(*[scene(*s) for s in specs])
    c = cfg_with()
    batch = both(c, list(juncs), list(heats))
    assert sum(len(s) for s in batch[0]) > 5 and len(batch[0][2]) == 0
    for k in range(len(specs)):
        one = line2d.detect_scene(c, [juncs[k]], [heats[k]], return_stages=True)
        assert_same(([batch[0][k]], [batch[1][k]]), one)


def test_torch_gpu_tensors_in_and_out_equal_numpy():
    import torch
    junc, heat = scene(26, 83, 101, 6, 50)
    c = cfg_with()
    m = line2d.LineSegmentDetectionModule(**c)
    want = line2d.detect_scene(m, [junc], [heat], return_stages=True)
    tj, th = torch.from_numpy(junc).cuda(), torch.from_numpy(heat).cuda()
    assert_same(line2d.detect_scene(m, [tj], [th], return_stages=True), want)
    # a strided view is read in place through its row stride
    wide = torch.zeros((83, 128), device="cuda")
    wide[:, :101] = th
    assert_same(line2d.detect_scene(m, [tj], [wide[:, :101]], return_stages=True), want)
    line_map, junctions, refined = m.detect(tj, th)
    assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in (line_map, junctions, refined))
    nl, nj, nh = m.detect(junc, heat)
    assert np.array_equal(line_map.cpu().numpy(), nl) and np.array_equal(junctions.cpu().numpy(), nj)
    assert np.array_equal(refined.cpu().numpy(), nh)


def _views():
    """two synthetic views of one set of lines: the second is the first moved by a few pixels"""
    rng = np.random.default_rng(31)
    H, W = 96, 128
    lines = []
    while len(lines) < 10:
        a, b = rng.uniform([6, 6], [H - 9, W - 9]), rng.uniform([6, 6], [H - 9, W - 9])
        if np.linalg.norm(a - b) > 25:
            lines.append(np.stack([a, b]))
    lines = np.array(lines)
    base = rng.normal(size=(64, H // 12 + 2, W // 12 + 2))
    desc = np.kron(base, np.ones((1, 3, 3)))[:, : H // 4, : W // 4][None].astype(F)
    views = []
    for shift in (np.zeros(2), np.array([2.0, 3.0])):
        ln = lines + shift
        heat = gen.ridge_heatmap(rng, H, W, ln)
        views.append((np.round(ln.reshape(-1, 2)).astype(F), heat, desc))
    return views


def test_descinfo_bits_and_the_way_into_sold2matcher():
    import torch
    views = _views()
    c = cfg_with(use_candidate_suppression=False)
    segs = line2d.detect_scene(c, [v[0] for v in views], [v[1] for v in views])
    assert all(len(s) >= 8 for s in segs)
    descs = [v[2] for v in views]
    dev = line2d.compute_descinfo_scene(segs, descs)
    host = line2d.compute_descinfo_scene(segs, descs, host=True)
    for (dd, dv), (hd, hv) in zip(dev, host):
        assert dd.shape == (64, 5 * len(dv)) and np.array_equal(dd.view(np.uint32), hd.view(np.uint32))
        assert np.array_equal(dv, hv)
    on_gpu = line2d.compute_descinfo_scene(segs, [torch.from_numpy(d).cuda() for d in descs])
    for (gd, gv), (hd, hv) in zip(on_gpu, host):
        assert gd.is_cuda and np.array_equal(gd.cpu().numpy().view(np.uint32), hd.view(np.uint32))
    # C that is no multiple of the wave, an image without segments, points outside the map (zero padding)
    odd = np.random.default_rng(5).normal(size=(1, 70, 9, 11)).astype(F)
    far = np.array([[[0.0, 0.0], [35.9, 43.9]], [[-3.0, -2.0], [50.0, 60.0]]])
    d1 = line2d.compute_descinfo_scene([far, np.zeros((0, 2, 2))], [odd, odd])
    h1 = line2d.compute_descinfo_scene([far, np.zeros((0, 2, 2))], [odd, odd], host=True)
    assert np.array_equal(d1[0][0].view(np.uint32), h1[0][0].view(np.uint32)) and d1[1].shape == (0,)
    matcher = matching.SOLD2Matcher()
    got = matcher.match_scene({0: dev[0], 1: dev[1]}, {0: [1], 1: [0]})
    want = matching.match_pair_host(host[0], host[1], "sold2", topk=matcher.topk)
    assert sorted(map(tuple, got[0][1])) == sorted(map(tuple, want))
    rows = matcher.match_segs_with_descinfo(dev[0], dev[1])
    assert len(rows) >= 5
    assert np.array_equal(rows, matching.match_pair_host(host[0], host[1], "sold2", topk=0))
    # matched lines are the same line of the scene, moved by (2, 3)
    a, b = segs[0][rows[:, 0]], segs[1][rows[:, 1]] - np.array([2.0, 3.0])
    close = np.minimum(np.abs(a - b).max((1, 2)), np.abs(a - b[:, ::-1]).max((1, 2))) < 4.0
    assert close.mean() > 0.7


def test_kernel_times_are_reported():
    junc, heat = scene(27, 80, 96, 6, 40)
    line2d.detect_scene(cfg_with(), [junc], [heat])
    ms = line2d.kernel_ms()
    assert set(ms) == set(line2d.KERNEL_MS_KEYS) and ms["kernels"] > 0 and ms["call"] >= ms["kernels"]
