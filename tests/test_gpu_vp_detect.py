"""-m gpu: limap_amd.vplib on the device.  Zero tolerance throughout: labels exact, vanishing points by bit pattern,
against tests/vp_oracle.py (DESIGN.md section 18 and the reference's tail), against the host path, batched against
single images, on the Manhattan scenes against the values the golden generator recorded, and end to end into the
VP-guided proposals of the triangulator."""
import json
import os

import numpy as np
import pytest

import vp_oracle as vo
from test_vp_host import GOLD, NAMES, bits, load, random_scene

pytestmark = pytest.mark.gpu


def _device(lines, cfg):
    from limap_amd import vplib
    (r, clu), = vplib._detect([np.ascontiguousarray(lines, np.float64).reshape(-1, 4)], vplib.BaseVPDetectorConfig(cfg),
                              clusters=True)
    return r, clu


def _check(lines, cfg):
    r, clu = _device(lines, cfg)
    o = vo.detect(lines, cfg)
    assert np.array_equal(clu, o["clusters"])
    assert np.array_equal(np.asarray(r.labels, np.int64), o["labels"])
    assert np.array_equal(bits(r.vps), bits(o["vps"]))
    return r, o


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_oracle_on_the_goldens(gpu_lib, name):
    z, cfg = load(name)
    r, _ = _check(z["lines"], cfg)
    if z["from_oracle"]:  # ... and so the reference's own tail
        assert np.array_equal(np.asarray(r.labels, np.int64), z["ref_labels"])
        assert np.array_equal(bits(r.vps), bits(z["ref_vps"]))


@pytest.mark.parametrize("seed", [0, 7])
def test_random_clutter_two_seeds(gpu_lib, seed):
    lines = random_scene(np.random.default_rng(21), 300)
    r, o = _check(lines, dict(seed=seed))
    assert o["vps"].shape[0] > 0


# 63 / 64 / 65: a word of the preference set; 511 / 512 / 513: the tile k_vp_pref stages (kVpHypTile); 1024 and 4096 end
# exactly on a tile
@pytest.mark.parametrize("n_hyp", [1, 64, 65, 5000, 63, 511, 512, 513, 1024, 4096])
def test_num_hypotheses(gpu_lib, n_hyp):
    _check(random_scene(np.random.default_rng(22), 150), dict(num_hypotheses=n_hyp, seed=1))


def _long_lines(rng, n):
    """n lines of 45 .. 200 pixels, a quarter of them through each of three points"""
    lines = random_scene(rng, n, n_pencils=3)
    ln = vo.lengths(lines)
    d = (lines[:, 2:] - lines[:, :2]) / ln[:, None]
    lines[:, 2:] = lines[:, :2] + d * np.maximum(ln, 45.0)[:, None]
    return lines


@pytest.mark.parametrize("n_valid", [0, 1, 19, 20, 1500])
def test_valid_line_counts(gpu_lib, n_valid):
    rng = np.random.default_rng(100 + n_valid)
    c = rng.uniform([0, 0], [1024, 768], (6, 2))
    short = np.concatenate([c, c + rng.uniform(-20, 20, (6, 2))], 1)
    lines = np.concatenate([_long_lines(rng, n_valid) if n_valid else np.zeros((0, 4)), short], 0)
    lines = lines[rng.permutation(lines.shape[0])]
    assert int((vo.lengths(lines) >= 40.0).sum()) == n_valid
    r, o = _check(lines, None)
    if n_valid < 20:
        assert (o["labels"] == -1).all() and r.count_vps() == 0
    if n_valid == 1500:
        assert r.count_vps() > 0


def _with_short_lines(rng, n_valid):
    """n_valid lines that pass the length filter and six that do not, shuffled"""
    c = rng.uniform([0, 0], [1024, 768], (6, 2))
    short = np.concatenate([c, c + rng.uniform(-20, 20, (6, 2))], 1)
    lines = np.concatenate([_long_lines(rng, n_valid), short], 0)
    lines = lines[rng.permutation(lines.shape[0])]
    assert int((vo.lengths(lines) >= 40.0).sum()) == n_valid
    return lines


# the 256-line blocks of k_vp_pref (kVpBlock) and the 512 lanes of k_vp_cluster, at the default configuration
@pytest.mark.parametrize("n_valid", [255, 256, 257, 511, 512, 513])
def test_valid_line_counts_on_block_edges(gpu_lib, n_valid):
    r, o = _check(_with_short_lines(np.random.default_rng(200 + n_valid), n_valid), None)
    assert r.count_vps() > 0


# the edge of the LDS state of k_vp_cluster (kVpLdsClusters = 2048): above it the state lives in global memory
@pytest.mark.parametrize("n_valid,n_hyp", [(2047, 512), (2048, 512), (2049, 512), (2600, 320)])
def test_valid_line_counts_on_the_lds_edge(gpu_lib, n_valid, n_hyp):
    assert (n_valid > 2048) == (n_valid in (2049, 2600))
    r, o = _check(_with_short_lines(np.random.default_rng(300 + n_valid), n_valid), dict(num_hypotheses=n_hyp))
    assert r.count_vps() > 0


def _same_results(got, want):
    assert len(got) == len(want)
    for k, ((r, clu), (h, hclu)) in enumerate(zip(got, want)):
        assert r.labels == h.labels and np.array_equal(clu, hclu) and np.array_equal(bits(r.vps), bits(h.vps)), k


def _against_oracle(lines, cfg, r, clu):
    o = vo.detect(lines, cfg)
    assert np.array_equal(clu, o["clusters"])
    assert np.array_equal(np.asarray(r.labels, np.int64), o["labels"])
    assert np.array_equal(bits(r.vps), bits(o["vps"]))


def test_batch_of_300_mixed_images(gpu_lib):
    """more workgroups than compute units, images below the guard, empty ones and one above 2048 valid lines in one
    call: every image against the host path, twelve against the oracle"""
    from limap_amd import vplib
    rng = np.random.default_rng(25)
    sizes = rng.integers(20, 200, 300)
    sizes[[3, 40, 41, 150, 299]] = [19, 0, 7, 1, 12]  # below the guard
    sizes[120] = 2100
    scenes = [_with_short_lines(rng, int(n)) if n else np.zeros((0, 4)) for n in sizes]
    assert int((vo.lengths(scenes[120]) >= 40.0).sum()) > 2048
    cfg = dict(num_hypotheses=192, seed=3)
    got = vplib._detect(scenes, vplib.BaseVPDetectorConfig(cfg), clusters=True)
    _same_results(got, vplib._detect_host(scenes, vplib.BaseVPDetectorConfig(cfg), clusters=True))
    for k in (0, 3, 40, 41, 77, 119, 120, 121, 150, 200, 298, 299):
        _against_oracle(scenes[k], cfg, *got[k])
    assert all(got[k][0].count_vps() == 0 and (got[k][1] == -1).all() for k in (3, 40, 41, 150, 299))
    assert sum(r.count_vps() for r, _ in got) > 100


def test_65536_active_images(gpu_lib):
    """one more image than a 16-bit grid dimension holds: k_vp_hyp takes the image from blockIdx.x, so the scene is
    computed like any other.  Every image against the host path, 50 against the oracle"""
    from limap_amd import vplib
    n_img = 65536
    rng = np.random.default_rng(26)
    lines = _long_lines(rng, 20 * n_img)
    assert (vo.lengths(lines) >= 40.0).all()  # 20 valid lines each: every image passes the guard and is active
    scenes = list(lines.reshape(n_img, 20, 4))
    cfg = dict(num_hypotheses=1)
    got = vplib._detect(scenes, vplib.BaseVPDetectorConfig(cfg), clusters=True)
    _same_results(got, vplib._detect_host(scenes, vplib.BaseVPDetectorConfig(cfg), clusters=True))
    for k in np.concatenate([[0, 65534, 65535], rng.choice(n_img, 47, replace=False)]):
        _against_oracle(scenes[int(k)], cfg, *got[int(k)])
    assert all((clu >= 0).all() for _, clu in got)
    assert sum(len(set(clu.tolist())) < 20 for _, clu in got) > n_img // 2  # the hypothesis' own two lines merge


def test_no_lines_at_all(gpu_lib):
    r, o = _check(np.zeros((0, 4)), None)
    assert r.labels == [] and r.vps == []


def test_duplicated_lines(gpu_lib):
    rng = np.random.default_rng(23)
    a = random_scene(rng, 60)
    _check(np.concatenate([a, a[:30], a[:10]], 0)[rng.permutation(100)], dict(num_hypotheses=800))


def test_batch_equals_single_images_equals_host(gpu_lib):
    from limap_amd import vplib
    rng = np.random.default_rng(24)
    scenes = {11: random_scene(rng, 140), 3: np.zeros((0, 4)), 8: random_scene(rng, 19), 5: random_scene(rng, 400),
              6: random_scene(rng, 21), 2: random_scene(rng, 300)}
    cfg = dict(method="jlinkage", num_hypotheses=1500, seed=5)
    det = vplib.get_vp_detector(cfg)
    res = det.detect_vp_all_images(scenes)
    assert list(res) == list(scenes)
    host = vplib.detect_vps_host(scenes, cfg)
    for k, lines in scenes.items():
        one = det.detect_vp(lines)
        for other in (one, host[k]):
            assert other.labels == res[k].labels and np.array_equal(bits(other.vps), bits(res[k].vps))
    assert sum(r.count_vps() for r in res.values()) > 0
    # lines in the other accepted forms
    from limap_amd.base import Line2d
    as_objs = [Line2d(l[:2].copy(), l[2:].copy()) for l in scenes[11]]
    assert det.detect_vp(as_objs).labels == res[11].labels
    assert det.detect_vp(scenes[11].reshape(-1, 2, 2)).labels == res[11].labels


def test_manhattan_recovery_is_the_recorded_one(gpu_lib):
    """The generator ran the oracle on these scenes, refused any in which a true direction got no vanishing point, and
    recorded angular error and label share per direction: the device reproduces exactly those values."""
    with open(os.path.join(GOLD, "vp_recovery.json")) as f:
        rec = json.load(f)
    assert len(rec) >= 2
    for name, want in rec.items():
        z, cfg = load(name)
        r, _ = _device(z["lines"], cfg)
        got = vo.recovery(z["dirs"], np.asarray(r.labels), np.asarray(r.vps).reshape(-1, 3), z["K"], z["R"])
        assert got == want
        assert all(w["vp"] >= 0 and w["angle_deg"] < 1.0 and w["share"] > 0.9 for w in want)
        assert len({w["vp"] for w in want}) == 3


def test_rejected_configurations(gpu_lib):
    lines = random_scene(np.random.default_rng(0), 30)
    for bad in (dict(min_num_supports=2), dict(num_hypotheses=0), dict(num_hypotheses=1 << 21)):
        with pytest.raises(ValueError):
            _device(lines, bad)


def test_end_to_end_into_the_triangulator(gpu_lib, oracle):
    """get_vp_detector(...).detect_vp_all_images -> InitVPResults -> triangulation with use_vp: equal to the oracle
    triangulator fed the same VPResults"""
    from limap_amd import synthetic as syn, triangulation as tri, vplib
    from helpers import compare_best, compare_candidates, compare_tracks, compare_valid_edges
    sc = syn.make_scene(n_views=10, n_segs=120, n_neighbors=4, seed=51)
    all_2d_lines = {int(i): sc.segs_of(n) for n, i in enumerate(sc.img_ids)}
    vp_cfg = dict(method="jlinkage", min_length=15.0, inlier_threshold=1.5, min_num_supports=5, num_hypotheses=2000)
    vpresults = vplib.get_vp_detector(vp_cfg, n_jobs=1).detect_vp_all_images(all_2d_lines, None)
    assert list(vpresults) == list(all_2d_lines)
    assert sum(r.count_vps() for r in vpresults.values()) >= len(all_2d_lines)  # the box's axes are found
    for k in list(all_2d_lines)[:3]:
        o = vo.detect(all_2d_lines[k], vp_cfg)
        assert np.array_equal(np.asarray(vpresults[k].labels), o["labels"]) and \
            np.array_equal(bits(vpresults[k].vps), bits(o["vps"]))
    cfg = syn.default_triangulation_cfg(debug_mode=True)
    cfg.update(use_vp=True)
    T = tri.GlobalLineTriangulator(cfg)
    O = oracle.OracleTriangulator(cfg, faithful=False)
    T.SetRanges(sc.ranges); O.SetRanges(sc.ranges)
    T.InitArrays(sc.img_ids, sc.kvec, sc.qvec, sc.tvec, [sc.segs_of(i) for i in range(sc.n_images)])
    O.Init(sc.img_ids, sc.kvec, sc.qvec, sc.tvec, sc.seg_off, sc.segs)
    T.InitVPResults(vpresults)  # the VPResult objects as they are
    O.InitVPResults({k: (np.asarray(r.labels, np.int32), np.asarray(r.vps, float).reshape(-1, 3))
                     for k, r in vpresults.items()})
    assert T.GetVPResult(int(sc.img_ids[0])) is vpresults[int(sc.img_ids[0])]
    for i in sc.img_ids:
        m = sc.matches_of(int(i))
        T.TriangulateImage(int(i), m)
        O.TriangulateImage(int(i), m)
    g, o = T.context().get_all_tris(), O.get_all_tris()
    from helpers import run_product
    n_alg = run_product(sc, dict(cfg, use_vp=False)).context().stats()["candidates"]
    assert g["off"][-1] > n_alg  # the VP branch contributes candidates
    compare_candidates(g, o)
    compare_best(T.context().get_best(), O.get_best())
    compare_valid_edges(T.context().get_valid_edges(), O.get_valid_edges())
    T.context().compute_tracks()
    compare_tracks(T.context().get_tracks(), O.ComputeLineTracks())
