"""limap_amd.vplib without a GPU: tests/vp_oracle.py (a literal restatement of DESIGN.md section 18 and of the
reference's tail) reproduces every golden the reference's own code wrote (tests/golden/make_vp_golden.py) bit for
bit; the library's host path equals the oracle; the clustering's order on cases worked out by hand; the Python API."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import vp_cluster_cases as vcc
import vp_oracle as vo

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vp")
NAMES = sorted(os.path.basename(p)[3:-4] for p in glob.glob(os.path.join(GOLD, "vp_*.npz")))


def load(name):
    z = np.load(os.path.join(GOLD, f"vp_{name}.npz"))
    cfg = {k[4:]: z[k].item() for k in z.files if k.startswith("cfg_")}
    return z, cfg


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64).reshape(-1, 3)).view(np.uint64)


def test_fixtures_cover_the_cases():
    assert {"guard19", "guard20", "len_at", "len_under", "tail", "tail_cfg", "parallel", "empty", "two_pencils",
            "duplicates", "manhattan0", "manhattan1"} <= set(NAMES)
    z, cfg = load("guard19")
    assert z["ref_sample_calls"] == 0 and (z["ref_labels"] == -1).all()
    z, cfg = load("guard20")
    assert z["ref_sample_calls"] == 1 and z["ref_vps"].shape[0] == 1
    z, _ = load("len_at")
    assert vo.lengths(z["lines"])[20] == 40.0 and z["ref_cluster_calls"] == 1
    z, _ = load("len_under")
    assert vo.lengths(z["lines"])[20] < 40.0 and z["ref_cluster_calls"] == 0
    z, _ = load("parallel")
    assert abs(z["ref_vps"][0, 2]) < 1e-12  # at infinity
    z, cfg = load("tail_cfg")
    assert cfg["th_perp_supports"] == 8.0 and z["ref_vps"].shape[0] == 3  # 3.0 is what the reference uses


@pytest.mark.parametrize("name", NAMES)
def test_oracle_reproduces_the_reference(name):
    z, cfg = load(name)
    lines = z["lines"]
    ids, go = (np.zeros(0, np.int64), False) if lines.shape[0] == 0 else vo.valid_lines(lines, cfg)
    assert bool(z["ref_cluster_calls"]) == go
    if go:  # what the reference handed to the clustering call: the valid lines, rounded to FP32
        assert np.array_equal(z["ref_seen_pts"], lines[ids].astype(np.float32))
        assert z["ref_seen_threshold"] == np.float32(cfg["inlier_threshold"])
    labels, vps = vo.tail(lines, ids, z["injected"] if go else None, cfg)
    assert np.array_equal(labels, z["ref_labels"])
    assert np.array_equal(bits(vps), bits(z["ref_vps"]))
    if z["from_oracle"]:
        o = vo.detect(lines, cfg)
        assert np.array_equal(o["labels"], z["ref_labels"]) and np.array_equal(bits(o["vps"]), bits(z["ref_vps"]))


def _host(lines, cfg):
    from limap_amd import vplib
    (r, clu), = vplib._detect_host([np.ascontiguousarray(lines, np.float64).reshape(-1, 4)],
                                   vplib.BaseVPDetectorConfig(cfg), 2, clusters=True)
    return r, clu


def _same(r, clu, o):
    assert np.array_equal(clu, o["clusters"])
    assert np.array_equal(np.asarray(r.labels, np.int64), o["labels"])
    assert np.array_equal(bits(r.vps), bits(o["vps"]))


@pytest.mark.parametrize("name", NAMES)
def test_host_path_reproduces_the_goldens(gpu_lib, name):
    z, cfg = load(name)
    r, clu = _host(z["lines"], cfg)
    _same(r, clu, vo.detect(z["lines"], cfg))
    if z["from_oracle"]:
        assert np.array_equal(np.asarray(r.labels, np.int64), z["ref_labels"])
        assert np.array_equal(bits(r.vps), bits(z["ref_vps"]))


def random_scene(rng, n, n_pencils=2):
    c = rng.uniform([0, 0], [1024, 768], (n, 2))
    ang = rng.uniform(0, np.pi, n)
    h = 0.5 * rng.uniform(20, 200, n)[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
    lines = np.concatenate([c - h, c + h], 1)
    for p in range(n_pencils):  # a share of the lines through a common point
        k = rng.choice(n, n // 4, replace=False)
        pt = rng.uniform([-2000, -2000], [3000, 3000])
        d = lines[k, :2] - pt
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        lines[k, 2:] = lines[k, :2] + d * rng.uniform(45, 150, (len(k), 1)) + rng.normal(0, 0.2, (len(k), 2))
    return lines


@pytest.mark.parametrize("seed,n,cfg", [(1, 120, None), (2, 90, dict(num_hypotheses=65, seed=9)),
                                         (3, 200, dict(num_hypotheses=1000, inlier_threshold=2.0, min_num_supports=4)),
                                         (4, 60, dict(num_hypotheses=1)), (5, 64, dict(num_hypotheses=64, min_length=0.0))])
def test_host_path_equals_oracle_on_random_scenes(gpu_lib, seed, n, cfg):
    lines = random_scene(np.random.default_rng(seed), n)
    r, clu = _host(lines, cfg)
    _same(r, clu, vo.detect(lines, cfg))


def test_host_batch_equals_single_images(gpu_lib):
    from limap_amd import vplib
    rng = np.random.default_rng(7)
    scenes = {5: random_scene(rng, 80), 2: np.zeros((0, 4)), 9: random_scene(rng, 19), 1: random_scene(rng, 130)}
    cfg = dict(num_hypotheses=500)
    res = vplib.detect_vps_host(scenes, cfg)
    assert list(res) == [5, 2, 9, 1]
    for k, lines in scenes.items():
        one = vplib.detect_vps_host({0: lines}, cfg)[0]
        assert one.labels == res[k].labels and np.array_equal(bits(one.vps), bits(res[k].vps))
        assert res[k].count_lines() == lines.shape[0]


# ---- the clustering on cases worked out by hand ---------------------------------------------------------------------------
def _sets(sets, m=8):
    p = np.zeros((len(sets), m), bool)
    for k, s in enumerate(sets):
        p[k, list(s)] = True
    return p


def _lib_cluster(gpu_lib, pref):
    n, m = pref.shape
    w = (m + 63) // 64
    words = np.zeros((max(n, 1), w), np.uint64)
    for k in range(n):
        for b in np.nonzero(pref[k])[0]:
            words[k, b // 64] |= np.uint64(1) << np.uint64(b % 64)
    roots = np.zeros(max(n, 1), np.int32)
    rc = gpu_lib.lt_fn_vp_cluster_host(n, w, words.ctypes.data_as(C.POINTER(C.c_uint64)),
                                       roots.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == 0
    return roots[:n]


KAT = [
    # four sets in a ring, every neighbouring pair at 1/3: the tie goes to (0, 1); {1} then meets nothing, (2, 3) follows
    ([{0, 1}, {1, 2}, {2, 3}, {3, 0}], [0, 0, 2, 2]),
    # the same ratio 2/3 for (0, 2) and (1, 3), ahead of (1, 2) at 1/4 and (2, 3) at 1/5: smallest i first, then (1, 3)
    ([{0, 1}, {2, 3}, {1, 2, 0}, {3, 4, 2}], [0, 1, 0, 1]),
    # an empty preference set never merges, whatever else happens
    ([set(), {0}, {0}, set()], [0, 1, 1, 3]),
    # the greatest ratio first: (0, 1) at 4/5, not (1, 2) at 1/6; afterwards {0,1,2,3} and {4,5} do not meet: stop
    ([{0, 1, 2, 3}, {0, 1, 2, 3, 4}, {4, 5}], [0, 0, 2]),
    # disjoint sets: nothing to do; one cluster; none
    ([{0}, {1}, {2}], [0, 1, 2]),
    ([{3, 4}], [0]),
    ([], []),
    # equal ratios by cross-multiplication, 2/4 against 1/2: (0, 1) before (2, 3)
    ([{0, 1, 2}, {1, 2, 3}, {4}, {4, 5}], [0, 0, 2, 2]),
]


@pytest.mark.parametrize("sets,want", KAT)
def test_clustering_known_answers(gpu_lib, sets, want):
    pref = _sets(sets)
    assert vo.cluster(pref).tolist() == want
    assert _lib_cluster(gpu_lib, pref).tolist() == want


def test_clustering_random_sets_host_equals_oracle(gpu_lib):
    rng = np.random.default_rng(11)
    for n, m, p in ((40, 70, 0.2), (25, 130, 0.5), (60, 64, 0.05)):
        pref = rng.random((n, m)) < p
        assert _lib_cluster(gpu_lib, pref).tolist() == vo.cluster(pref).tolist()


def host_cluster(gpu_lib, pref):
    """lt_fn_vp_cluster_host on an (n, M) bool matrix"""
    words = vcc.pack(pref)
    n, w = words.shape
    roots = np.zeros(max(n, 1), np.int32)
    rc = gpu_lib.lt_fn_vp_cluster_host(n, w, words.ctypes.data_as(C.POINTER(C.c_uint64)),
                                       roots.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == 0
    return roots[:n]


def test_pack_is_the_layout_of_the_known_answers(gpu_lib):
    rng = np.random.default_rng(12)
    pref = rng.random((9, 130)) < 0.3
    words = vcc.pack(pref)
    assert words.shape == (9, 3) and words.dtype == np.uint64
    for k in range(9):
        for b in range(130):
            assert bool((int(words[k, b // 64]) >> (b % 64)) & 1) == bool(pref[k, b])
    assert np.array_equal(host_cluster(gpu_lib, pref), _lib_cluster(gpu_lib, pref))


# the members of 2047 rows and more take the oracle 2.5 - 8 s each, 62 s together: they run in tests/test_gpu_vp_cluster.py, where the host
# twin is compared with the oracle on them as well
HOST_CASES = vcc.all_cases(large=False)


@pytest.mark.parametrize("name,pref", HOST_CASES, ids=[c[0] for c in HOST_CASES])
def test_clustering_case_families_host_equals_oracle(gpu_lib, name, pref):
    assert np.array_equal(host_cluster(gpu_lib, pref), vo.cluster(pref))


def test_case_families_are_what_they_claim():
    cases = dict(vcc.all_cases())
    assert {n for n in vcc.RANDOM_N if n > vcc.LDS_CLUSTERS} == {2049, 2600}
    for n in vcc.RANDOM_N:
        for p in vcc.RANDOM_P:
            assert cases[f"random_n{n}_p{p}"].shape[0] == n
    assert all(cases[f"ties_n{n}"].all(0).sum() == 3 for n in (2, 3, 64, 65, 130))
    assert {m for m in (1, 63, 64, 65, 128, 5000)} == {cases[f"edge_bits_m{m}"].shape[1] for m in (1, 63, 64, 65, 128, 5000)}
    e = cases["empty_n50_m40"]
    assert not e[0].any() and not e[-1].any() and not e[10:20].any() and e.any(1).sum() > 20
    d = vo.cluster(cases["disjoint_40_groups"])
    assert 40 <= len(set(d.tolist())) and cases["disjoint_40_groups"].shape[0] > 400
    # the re-scan constructions do what their docstring says: L hub merges, then the leaves' next partners
    r = vo.cluster(cases["rescan_hub_high_a30_L4"])
    assert [int(r[30 + l]) for l in range(4)] == [0, 1, 2, 3]
    r = vo.cluster(cases["rescan_hub_low_a30_L4"])
    assert [int(r[30 + 2 * l + 1]) for l in range(4)] == [30, 32, 34, 36] and int(r[38]) == 0


# ---- the Python surface -----------------------------------------------------------------------------------------------------
def test_config_semantics():
    from limap_amd import vplib
    c = vplib.BaseVPDetectorConfig()
    assert c.as_dict() == dict(min_length=40.0, inlier_threshold=1.0, min_num_supports=5, th_perp_supports=3.0)
    assert (c.num_hypotheses, c.seed) == (5000, 0)
    c = vplib.BaseVPDetectorConfig(dict(method="jlinkage", min_length=25, min_num_supports=7.0, unknown_key=1, seed=3))
    assert c.as_dict() == dict(min_length=25.0, inlier_threshold=1.0, min_num_supports=7, th_perp_supports=3.0)
    assert c.seed == 3 and isinstance(c.min_num_supports, int)
    assert vplib.JLinkage(dict(inlier_threshold=2.5)).as_dict()["inlier_threshold"] == 2.5
    assert list(c.as_dict()) == ["min_length", "inlier_threshold", "min_num_supports", "th_perp_supports"]


def test_vpresult_api():
    from limap_amd import vplib
    r = vplib.VPResult([0, -1, 1, 0], [[1.0, 0, 0], [0, 1.0, 0]])
    assert (r.count_lines(), r.count_vps()) == (4, 2)
    assert r.GetVPLabel(2) == 1 and r.HasVP(0) and not r.HasVP(1)
    assert np.array_equal(r.GetVP(2), [0, 1.0, 0]) and np.array_equal(r.GetVPbyCluster(0), [1.0, 0, 0])
    with pytest.raises(ValueError, match="HasVP"):
        r.GetVP(1)
    d = r.as_dict()
    assert d["labels"] == [0, -1, 1, 0] and len(d["vps"]) == 2
    r2 = vplib.VPResult(d)
    assert r2.labels == r.labels and np.array_equal(np.array(r2.vps), np.array(r.vps))
    r3 = vplib.VPResult(r2)
    assert r3.labels == r.labels
    e = vplib.VPResult()
    assert e.count_lines() == 0 and e.count_vps() == 0 and vplib.VPResult({}).labels == []


def test_get_vp_detector():
    import limap_amd
    from limap_amd import vplib
    assert limap_amd.vplib is vplib and "vplib" in limap_amd.__all__
    det = vplib.get_vp_detector(dict(method="jlinkage", min_length=30), n_jobs=4)
    assert isinstance(det, vplib.JLinkage) and det.get_module_name() == "JLinkage" and det.n_jobs == 4
    assert det.config_.min_length == 30.0
    for method in ("progressivex", "deepvp"):
        with pytest.raises(NotImplementedError):
            vplib.get_vp_detector(dict(method=method))
    with pytest.raises(KeyError):
        vplib.get_vp_detector({})


def test_host_path_rejects_what_upstream_leaves_undefined(gpu_lib):
    from limap_amd import vplib
    lines = random_scene(np.random.default_rng(0), 30)
    for bad in (dict(min_num_supports=2), dict(num_hypotheses=0), dict(inlier_threshold=float("nan"))):
        with pytest.raises(ValueError):
            vplib.detect_vps_host({0: lines}, bad)
    with pytest.raises(ValueError):
        vplib.detect_vps_host({0: np.array([[0.0, 0.0, np.inf, 1.0]])})
