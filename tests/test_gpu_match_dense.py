"""The dense kind of limap_amd.matching on the device: lt_match_dense_pairs (match_scene_dense, DenseLineMatcher)
against the host restatement lt_fn_match_dense_pair_host, zero tolerance -- rows AND the FP32 dists of the returned rows
bit for bit -- at the edges of the 16 x 16 tile of k_dense_pairs, for every sample count and warp size, on the values
exactly on the thresholds, with non-finite warps, zero-length lines and ties across a tile edge; batching; the golden
fixtures; rejections; the end-to-end path into the triangulator ("Dense").  Nothing here reads the
reference tree."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import dense_cases as dc
from limap_amd import _capi, matching, synthetic as syn

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 15, 16, 17, 33, 130]  # lines per image: below, at and above the 16-wide tile, several tiles
Opts = matching.BaseDenseLineMatcherOptions
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "match_dense")


def _check(cases, opts, thresh=0.5, **kw):
    """cases = [(descinfo1, descinfo2, warps)]: one batched call over all of them == the restatement per pair (rows and
    score bits).  Returns the device rows per case."""
    descinfos, neighbors, warps = {}, {}, {}
    for q, (a, b, w) in enumerate(cases):
        descinfos[2 * q], descinfos[2 * q + 1] = a, b
        neighbors[2 * q] = [2 * q + 1]
        warps[(2 * q, 2 * q + 1)] = w
    out, sc = matching.match_scene_dense(descinfos, neighbors, warps, opts, thresh, return_scores=True, **kw)
    rows = []
    for q, (a, b, w) in enumerate(cases):
        w = [x.cpu().numpy() if hasattr(x, "cpu") else x for x in w]
        hr, hs = matching.match_dense_pair_host(a, b, w, opts, thresh, return_scores=True)
        got, gs = out[2 * q][2 * q + 1], sc[2 * q][2 * q + 1]
        assert got.dtype == np.int32 and got.shape == hr.shape, (q, got.shape, hr.shape)
        assert np.array_equal(got, hr), q
        assert np.array_equal(dc.bits(gs), dc.bits(hs)), q
        rows.append(got)
    return rows


@pytest.mark.parametrize("one_to_many", [False, True])
def test_tile_edges(one_to_many):
    rng = np.random.default_rng([61, int(one_to_many)])
    cases = [dc.overlapping_pair(rng, n1, n2) for n1 in SIZES for n2 in SIZES]
    cases += [dc.random_pair(rng, n1, n2) for n1 in SIZES for n2 in (1, 17, 130)]
    rows = _check(cases, Opts(one_to_many=one_to_many))
    assert sum(len(r) for r in rows) > 200
    t, k = matching.timers(), matching.dense_kernel_ms()
    assert (t >= 0).all() and t[1] > 0 and (k > 0).all()


@pytest.mark.parametrize("dims", [(1, 1), (1, 7), (5, 3), (40, 56)])
@pytest.mark.parametrize("S", [2, 21, 63, 64])
def test_sample_counts_and_warp_sizes(S, dims):
    rng = np.random.default_rng([62, S, dims[0], dims[1]])
    cases = [dc.overlapping_pair(rng, 17, 33, dims=dims), dc.random_pair(rng, 33, 17, dims, dims[::-1]),
             dc.homography_pair(rng, 20, 20, (48, 64), (40, 56), dims, dims, holes=2)]
    rows = _check(cases, Opts(n_samples=S, pixel_th=12.0))
    _check(cases, Opts(n_samples=S, pixel_th=12.0, one_to_many=True))
    if dims == (40, 56):
        assert len(rows[0]) > 0 and len(rows[2]) > 0


def test_torch_gpu_tensors_are_read_in_place():
    import torch
    rng = np.random.default_rng(63)
    cases = [dc.overlapping_pair(rng, 33, 17), dc.random_pair(rng, 17, 33), dc.homography_pair(
        rng, 20, 24, (48, 64), (40, 56), (24, 56), (48, 20), holes=2)]
    on_host = _check(cases, Opts())
    on_dev = [(a, b, tuple(torch.from_numpy(x).cuda() for x in w)) for a, b, w in cases]
    for x, y in zip(on_host, _check(on_dev, Opts())):
        assert np.array_equal(x, y)
    # a transposed view and a float64 tensor are made contiguous FP32 first
    odd = [(a, b, (w[0].double(), w[1].t().contiguous().t(), w[2], w[3])) for a, b, w in on_dev]
    for x, y in zip(on_host, _check(odd, Opts())):
        assert np.array_equal(x, y)
    # mixed: a pair on the host between pairs on the device
    for x, y in zip(on_host, _check([on_dev[0], cases[1], on_dev[2]], Opts())):
        assert np.array_equal(x, y)


def test_samples_on_texel_centres_on_the_border_and_outside():
    rng = np.random.default_rng(64)
    shape = (64, 64)
    w = rng.uniform(-1, 1, (64, 64, 2)).astype(np.float32)
    c = rng.uniform(0.4, 1.0, (64, 64)).astype(np.float32)
    lines = np.array([
        [[8.5, 32.5], [56.5, 32.5]],     # S = 5: every sample a texel centre
        [[0.0, 0.0], [64.0, 64.0]],      # both ends exactly on the -1 / +1 border
        [[0.0, 64.0], [64.0, 0.0]],
        [[-32.0, 10.0], [96.0, 10.0]],   # a quarter of the samples outside on either side
        [[32.0, -64.0], [32.0, 128.0]],
        [[-5.0, -5.0], [-50.0, -60.0]],  # wholly outside
        [[0.5, 0.5], [63.5, 63.5]],      # the first and the last texel centre
        [[64.0, 3.0], [64.0, 61.0]],     # along the +1 border
    ])
    a, b = dc.descinfo(lines, shape), dc.descinfo(dc.rand_lines(rng, 20, shape), shape)
    for S in (5, 21):
        for warps in ((w, c, w[::-1].copy(), c), (dc.identity_warp((64, 64)), c, dc.identity_warp((7, 3)), c[:7, :3].copy())):
            _check([(a, b, warps), (b, a, warps)], Opts(n_samples=S, pixel_th=30.0, one_to_many=True))
            _check([(a, a, warps)], Opts(n_samples=S, pixel_th=30.0))


@pytest.mark.parametrize("name", dc.THRESHOLD_CASES)
def test_values_on_the_thresholds(name):
    a, b, warps, o, thresh, want = dc.threshold_case(name)
    rows = _check([(a, b, warps)], Opts(**o), thresh)
    assert np.array_equal(rows[0], want), name


def test_non_finite_warps_and_zero_length_lines():
    rng = np.random.default_rng(65)
    a, b, w = dc.overlapping_pair(rng, 33, 33)
    w = [x.copy() for x in w]
    w[0][5:9, 10:30, 0] = np.nan
    w[0][20:24, 10:30, 1] = np.inf
    w[2][7, :, :] = -np.inf
    w[1][30:33, :] = np.nan
    w[3][12, 5:9] = np.inf
    w[2][30:, 40:, 0] = 3.0e38
    a["lines"][4, 1] = a["lines"][4, 0]
    b["lines"][4, 1] = b["lines"][4, 0]
    b["lines"][17, 0] = b["lines"][17, 1]
    for otm in (False, True):
        rows = _check([(a, b, w), (b, a, (w[2], w[3], w[0], w[1]))], Opts(one_to_many=otm))
        assert len(rows[0]) > 0
        assert 4 not in rows[0][:, 0] and 4 not in rows[0][:, 1] and 17 not in rows[0][:, 1]


def test_ties_of_the_row_minimum_across_a_tile_edge():
    rng = np.random.default_rng(66)
    a, b, w = dc.overlapping_pair(rng, 40, 40, jitter=0.5)
    b["lines"][19] = b["lines"][3]    # another tile
    b["lines"][16] = b["lines"][15]   # either side of a tile edge
    b["lines"][39] = b["lines"][15]
    rows = _check([(a, b, w)], Opts())[0]
    pairs = set(map(tuple, rows.tolist()))
    assert {(3, 3), (3, 19), (15, 15), (15, 16), (15, 39)} <= pairs


def test_batching_equals_single_pairs():
    rng = np.random.default_rng(67)
    dims = [(1, 1), (1, 7), (5, 3), (40, 56), (24, 56), (48, 20)]
    cases = []
    for q in range(12):
        n1, n2 = int(rng.integers(0, 40)), int(rng.integers(0, 40))
        d12, d21 = dims[q % 6], dims[(q + 2) % 6]
        cases.append(dc.homography_pair(rng, n1, n2, (48, 64), (40, 56), d12, d21, holes=1) if q % 2 else
                     dc.random_pair(rng, n1, n2, d12, d21))
    opts = Opts(pixel_th=15.0)
    whole = _check(cases, opts)
    assert sum(len(r) for r in whole) > 0
    for budget in (1, 4096, 20000):   # a call per pair, a few pairs per call
        for x, y in zip(whole, _check(cases, opts, warp_bytes=budget)):
            assert np.array_equal(x, y)
    for x, c in zip(whole, cases):
        assert np.array_equal(x, _check([c], opts)[0])


class _Fixed(matching.BaseDenseMatcher):
    def __init__(self, warps, thresh):
        self.warps, self.thresh = warps, thresh

    def get_sample_thresh(self):
        return self.thresh

    def get_warping_symmetric(self, img1, img2):
        return self.warps


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLD, "*.npz"))), ids=os.path.basename)
def test_golden_fixtures_on_the_device(path):
    z = np.load(path)
    a, b = dc.descinfo(z["lines1"], z["shape1"]), dc.descinfo(z["lines2"], z["shape2"])
    warps = (z["warp12"], z["cert12"], z["warp21"], z["cert21"])
    base = Opts(n_samples=int(z["n_samples"]), segment_percentage_th=float(z["segment_percentage_th"]),
                pixel_th=float(z["pixel_th"]))
    thresh = float(z["sample_thresh"])
    one = _check([(a, b, warps)], base, thresh)[0]
    many = _check([(a, b, warps)], base._replace(one_to_many=True), thresh)[0]
    name = os.path.basename(path)[:-4]
    if name in ("zero_length_12_12", "tie_10_12", "empty_0_9", "empty_9_0", "two_samples_17_16"):  # fully decided
        assert np.array_equal(one, z["ref_one"]) and np.array_equal(many, z["ref_many"])
    # the matcher class: upstream's method names over the same call
    m = matching.DenseLineMatcher(matching.DenseNaiveExtractor(), _Fixed(warps, thresh), base,
                                  matching.BaseMatcherOptions(topk=0))
    assert np.array_equal(m.match_pair(a, b), one)
    assert np.array_equal(m.match_segs_with_descinfo(a, b), one)
    assert np.array_equal(m.match_segs_with_descinfo_topk(a, b, topk=3), many)  # topk is ignored, as upstream
    m10 = matching.DenseLineMatcher(None, _Fixed(warps, thresh), base, matching.BaseMatcherOptions(topk=10))
    assert np.array_equal(m10.match_pair(a, b), many)
    h = matching.match_dense_dists_host(a, b, warps, base, thresh)
    d, o = m.compute_distance_one_direction(a, b, warps[0], warps[1])
    assert d.shape == h[0].shape and np.array_equal(dc.bits(d), dc.bits(h[0])) and np.array_equal(dc.bits(o), dc.bits(h[1]))
    d, o = m.compute_distance_one_direction(b, a, warps[2], warps[3])
    assert d.shape == h[2].shape and np.array_equal(dc.bits(d), dc.bits(h[2])) and np.array_equal(dc.bits(o), dc.bits(h[3]))


def _raw(ctx, n_samples=21, dims=(2, 2, 2, 2, 2, 2, 2, 2), shapes=(48, 64, 48, 64), pair=(0, 1), pixel_th=10.0, n=3):
    lines = np.tile(np.array([[1, 2, 30, 20]], np.float32), (2 * n, 1))
    line_off = _capi.i64([0, n, 2 * n])
    w, c = np.zeros((4, 4, 2), np.float32), np.zeros((4, 4), np.float32)
    wp, cp = (C.c_void_p * 2)(w.ctypes.data, w.ctypes.data), (C.c_void_p * 2)(c.ctypes.data, c.ctypes.data)
    cfg = _capi.LtMatchDenseConfig(n_samples, 0, 0.2, pixel_th, 0.5, 0, 0, 0)
    return ctx.L.lt_match_dense_pairs(ctx.h, 2, _capi.ptr(line_off, C.c_int64), lines.ctypes.data_as(C.POINTER(C.c_float)),
                                      _capi.ptr(_capi.i32(shapes), C.c_int32), 1, _capi.ptr(_capi.i32(pair), C.c_int32),
                                      wp, cp, _capi.ptr(_capi.i32(dims), C.c_int32), C.byref(cfg), None)


def test_rejected_before_any_launch():
    ctx = _capi.Context()

    def rejected(**kw):
        rc = _raw(ctx, **kw)
        msg = ctx.L.lt_last_error(ctx.h).decode()
        assert rc == -2 and msg.startswith("lt_match_dense_pairs: "), (rc, msg)
        return msg

    assert _raw(ctx) == 0
    for S in (1, 65, -3):
        assert "n_samples" in rejected(n_samples=S)
    assert "dims" in rejected(dims=(0, 2, 0, 2, 2, 2, 2, 2)) and "at least 1" in rejected(dims=(2, 2, 2, 2, 2, 0, 2, 0))
    assert "cert and warp shapes differ" in rejected(dims=(2, 2, 2, 3, 2, 2, 2, 2))
    assert "16384" in rejected(dims=(2, 16385, 2, 16385, 2, 2, 2, 2))
    assert "shapes" in rejected(shapes=(48, 0, 48, 64)) and "shapes" in rejected(shapes=(48, 64, -1, 64))
    assert "pair_img" in rejected(pair=(0, 2))
    assert "pixel_th" in rejected(pixel_th=float("nan"))
    assert _raw(ctx, n_samples=64) == 0 and _raw(ctx, n_samples=2) == 0  # the context still works
    ctx.close()
    rng = np.random.default_rng(68)
    a, b, w = dc.random_pair(rng, 4, 4)
    with pytest.raises(ValueError, match="n_samples"):
        matching.match_scene_dense({0: a, 1: b}, {0: [1]}, {(0, 1): w}, Opts(n_samples=65), 0.5)
    with pytest.raises(ValueError, match="shapes differ"):
        matching.match_scene_dense({0: a, 1: b}, {0: [1]}, {(0, 1): (w[0], w[1][:3], w[2], w[3])}, Opts(), 0.5)
    with pytest.raises(ValueError, match="sample_thresh"):
        matching.match_scene_dense({0: a, 1: b}, {0: [1]}, {(0, 1): w}, Opts())


def _plane_warps(sc, dims=(30, 40)):
    """per (image, neighbour) a homography fitted to the ground-truth correspondences of the two images' segments (the
    scene is made of planes), as a warp; the identity where fewer than four segments correspond"""
    shape = (syn.H_IMG, syn.W_IMG)

    def fit(p, q):
        A = []
        for (x, y), (u, v) in zip(p, q):
            A.append([-x, -y, -1, 0, 0, 0, u * x, u * y, u])
            A.append([0, 0, 0, -x, -y, -1, v * x, v * y, v])
        H = np.linalg.svd(np.asarray(A))[2][-1].reshape(3, 3)
        return H / H[2, 2]

    index = {int(i): k for k, i in enumerate(sc.img_ids)}
    cert = np.full(dims, 0.9, np.float32)
    out = {}
    for i, nbs in sc.neighbors.items():
        for j in nbs:
            ki, kj = index[int(i)], index[int(j)]
            g1, g2 = sc.gt_ids[sc.seg_off[ki]:sc.seg_off[ki + 1]], sc.gt_ids[sc.seg_off[kj]:sc.seg_off[kj + 1]]
            s1, s2 = sc.segs_of(ki), sc.segs_of(kj)
            p, q = [], []
            for l, g in enumerate(g1):
                w = np.nonzero(g2 == g)[0] if g >= 0 else []
                if len(w):
                    p += [s1[l, :2], s1[l, 2:4]]
                    q += [s2[w[0], :2], s2[w[0], 2:4]]
            H = fit(np.array(p) / 100.0, np.array(q) / 100.0) if len(p) >= 8 else np.eye(3)
            S = np.diag([100.0, 100.0, 1.0])
            H = S @ H @ np.linalg.inv(S)
            out[(int(i), int(j))] = (dc.homography_warp(H, dims, shape, shape), cert,
                                     dc.homography_warp(np.linalg.inv(H), dims, shape, shape), cert)
    return out


def test_end_to_end_into_the_triangulator():
    from limap_amd import triangulation as tri
    sc = syn.make_scene(n_views=8, n_segs=50, n_neighbors=3, seed=9)
    shape = (syn.H_IMG, syn.W_IMG)
    di = {int(i): dc.descinfo(sc.segs_of(k)[:, :4], shape) for k, i in enumerate(sc.img_ids)}
    warps = _plane_warps(sc)
    opts = Opts(pixel_th=25.0, one_to_many=True)
    dev = matching.match_scene_dense(di, sc.neighbors, warps, opts, 0.5)
    host = {int(i): {int(j): matching.match_dense_pair_host(di[int(i)], di[int(j)], warps[(int(i), int(j))], opts, 0.5)
                     for j in sc.neighbors[int(i)]} for i in sc.img_ids}
    n_rows = 0
    for i in host:
        for j in host[i]:
            assert np.array_equal(dev[i][j], host[i][j])
            n_rows += len(host[i][j])
    assert n_rows > 0

    def tracks_of(matches):
        T = tri.GlobalLineTriangulator(syn.default_triangulation_cfg())
        T.SetRanges(sc.ranges)
        T.InitArrays(sc.img_ids, sc.kvec, sc.qvec, sc.tvec, [sc.segs_of(i) for i in range(sc.n_images)])
        T.TriangulateAll(matches)
        T.ComputeLineTracks()
        return T.context().get_tracks()

    a, b = tracks_of(dev), tracks_of(host)
    for key in ("off", "image_ids", "line_ids"):
        assert np.array_equal(a[key], b[key])


def test_match_all_neighbors_writes_the_files(tmp_path):
    rng = np.random.default_rng(69)
    a, b, w = dc.overlapping_pair(rng, 20, 20)
    di = {0: a, 1: b}

    class Extractor(matching.DenseNaiveExtractor):
        def read_descinfo(self, folder, idx):
            return di[int(idx)]

    back = (w[2], w[3], w[0], w[1])

    class Both(matching.BaseDenseMatcher):
        def get_sample_thresh(self):
            return 0.5

        def get_warping_symmetric(self, img1, img2):
            return w  # (the two images are interchangeable here: identity warps)

    m = matching.DenseLineMatcher(Extractor(), Both(), Opts(), matching.BaseMatcherOptions(topk=0, n_neighbors=1))
    folder = m.match_all_neighbors(str(tmp_path), [0, 1], {0: [1], 1: [0]}, "unused")
    assert folder.endswith("dense_n1_top0")
    got = matching.limapio.read_matches(folder, 0)
    assert np.array_equal(got[1], matching.match_dense_pair_host(a, b, w, Opts(), 0.5)) and len(got[1]) > 0
    got = matching.limapio.read_matches(folder, 1)
    assert np.array_equal(got[0], matching.match_dense_pair_host(b, a, back, Opts(), 0.5))
