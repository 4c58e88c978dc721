"""limap_amd.matching on the device: lt_match_scene against the host restatement lt_fn_match_pair_host, zero tolerance
-- rows AND the FP32 scores of the returned rows bit for bit -- on every golden and on random scenes that hit the
tiling edges; rejections; the end-to-end path into the triangulator.  A score that differs is a
finding about the accumulation order of the kernel, never a reason for a tolerance."""
import ctypes as C
import glob
import importlib.util
import os

import numpy as np
import pytest

from limap_amd import _capi, matching, synthetic as syn

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_match_golden", os.path.join(HERE, "golden", "make_match_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(gen.OUT, "*.npz")))

TILE = 128  # descriptor rows of image 1 per workgroup (4 waves x 32)
KEY = {"l2d2": "line_descriptors", "endpoints": "endpoints_desc"}


def _rand(rng, kind, m, dim):
    per = 2 if kind == "endpoints" else 1
    d = rng.standard_normal((m * per, dim)).astype(np.float32)
    return np.ascontiguousarray(d.T) if kind == "endpoints" else d


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_scene(kind, topk, descs, pairs):
    """one batched call over all pairs == the restatement per pair (rows and score bits)"""
    neighbors = {}
    for a, b in pairs:
        neighbors.setdefault(a, []).append(b)
    out, sc = matching.match_scene({m: d for m, d in enumerate(descs)}, neighbors, kind, topk, return_scores=True)
    for a, b in pairs:
        hr, hs = matching.match_pair_host(descs[a], descs[b], kind, topk, return_scores=True)
        assert out[a][b].dtype == np.int32 and np.array_equal(out[a][b], hr), (kind, topk, a, b)
        assert np.array_equal(_bits(sc[a][b]), _bits(hs)), (kind, topk, a, b)


@pytest.mark.parametrize("name", FIXTURES)
def test_goldens_device_equals_restatement(name):
    kind, topk, descs, pairs, _ = gen.load_fixture(os.path.join(gen.OUT, name + ".npz"))
    _check_scene(kind, topk, descs, pairs)


def test_fixture_list_is_complete():
    assert len(FIXTURES) == 10


@pytest.mark.parametrize("kind,dim", [("l2d2", 128), ("endpoints", 256)])
@pytest.mark.parametrize("topk", [1, 10, matching.MAX_TOPK])
def test_tiling_edges(kind, dim, topk):
    rng = np.random.default_rng([7, dim, topk])
    per = 2 if kind == "endpoints" else 1
    sizes = [0, 1, 63, 64, 65, TILE // per - 1, TILE // per, TILE // per + 1, 1000]
    descs = [_rand(rng, kind, m, dim) for m in sizes]
    n = len(sizes)
    pairs = [(a, (a + s) % n) for a in range(n) for s in (1, 3, 4, 8)]  # every size on either side, incl. M2 < topk
    _check_scene(kind, topk, descs, pairs)


@pytest.mark.parametrize("dim", [8, 64, 136, 256])
def test_other_widths_and_mutual(dim):
    rng = np.random.default_rng([9, dim])
    descs = [_rand(rng, "l2d2", m, dim) for m in (0, 1, 65, 129, 300)]
    pairs = [(a, b) for a in range(5) for b in range(5) if a != b]
    _check_scene("l2d2", 0, descs, pairs)
    _check_scene("l2d2", 7, descs, pairs)


def test_exact_ties_on_the_device():
    rng = np.random.default_rng(3)
    base = rng.standard_normal((40, 128)).astype(np.float32)
    d1 = rng.standard_normal((70, 128)).astype(np.float32)
    d2 = base[rng.integers(0, 40, 200)]  # every column has duplicates, across tiles and lanes
    _check_scene("l2d2", 10, [d1, d2], [(0, 1), (1, 0)])
    _check_scene("l2d2", 0, [d2, d2[::-1].copy()], [(0, 1)])
    rows = matching.match_scene({0: d1, 1: d2}, {0: [1]}, "l2d2", 10, return_scores=True)
    cols, sc = rows[0][0][1][:, 1].reshape(70, 10), rows[1][0][1].reshape(70, 10)
    eq = sc[:, :-1] == sc[:, 1:]
    assert eq.any() and (cols[:, :-1][eq] < cols[:, 1:][eq]).all()


def test_one_pair_and_two_thousand_pairs_in_one_call():
    rng = np.random.default_rng(11)
    descs = [_rand(rng, "l2d2", int(m), 128) for m in rng.integers(20, 90, 100)]
    pairs = [(a, (a + s) % 100) for a in range(100) for s in range(1, 21)]
    assert len(pairs) == 2000
    _check_scene("l2d2", 10, descs, pairs)
    _check_scene("l2d2", 10, descs, pairs[:1])


def test_batched_equals_per_pair_calls_and_torch_input():
    import torch
    rng = np.random.default_rng(12)
    for kind, dim, cls in (("l2d2", 128, matching.L2D2Matcher), ("endpoints", 256, matching.NNEndpointsMatcher)):
        descs = {m: _rand(rng, kind, s, dim) for m, s in enumerate((90, 130, 31))}
        nbs = {0: [1, 2], 1: [0], 2: [1, 0]}
        batched = matching.match_scene(descs, nbs, kind, 10)
        on_gpu = {m: {KEY[kind]: torch.from_numpy(d).cuda()} for m, d in descs.items()}
        from_torch = matching.match_scene(on_gpu, nbs, kind, 10)
        m10 = cls(None, matching.BaseMatcherOptions(topk=10))
        for a, v in nbs.items():
            for b in v:
                single = m10.match_pair({KEY[kind]: descs[a]}, {KEY[kind]: descs[b]})
                assert np.array_equal(batched[a][b], single) and np.array_equal(batched[a][b], from_torch[a][b])
    m0 = matching.L2D2Matcher(None, matching.BaseMatcherOptions(topk=0))
    a, b = _rand(rng, "l2d2", 80, 128), _rand(rng, "l2d2", 95, 128)
    assert np.array_equal(m0.match_pair({"line_descriptors": a}, {"line_descriptors": b}),
                          matching.match_pair_host(a, b, "l2d2", 0))


def test_every_kind_in_turn_on_one_context():
    """The three native matchers leave their result in one state of the context, which lt_match_get* read: every kind
    after another kind, mutual after top-k and back, with and without scores, each identical to its restatement.  17 and
    33 lines cross the 4- and 16-line tiles of SOLD2, the 16-line tile of the dense kind and the 32-row tile of the
    descriptor kinds."""
    import dense_cases as dc
    import wunsch_cases as wc
    rng = np.random.default_rng(23)
    ctx = matching._context(0)
    descs = {"l2d2": [_rand(rng, "l2d2", m, 8) for m in (17, 33)], "endpoints": [_rand(rng, "endpoints", m, 8) for m in (17, 33)],
             "sold2": [wc.rand_descinfo(rng, m, 5) for m in (17, 33)]}
    da, db, warps = dc.overlapping_pair(rng, 17, 33, dims=(1, 1))  # a warp of one texel
    opts = matching.BaseDenseLineMatcherOptions()

    def same(rows, scores, host):
        assert rows.dtype == np.int32 and len(rows) > 0 and rows.shape == host[0].shape and np.array_equal(rows, host[0])
        if scores is not None:
            assert np.array_equal(_bits(scores), _bits(host[1]))
        else:  # the call did not ask for scores (want_scores): LT_ERR_STATE
            buf = np.zeros(1, np.float32)
            assert ctx.L.lt_match_get_scores(ctx.h, buf.ctypes.data_as(C.POINTER(C.c_float))) == -4

    def sparse(kind, topk, scores):
        got = matching.match_scene(dict(enumerate(descs[kind])), {0: [1]}, kind, topk, return_scores=scores)
        host = matching.match_pair_host(descs[kind][0], descs[kind][1], kind, topk, return_scores=True)
        same(got[0][0][1] if scores else got[0][1], got[1][0][1] if scores else None, host)

    sparse("l2d2", 0, False)
    sparse("sold2", 10, True)
    got = matching.match_scene_dense({0: da, 1: db}, {0: [1]}, {(0, 1): warps}, opts, 0.5, return_scores=True)
    same(got[0][0][1], got[1][0][1], matching.match_dense_pair_host(da, db, warps, opts, 0.5, return_scores=True))
    sparse("endpoints", 10, False)
    sparse("sold2", 0, True)
    sparse("l2d2", 10, True)


def test_match_all_neighbors_writes_the_files(tmp_path):
    sc = syn.make_scene(n_views=4, n_segs=30, n_neighbors=2, seed=6)
    di = syn.make_descriptors(sc, "l2d2", seed=1)

    class Extractor:
        def read_descinfo(self, folder, idx):
            return di[int(idx)]

    m = matching.L2D2Matcher(Extractor(), matching.BaseMatcherOptions(topk=5, n_neighbors=2))
    folder = m.match_all_neighbors(str(tmp_path), [int(i) for i in sc.img_ids], sc.neighbors, "unused")
    assert folder.endswith("l2d2_n2_top5")
    for i in sc.img_ids:
        got = m.read_match(folder, int(i))
        assert sorted(got) == sorted(sc.neighbors[int(i)])
        for j, rows in got.items():
            assert np.array_equal(rows, matching.match_pair_host(di[int(i)], di[int(j)], "l2d2", 5))


def _scene_call(ctx, parts, dim, pair_off, pair_nb, kind, topk):
    desc_off = np.zeros(len(parts) + 1, np.int64)
    desc_off[1:] = np.cumsum([p.shape[0] for p in parts])
    flat = np.ascontiguousarray(np.concatenate(parts, 0), np.float32)
    cfg = _capi.LtMatchConfig(kind, topk, 0, 0)
    po, pn = _capi.i64(pair_off), _capi.i32(pair_nb)
    return ctx.L.lt_match_scene(ctx.h, len(parts), _capi.ptr(desc_off, C.c_int64), C.c_void_p(flat.ctypes.data), dim,
                                _capi.ptr(po, C.c_int64), _capi.ptr(pn, C.c_int32), C.byref(cfg), None)


def test_rejected_before_any_launch():
    ctx = _capi.Context()
    ok = np.ones((4, 128), np.float32)

    def rejected(parts, dim=128, kind=0, topk=10, nb=(1,)):
        rc = _scene_call(ctx, parts, dim, [0, len(nb), len(nb)], list(nb), kind, topk)
        msg = ctx.L.lt_last_error(ctx.h).decode()
        assert rc == -2 and msg.startswith("lt_match_scene: "), (rc, msg)
        return msg

    for v in (np.nan, np.inf, -np.inf, 2.0 ** 58):
        bad = ok.copy()
        bad[3, 77] = v
        assert "not finite" in rejected([ok, bad])
    assert "negative" in rejected([ok, ok], topk=-1)
    assert "LT_MATCH_MAX_TOPK" in rejected([ok, ok], topk=matching.MAX_TOPK + 1)
    assert "width" in rejected([np.ones((4, 12), np.float32)] * 2, dim=12)
    assert "width" in rejected([np.ones((4, 264), np.float32)] * 2, dim=264)
    assert "odd number of endpoints" in rejected([np.ones((3, 128), np.float32), ok], kind=1)
    assert "mutual" in rejected([ok, ok], kind=1, topk=0)
    assert "65535" in rejected([np.zeros((65536, 8), np.float32), np.ones((4, 8), np.float32)], dim=8)
    assert "not an image" in rejected([ok, ok], nb=(2,))
    # the Python layer: widths that differ across the call, non-finite values in a tensor on the device
    with pytest.raises(ValueError, match="widths differ"):
        matching.match_scene({0: ok, 1: np.ones((4, 64), np.float32)}, {0: [1]}, "l2d2", 10)
    import torch
    bad = torch.ones(4, 128, device="cuda")
    bad[1, 5] = float("nan")
    with pytest.raises(ValueError, match="not finite"):
        matching.match_scene({0: torch.ones(4, 128, device="cuda"), 1: bad}, {0: [1]}, "l2d2", 10)
    # the context still works
    assert _scene_call(ctx, [ok, ok], 128, [0, 1, 1], [1], 0, 2) == 0
    ctx.close()


@pytest.mark.parametrize("kind", ["l2d2", "endpoints"])
def test_end_to_end_into_the_triangulator(kind):
    from limap_amd import triangulation as tri
    sc = syn.make_scene(n_views=10, n_segs=60, n_neighbors=4, seed=8)
    di = syn.make_descriptors(sc, kind, noise=0.02, seed=3)
    dev = matching.match_scene(di, sc.neighbors, kind, 10)
    host = {int(i): {int(j): matching.match_pair_host(di[int(i)], di[int(j)], kind, 10) for j in sc.neighbors[int(i)]}
            for i in sc.img_ids}

    def tracks_of(matches):
        T = tri.GlobalLineTriangulator(syn.default_triangulation_cfg())
        T.SetRanges(sc.ranges)
        T.InitArrays(sc.img_ids, sc.kvec, sc.qvec, sc.tvec, [sc.segs_of(i) for i in range(sc.n_images)])
        T.TriangulateAll(matches)
        T.ComputeLineTracks()
        return T.context().get_tracks()

    a, b = tracks_of(dev), tracks_of(host)
    assert len(a["off"]) > 1
    for key in ("off", "image_ids", "line_ids"):
        assert np.array_equal(a[key], b[key])

    def gt_share(matches):  # share of lines whose GT correspondence (where the neighbour sees it) is among the rows
        hit = tot = 0
        for k, i in enumerate(sc.img_ids):
            g1 = sc.gt_ids[sc.seg_off[k]:sc.seg_off[k + 1]]
            for j in sc.neighbors[int(i)]:
                kj = int(np.searchsorted(sc.img_ids, j))
                g2 = sc.gt_ids[sc.seg_off[kj]:sc.seg_off[kj + 1]]
                rows = matches[int(i)][int(j)]
                pairs = set(map(tuple, rows.tolist()))
                for l, g in enumerate(g1):
                    w = np.nonzero(g2 == g)[0] if g >= 0 else []
                    if len(w):
                        tot += 1
                        hit += (l, int(w[0])) in pairs
        return hit, tot

    hd, hh = gt_share(dev), gt_share(host)
    assert hd[1] > 0 and hd[0] >= hh[0] and hd[1] == hh[1]
