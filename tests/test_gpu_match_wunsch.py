"""The SOLD2 kind of limap_amd.matching on the device: lt_match_wunsch_scene against the host restatement
lt_fn_match_wunsch_pair_host, zero tolerance -- rows AND the FP32 line scores of the returned rows bit for bit -- at
the edges of the tiling, for every sample count and width, in the top-k and the mutual Needleman-Wunsch form; the
definition cases; rejections; files; the end-to-end path into the triangulator ("SOLD2").

Tile sizes of k_wunsch_topk: 4 lines per wave and per staged tile of the neighbour, 16 lines per workgroup; k_wunsch_nw
takes 16 candidates per pass of a line's lane group."""
import ctypes as C

import numpy as np
import pytest

import wunsch_cases as wc
from limap_amd import _capi, matching, synthetic as syn

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 3, 4, 5, 15, 16, 17, 33, 130]  # lines per image: around 4 (a tile), 16 (a workgroup), several workgroups


def _pairs_every_size_on_either_side(n):
    return [(a, (a + s) % n) for a in range(n) for s in (1, 3, 4, 7)]


def _check_scene(topk, descs, pairs, S=5, kc=10):
    """one batched call over all pairs == the restatement per pair (rows and score bits)"""
    neighbors = {}
    for a, b in pairs:
        neighbors.setdefault(a, []).append(b)
    out, sc = matching.match_scene({m: d for m, d in enumerate(descs)}, neighbors, "sold2", topk, return_scores=True,
                                   num_samples=S, top_k_candidates=kc)
    for a, b in pairs:
        hr, hs = matching.match_pair_host(descs[a], descs[b], "sold2", topk, return_scores=True, num_samples=S,
                                          top_k_candidates=kc)
        assert out[a][b].dtype == np.int32 and out[a][b].shape == hr.shape, (topk, S, kc, a, b)
        assert np.array_equal(out[a][b], hr), (topk, S, kc, a, b)
        assert np.array_equal(wc.bits(sc[a][b]), wc.bits(hs)), (topk, S, kc, a, b)
    return out


@pytest.mark.parametrize("topk", [1, 10, matching.MAX_TOPK])
def test_tiling_edges_topk(topk):
    rng = np.random.default_rng([41, topk])
    descs = [wc.rand_descinfo(rng, n) for n in SIZES]
    _check_scene(topk, descs, _pairs_every_size_on_either_side(len(SIZES)))


@pytest.mark.parametrize("kc", [1, 10])
def test_tiling_edges_mutual(kc):
    rng = np.random.default_rng([42, kc])
    descs = [wc.rand_descinfo(rng, n) for n in SIZES]
    out = _check_scene(0, descs, _pairs_every_size_on_either_side(len(SIZES)), kc=kc)
    assert sum(len(r) for v in out.values() for r in v.values()) > 0


@pytest.mark.parametrize("dim", [8, 128, 256])
@pytest.mark.parametrize("S", [2, 5, 8])
def test_sample_counts_and_widths(S, dim):
    rng = np.random.default_rng([43, S, dim])
    descs = [wc.rand_descinfo(rng, n, S, dim, prefix=False) for n in (0, 1, 17, 33)]
    pairs = [(a, b) for a in range(4) for b in range(4) if a != b]
    _check_scene(10, descs, pairs, S=S)
    _check_scene(0, descs, pairs, S=S)


def test_more_candidates_than_a_lane_group_pass():
    rng = np.random.default_rng(44)
    descs = [wc.rand_descinfo(rng, 37), wc.rand_descinfo(rng, 70)]
    _check_scene(0, descs, [(0, 1), (1, 0)], kc=matching.MAX_TOPK)
    _check_scene(0, descs, [(0, 1), (1, 0)], kc=17)


@pytest.mark.parametrize("name", wc.DEFINITION_CASES)
def test_definition_cases_on_the_device(name):
    a, b, S, topk, kc = wc.definition_case(name)
    _check_scene(topk, [a, b], [(0, 1), (1, 0)], S=S, kc=kc)
    _check_scene(0, [a, b], [(0, 1), (1, 0)], S=S, kc=kc)
    if name == "ties":
        rows, sc = matching.match_scene({0: a, 1: b}, {0: [1]}, "sold2", 10, return_scores=True)
        cols, s = rows[0][1][:, 1].reshape(-1, 10), sc[0][1].reshape(-1, 10)
        eq = s[:, :-1] == s[:, 1:]
        assert eq.any() and (cols[:, :-1][eq] < cols[:, 1:][eq]).all()


def test_batched_equals_per_pair_calls_torch_input_and_repeat():
    import torch
    rng = np.random.default_rng(45)
    descs = {m: wc.rand_descinfo(rng, n) for m, n in enumerate((40, 130, 31, 0))}
    nbs = {0: [1, 2, 3], 1: [0], 2: [1, 0], 3: [1]}
    on_gpu = {m: [torch.from_numpy(d[0]).cuda(), d[1]] for m, d in descs.items()}
    for topk in (10, 0):
        batched, bs = matching.match_scene(descs, nbs, "sold2", topk, return_scores=True)
        again, as_ = matching.match_scene(descs, nbs, "sold2", topk, return_scores=True)
        from_torch, ts = matching.match_scene(on_gpu, nbs, "sold2", topk, return_scores=True)
        permuted, ps = matching.match_scene(descs, {2: [0, 1], 3: [1], 1: [0], 0: [3, 2, 1]}, "sold2", topk,
                                            return_scores=True)
        m = matching.SOLD2Matcher(None, matching.BaseMatcherOptions(topk=topk))
        for a, v in nbs.items():
            for b in v:
                single = m.match_pair(descs[a], descs[b])
                for other, osc in ((again, as_), (from_torch, ts), (permuted, ps)):
                    assert np.array_equal(batched[a][b], other[a][b]), (topk, a, b)
                    assert np.array_equal(wc.bits(bs[a][b]), wc.bits(osc[a][b])), (topk, a, b)
                assert np.array_equal(batched[a][b], single), (topk, a, b)
    t, k = matching.timers(), matching.kernel_ms()
    assert (t >= 0).all() and t[1] > 0 and k[0] > 0 and k[1] > 0


def _scene_call(ctx, infos, dim, pair_off, pair_nb, topk=10, S=5, kc=10, n_desc=None):
    rows = [np.ascontiguousarray(np.asarray(d[0], np.float32).T) for d in infos]
    valids = [np.ascontiguousarray(d[1], np.uint8) for d in infos]
    line_off = np.zeros(len(infos) + 1, np.int64)
    line_off[1:] = np.cumsum([v.shape[0] for v in valids])
    desc_off = np.zeros(len(infos) + 1, np.int64)
    desc_off[1:] = np.cumsum([r.shape[0] for r in rows] if n_desc is None else n_desc)
    flat = np.ascontiguousarray(np.concatenate(rows, 0), np.float32)
    valid = np.ascontiguousarray(np.concatenate([v.reshape(-1) for v in valids]), np.uint8)
    cfg = _capi.LtMatchWunschConfig(topk, S, kc, 0, 0, 0)
    po, pn = _capi.i64(pair_off), _capi.i32(pair_nb)
    return ctx.L.lt_match_wunsch_scene(ctx.h, len(infos), _capi.ptr(line_off, C.c_int64), _capi.ptr(desc_off, C.c_int64),
                                       C.c_void_p(flat.ctypes.data), valid.ctypes.data_as(C.POINTER(C.c_uint8)), dim,
                                       _capi.ptr(po, C.c_int64), _capi.ptr(pn, C.c_int32), C.byref(cfg), None)


def test_rejected_before_any_launch():
    ctx = _capi.Context()
    rng = np.random.default_rng(46)
    ok = wc.rand_descinfo(rng, 4)

    def rejected(infos, dim=128, nb=(1,), **kw):
        rc = _scene_call(ctx, infos, dim, [0, len(nb), len(nb)], list(nb), **kw)
        msg = ctx.L.lt_last_error(ctx.h).decode()
        assert rc == -2 and msg.startswith("lt_match_wunsch_scene: "), (rc, msg)
        return msg

    for v in (np.nan, np.inf, -np.inf, 2.0 ** 58):
        bad = [ok[0].copy(), ok[1]]
        bad[0][77, 3] = v
        assert "not finite" in rejected([ok, bad])
    assert "negative" in rejected([ok, ok], topk=-1)
    assert "LT_MATCH_MAX_TOPK" in rejected([ok, ok], topk=matching.MAX_TOPK + 1)
    assert "top_k_candidates" in rejected([ok, ok], topk=0, kc=0)
    assert "top_k_candidates" in rejected([ok, ok], topk=0, kc=matching.MAX_TOPK + 1)
    for S in (1, 9):
        w = [np.ones((128, 4 * S), np.float32), np.ones((4, S), bool)]
        assert "num_samples" in rejected([w, w], S=S)
    for dim in (12, 264):
        w = [np.ones((dim, 20), np.float32), np.ones((4, 5), bool)]
        assert "width" in rejected([w, w], dim=dim)
    big = [np.zeros((8, 2 * 65536), np.float32), np.ones((65536, 2), bool)]
    small = [np.ones((8, 8), np.float32), np.ones((4, 2), bool)]
    assert "65535" in rejected([big, small], dim=8, S=2)
    assert "not num_samples times" in rejected([ok, ok], n_desc=[20, 19])
    none_valid = [ok[0], ok[1].copy()]
    none_valid[1][2, :] = False
    assert "no valid sample" in rejected([ok, none_valid])
    assert "not an image" in rejected([ok, ok], nb=(2,))
    # the Python layer
    with pytest.raises(ValueError, match="columns per line"):
        matching.match_scene({0: ok, 1: [ok[0][:, :19], ok[1]]}, {0: [1]}, "sold2", 10)
    with pytest.raises(ValueError, match="widths differ"):
        matching.match_scene({0: ok, 1: wc.rand_descinfo(rng, 4, 5, 64)}, {0: [1]}, "sold2", 10)
    import torch
    bad = torch.from_numpy(ok[0]).cuda()
    bad[5, 1] = float("nan")
    with pytest.raises(ValueError, match="not finite"):
        matching.match_scene({0: ok, 1: [bad, ok[1]]}, {0: [1]}, "sold2", 10)
    # the context still works
    assert _scene_call(ctx, [ok, ok], 128, [0, 1, 1], [1], topk=2) == 0
    assert _scene_call(ctx, [ok, ok], 128, [0, 1, 1], [1], topk=0) == 0
    ctx.close()


def test_match_all_neighbors_writes_the_files(tmp_path):
    sc = syn.make_scene(n_views=4, n_segs=30, n_neighbors=2, seed=6)
    di = syn.make_descriptors(sc, "sold2", seed=1)

    class Extractor:
        def read_descinfo(self, folder, idx):
            return di[int(idx)]

    for topk, tag in ((5, "sold2_n2_top5"), (0, "sold2_n2_top0")):
        m = matching.SOLD2Matcher(Extractor(), matching.BaseMatcherOptions(topk=topk, n_neighbors=2))
        folder = m.match_all_neighbors(str(tmp_path), [int(i) for i in sc.img_ids], sc.neighbors, "unused")
        assert folder.endswith(tag)
        for i in sc.img_ids:
            got = matching.limapio.read_matches(folder, int(i))
            assert sorted(got) == sorted(sc.neighbors[int(i)])
            for j, rows in got.items():
                assert np.array_equal(rows, matching.match_pair_host(di[int(i)], di[int(j)], "sold2", topk))


@pytest.mark.parametrize("topk", [10, 0])
def test_end_to_end_into_the_triangulator(topk):
    from limap_amd import triangulation as tri
    sc = syn.make_scene(n_views=10, n_segs=60, n_neighbors=4, seed=8)
    di = syn.make_descriptors(sc, "sold2", noise=0.02, seed=3)
    dev = matching.match_scene(di, sc.neighbors, "sold2", topk)
    host = {int(i): {int(j): matching.match_pair_host(di[int(i)], di[int(j)], "sold2", topk)
                     for j in sc.neighbors[int(i)]} for i in sc.img_ids}

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

    def gt_hits(matches):  # lines whose GT correspondence (where the neighbour sees the segment) is among the rows
        hit = tot = 0
        for k, i in enumerate(sc.img_ids):
            g1 = sc.gt_ids[sc.seg_off[k]:sc.seg_off[k + 1]]
            for j in sc.neighbors[int(i)]:
                kj = int(np.searchsorted(sc.img_ids, j))
                g2 = sc.gt_ids[sc.seg_off[kj]:sc.seg_off[kj + 1]]
                pairs = set(map(tuple, matches[int(i)][int(j)].tolist()))
                for l, g in enumerate(g1):
                    w = np.nonzero(g2 == g)[0] if g >= 0 else []
                    if len(w):
                        tot += 1
                        hit += (l, int(w[0])) in pairs
        return hit, tot

    hd, hh = gt_hits(dev), gt_hits(host)
    assert hd[1] > 0 and hd[0] > 0 and hd == hh
