"""lt_fit_segs (estimate_seg3d_from_depth over every segment on the GPU) against tests/fit_oracle.py, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import fit_oracle as fo
from fit_scenes import cams_of, compare, edge_segments, oracle_scene

pytestmark = pytest.mark.gpu

H, W = 120, 160


def _scene(n_views=3, n_segs=14, h=H, w=W, seed=2, dtype=np.float32, noise=0.003, holes=0.05, outliers=0.05):
    from limap_amd import synthetic as syn
    sc = syn.resize_scene(syn.make_scene(n_views=n_views, n_segs=n_segs, n_neighbors=2, seed=seed), h, w)
    depths = syn.render_depths(syn.make_scene(n_views=n_views, n_segs=n_segs, n_neighbors=2, seed=seed), h, w, noise,
                               holes, outliers, dtype, seed)
    all_2d = {int(i): np.concatenate([sc.segs_of(n), edge_segments(h, w)], 0) for n, i in enumerate(sc.img_ids)}
    return sc, all_2d, depths


def _run(sc, all_2d, depths, **kw):
    from limap_amd import fitting, synthetic as syn
    return fitting.fit_3d_segs_arrays(all_2d, syn.imagecols_of(sc), depths, **kw)


def _check(sc, all_2d, depths, res, seed=0, fitting_config=None):
    fc = dict(fitting_config or {})
    ref = oracle_scene(all_2d, sc, {i: np.asarray(d) for i, d in depths.items()}, ransac_th=fc.get("ransac_th", 0.75),
                       min_pct=fc.get("min_percentage_inliers", 0.6), var2d=fc.get("var2d", 5.0), seed=seed)
    arrs, info, _ = res
    n_ok = 0
    for i in ref:
        for l, r in enumerate(ref[i]):
            compare(arrs[i][l], info[i]["status"][l], info[i]["stats"][l], r, f"image {i} line {l}")
            n_ok += r["status"] == 0
    assert n_ok > 0
    return ref


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_scene_against_oracle(dtype):
    sc, all_2d, depths = _scene(dtype=dtype)
    ref = _check(sc, all_2d, depths, _run(sc, all_2d, depths))
    statuses = {r["status"] for i in ref for r in ref[i]}
    assert {0, 1} <= statuses


def test_nan_depths_and_few_pixels():
    sc, all_2d, depths = _scene(n_views=2, n_segs=6)
    i0 = int(sc.img_ids[0])
    d = depths[i0].copy()
    d[20, :] = np.nan  # the horizontal edge segment reads a NaN row: the median is NaN
    d[:, 30] = np.inf  # the vertical one keeps no pixel
    depths[i0] = d
    all_2d[i0] = np.concatenate([all_2d[i0], [[40.0, 50.0, 44.0, 50.0], [60.0, 61.0, 60.0, 70.0]]], 0)
    _check(sc, all_2d, depths, _run(sc, all_2d, depths))


def test_long_segments_use_the_scratch_path():
    h, w = 300, 400
    sc, all_2d, depths = _scene(n_views=2, n_segs=4, h=h, w=w, holes=0.0)
    arrs, info, tm = _run(sc, all_2d, depths)
    assert max(int(s[0]) for i in info for s in info[i]["stats"]) > 256
    _check(sc, all_2d, depths, (arrs, info, tm))


def test_strided_and_torch_maps_equal_host_arrays():
    import torch
    sc, all_2d, depths = _scene(n_views=2, n_segs=8, dtype=np.float64)
    base = _run(sc, all_2d, depths)
    strided = {}
    for i, d in depths.items():
        big = np.full((d.shape[0], d.shape[1] + 13), -7.0)
        big[:, :d.shape[1]] = d
        strided[i] = big[:, :d.shape[1]]
    assert not strided[int(sc.img_ids[0])].flags["C_CONTIGUOUS"]
    tdev = {i: torch.from_numpy(np.ascontiguousarray(d)).to("cuda") for i, d in depths.items()}
    for other in (_run(sc, all_2d, strided), _run(sc, all_2d, tdev)):
        for i in base[0]:
            assert np.array_equal(base[0][i].view(np.uint64), other[0][i].view(np.uint64))
            assert np.array_equal(base[1][i]["stats"], other[1][i]["stats"])


def _same(a, b):
    for i in a[0]:
        assert np.array_equal(a[0][i].view(np.uint64), b[0][i].view(np.uint64)), f"image {i}"
        assert np.array_equal(a[1][i]["stats"], b[1][i]["stats"]) and np.array_equal(a[1][i]["status"], b[1][i]["status"])


def test_torch_device_maps_are_ordered_after_torch_work():
    """GPU tensors read in place or converted on the device (a column slice with row stride > w, a transposed layout,
    an integer map, a map written behind a long queue of torch work) give the host arrays' results"""
    import torch
    sc, all_2d, depths = _scene(n_views=2, n_segs=8, dtype=np.float64)
    base = _run(sc, all_2d, depths)
    dev = {i: torch.from_numpy(d).to("cuda") for i, d in depths.items()}
    wide = {}
    for i, d in dev.items():
        big = torch.full((d.shape[0], d.shape[1] + 13), -7.0, dtype=d.dtype, device="cuda")
        big[:, :d.shape[1]] = d
        wide[i] = big[:, :d.shape[1]]
    i0 = int(sc.img_ids[0])
    assert wide[i0].stride(0) == wide[i0].shape[1] + 13 and wide[i0].stride(1) == 1
    _same(base, _run(sc, all_2d, wide))
    transposed = {i: d.t().contiguous().t() for i, d in dev.items()}
    assert transposed[i0].stride(1) != 1
    _same(base, _run(sc, all_2d, transposed))
    a = torch.randn(2048, 2048, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    late = {}
    for i, d in dev.items():
        m = torch.full_like(d, -1.0)
        for _ in range(8):  # keeps torch's stream busy for a while before the map is written
            a = (a @ a) * (1.0 / 2048.0)
        m.copy_(d)
        late[i] = m
    _same(base, _run(sc, all_2d, late))
    ints = {i: np.round(np.where(np.isfinite(d), d, 0.0) * 1000.0).astype(np.int32) for i, d in depths.items()}
    _same(_run(sc, all_2d, ints), _run(sc, all_2d, {i: torch.from_numpy(v).to("cuda") for i, v in ints.items()}))


def test_map_on_another_device_is_refused():
    import torch
    from limap_amd import fitting, synthetic as syn
    sc, all_2d, depths = _scene(n_views=1, n_segs=4)
    dev = {i: torch.from_numpy(d).to("cuda:0") for i, d in depths.items()}
    with pytest.raises(ValueError, match="cuda:1"):
        fitting.fit_3d_segs_arrays(all_2d, syn.imagecols_of(sc), dev, device=1)


def test_scratch_overflow_reruns_with_the_counted_size(monkeypatch):
    h, w = 300, 400
    sc, all_2d, depths = _scene(n_views=2, n_segs=4, h=h, w=w, holes=0.0)
    base = _run(sc, all_2d, depths)
    assert base[2]["attempts"] == 1
    monkeypatch.setenv("LT_TEST_FIT_SCRATCH_CAP", "1")
    small = _run(sc, all_2d, depths)
    assert small[2]["attempts"] == 2
    _same(base, small)


def test_chunks_read_every_map_once():
    from limap_amd import fitting, synthetic as syn
    sc, all_2d, depths = _scene(n_views=4, n_segs=5)
    reads = {}

    class Reader:
        def __init__(self, i):
            self.i = i

        def read_depth(self, img_hw=None):
            reads[self.i] = reads.get(self.i, 0) + 1
            return depths[self.i]

    base = _run(sc, all_2d, depths)
    budget = 2 * depths[int(sc.img_ids[0])].nbytes - 1  # two maps overflow a chunk
    got = fitting.fit_3d_segs_arrays(all_2d, syn.imagecols_of(sc), {i: Reader(i) for i in depths},
                                     max_chunk_bytes=budget)
    assert got[2]["chunks"] == 4 and all(v == 1 for v in reads.values()) and len(reads) == 4
    _same(base, got)


def test_chunks_unsorted_ids_empty_images_and_seed():
    from limap_amd import base, fitting
    sc, all_2d, depths = _scene(n_views=4, n_segs=8)
    ids = [int(i) for i in sc.img_ids]
    new_ids = [40, 7, 23, 11]
    m = dict(zip(ids, new_ids))
    ic = base.ImageCollection({m[i]: base.CameraView(sc.kvec[n], sc.qvec[n], sc.tvec[n]) for n, i in enumerate(ids)})
    a2 = {m[i]: all_2d[i] for i in reversed(ids)}
    a2[23] = np.zeros((0, 4))  # an image without segments
    dd = {m[i]: depths[i] for i in ids}
    one = fitting.fit_3d_segs_arrays(a2, ic, dd)
    chunked = fitting.fit_3d_segs_arrays(a2, ic, dd, max_chunk_bytes=1)
    assert chunked[2]["chunks"] == 4
    for i in new_ids:
        assert np.array_equal(one[0][i].view(np.uint64), chunked[0][i].view(np.uint64))
        assert np.array_equal(one[1][i]["stats"], chunked[1][i]["stats"])
    assert one[0][23].shape == (0, 2, 3)
    # the oracle with the new ids (the generator is keyed by image id)
    cams = {m[i]: (sc.kvec[n], sc.qvec[n], sc.tvec[n]) for n, i in enumerate(ids)}
    ref = fo.fit_scene(a2, cams, dd, fo.Options())
    for i in ref:
        for l, r in enumerate(ref[i]):
            compare(one[0][i][l], one[1][i]["status"][l], one[1][i]["stats"][l], r, f"image {i} line {l}")
    s7 = fitting.fit_3d_segs_arrays(a2, ic, dd, seed=7)
    assert any(not np.array_equal(s7[0][i], one[0][i]) for i in new_ids)
    ref7 = fo.fit_scene({7: a2[7]}, {7: cams[7]}, {7: dd[7]}, fo.Options(random_seed_=7))
    for l, r in enumerate(ref7[7]):
        compare(s7[0][7][l], s7[1][7]["status"][l], s7[1][7]["stats"][l], r, f"seed 7 line {l}")


def test_add_halfpix_context_reads_unshifted_segments():
    from limap_amd import _capi, fitting
    sc, all_2d, depths = _scene(n_views=2, n_segs=6, dtype=np.float64)
    ids = [int(i) for i in sc.img_ids]
    segs = np.concatenate([all_2d[i] for i in ids], 0)
    off = np.zeros(len(ids) + 1, np.int64)
    off[1:] = np.cumsum([len(all_2d[i]) for i in ids])
    ctx = _capi.Context(cfg_dict={"add_halfpix": True})
    ctx.init(ids, sc.kvec, sc.qvec, sc.tvec, off, segs)
    maps = [fitting._map_of(depths[i])[0] for i in ids]
    arr = (_capi.LtDepthMap * len(maps))(*maps)
    cfg = fitting._config()
    G = len(segs)
    seg = np.zeros((G, 6)); st = np.zeros(G, np.int32); stats = np.zeros((G, 5), np.int32)
    p = _capi.ptr
    ctx.chk(ctx.L.lt_fit_segs(ctx.h, 0, len(ids), arr, C.byref(cfg), p(seg, C.c_double), p(st, C.c_int32),
                              p(stats, C.c_int32)))
    ref = oracle_scene(all_2d, sc, depths)
    for n, i in enumerate(ids):
        for l, r in enumerate(ref[i]):
            g = off[n] + l
            compare(seg[g].reshape(2, 3), st[g], stats[g], r, f"image {i} line {l}")


def test_fit_3d_segs_structure_and_single_segment():
    from limap_amd import fitting, synthetic as syn
    sc, all_2d, depths = _scene(n_views=2, n_segs=5)
    out = fitting.fit_3d_segs(all_2d, syn.imagecols_of(sc), depths, dict(ransac_th=0.75, min_percentage_inliers=0.6,
                                                                         var2d=5.0, n_jobs=4))
    arrs = _run(sc, all_2d, depths)[0]
    for i in arrs:
        assert len(out[i]) == len(arrs[i])
        for (s, e), a in zip(out[i], arrs[i]):
            assert s.shape == (3,) and s.dtype == np.float64 and np.array_equal(s, a[0]) and np.array_equal(e, a[1])
    i0 = int(sc.img_ids[0])
    view = syn.imagecols_of(sc).camview(i0)
    ref = fo.fit_segment(all_2d[i0][0], depths[i0], *cams_of(sc)[i0], 0, 0, fo.Options())
    got = fitting.estimate_seg3d_from_depth(all_2d[i0][0], depths[i0], view)
    if ref["status"] == 0:
        assert np.array_equal(got[0], ref["seg"][0]) and np.array_equal(got[1], ref["seg"][1])
    else:
        assert got is None
