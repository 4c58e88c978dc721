"""CPU checks of the scan fitter's contract: tests/fit_scan_oracle.py against NumPy's norm and linspace,
torch's grid_sample sequence of hloc's interpolate_scan, and the reference's front-half arithmetic; the Python argument
errors that precede any device work; tracks_from_fit."""
import os
import re

import numpy as np
import pytest

import fit_oracle as fo
import fit_scan_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits_equal(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- sample count ---------------------------------------------------------------------------------------------------
def test_sample_count_equals_numpy_on_random_segments():
    rng = np.random.default_rng(0)
    segs = np.concatenate([rng.uniform(-300, 300, (50_000, 4)), rng.uniform(-2.0**20, 2.0**20, (50_000, 4))])
    ref = (np.linalg.norm(segs[:, 2:4] - segs[:, 0:2], axis=1) * 2).astype(np.int64)
    got = np.array([so.sample_count(s) for s in segs])
    assert np.array_equal(got, ref)


def _near_integer_segments(n_want=30, seed=1):
    """segments whose 2 |d| lies within an ulp of an integer and whose count the FMA and the plain norm disagree on"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(400_000):
        k = int(rng.integers(2, 4000))
        dx = float(rng.uniform(0, k / 2))
        dy = float(np.sqrt((k / 2) ** 2 - dx * dx))
        for ddy in (dy, np.nextafter(dy, 0), np.nextafter(dy, np.inf)):
            fmaf = int(np.sqrt(so.fma(ddy, ddy, dx * dx)) * 2.0)
            plain = int(np.sqrt(dx * dx + ddy * ddy) * 2.0)
            if fmaf != plain:
                out.append([1.0, 2.0, 1.0 + dx, 2.0 + ddy] if (1.0 + dx) - 1.0 == dx and (2.0 + ddy) - 2.0 == ddy
                           else [0.0, 0.0, dx, ddy])
        if len(out) >= n_want:
            break
    return np.array(out)


def test_sample_count_takes_the_fma_norm_numpy_takes():
    segs = _near_integer_segments()
    assert len(segs) >= 10, "no segment separates the FMA norm from the plain one"
    for s in segs:
        d = s[2:4] - s[0:2]
        numpy_form = int(np.linalg.norm(d) * 2)
        plain = int(np.sqrt(d[0] * d[0] + d[1] * d[1]) * 2.0)
        assert so.sample_count(s) == numpy_form, (
            f"segment {s.tolist()}: NumPy's norm gives {numpy_form}, the FMA form {so.sample_count(s)}, the plain form "
            f"{plain}: this host's NumPy does not evaluate the norm as sqrt(fma(dy, dy, dx * dx))")


# ---- linspace -------------------------------------------------------------------------------------------------------
def _linspace_cases():
    rng = np.random.default_rng(3)
    cases = [s for s in rng.uniform(-200, 200, (1500, 4))]
    cases += [np.array(c, float) for c in (
        [3.0, 4.0, 3.0, 90.0], [3.0, 90.0, 3.0, 4.0],          # vertical, both directions
        [2.5, 7.0, 80.25, 7.0], [80.25, 7.0, 2.5, 7.0],        # horizontal
        [1.0, 1.0, 1.0, 1.0], [0.0, 0.0, 0.3, 0.1],            # num 0
        [0.0, 0.0, 0.6, 0.0], [5.0, 5.0, 5.7, 5.2],            # num 1
        [0.0, 0.0, 1.0, 0.0], [4.0, 4.0, 4.8, 4.7],            # num 2
        [-20.0, -30.0, 40.5, 60.25], [60.25, 40.5, -20.0, -30.0],  # negative and reversed
        [1e-300, 5.0, 2e-300, 90.0],                           # a step that underflows to 0
    )]
    cases += [np.array([x, y, x + dx, y + dy]) for x, y, dx, dy in rng.integers(-50, 150, (300, 4)).astype(float)]
    return cases


def test_samples_equal_numpy_linspace_bit_for_bit():
    seen = set()
    for s in _linspace_cases():
        num = so.sample_count(s)
        ref = np.linspace(s[0:2], s[2:4], num)
        px, py = so.samples(s, num, np.arange(num))
        assert _bits_equal(px, ref[:, 0]) and _bits_equal(py, ref[:, 1]), s.tolist()
        seen.add(min(num, 3))
    assert seen == {0, 1, 2, 3}


def test_the_walk_keeps_exactly_the_filtered_samples():
    """the conservative index range loses no sample inside the image, also for shallow crossings of an edge and far
    away starts"""
    rng = np.random.default_rng(4)
    h, w = 37, 53
    segs = list(rng.uniform(-80, 130, (800, 4)))
    segs += [np.array([-500.0, y, 600.0, y + rng.uniform(-0.2, 0.2)]) for y in rng.uniform(-1, h, 150)]
    segs += [np.array([x, -400.0, x + rng.uniform(-1e-9, 1e-9), 500.0]) for x in rng.uniform(-1, w, 150)]
    segs += [np.array([0.0, 0.0, w - 1.0, h - 1.0]), np.array([1.0, 1.0, w - 2.0, 1.0]), np.array([-3e4, 5.0, 3e4, 6.0])]
    for s in segs:
        num = so.sample_count(s)
        px, py = so.samples(s, num, np.arange(num))
        keep = (0 < px) & (0 < py) & (px < w - 1) & (py < h - 1)
        n2, kx, ky = so.kept_samples(s, h, w)
        assert n2 == num and _bits_equal(kx, px[keep]) and _bits_equal(ky, py[keep]), s.tolist()
        lo, hi = so.walk(s, num, h, w)
        assert hi - lo + 1 <= 2 * np.hypot(h, w) + 8


def test_the_walk_of_a_huge_segment_stays_bounded():
    s = np.array([-(2.0**28), -(2.0**28) + 3.0, 2.0**28, 2.0**28 - 7.0])
    num = so.sample_count(s)
    assert num > 2**30
    lo, hi = so.walk(s, num, 768, 1024)
    assert 0 < hi - lo + 1 <= 2 * np.hypot(768, 1024) + 8


# ---- interpolate_scan -----------------------------------------------------------------------------------------------
def _scan(rng, H, W, nan=0.1, inf=0.02):
    scan = rng.normal(size=(H, W, 3)) * 10.0
    scan[rng.uniform(size=(H, W)) < nan] = np.nan
    scan[rng.uniform(size=(H, W)) < nan / 2, 2] = np.nan  # a hole in one channel only
    scan[rng.uniform(size=(H, W)) < inf, 1] = np.inf
    scan[rng.uniform(size=(H, W)) < inf / 2, 0] = -np.inf
    return scan


def _same_values(a, b):
    eq = (np.asarray(a).view(np.uint64) == np.asarray(b).view(np.uint64)) | (np.isnan(a) & np.isnan(b))
    return bool(eq.all())


@pytest.mark.parametrize("case", ["random", "half_integer", "integer", "last_row_col", "scan_larger"])
def test_interpolation_equals_torch_grid_sample(case):
    rng = np.random.default_rng(["random", "half_integer", "integer", "last_row_col", "scan_larger"].index(case))
    H, W = 41, 57
    if case == "scan_larger":
        H, W = 97, 131
    scan = _scan(rng, H, W)
    n = 2000
    if case == "random":
        kp = np.stack([rng.uniform(1e-3, W - 1 - 1e-3, n), rng.uniform(1e-3, H - 1 - 1e-3, n)], 1)
    elif case == "half_integer":  # nearest rounds these half to even
        kp = np.stack([rng.integers(1, W - 2, n) + 0.5, rng.integers(1, H - 2, n) + 0.5], 1)
    elif case == "integer":  # the round trip can bring x back as x - 1 ulp
        kp = np.stack([rng.integers(1, W - 1, n), rng.integers(1, H - 1, n)], 1).astype(np.float64)
    elif case == "last_row_col":
        kp = np.stack([W - 1 - rng.uniform(0, 0.6, n) * rng.integers(0, 2, n), H - 1 - rng.uniform(0, 0.6, n)], 1)
        kp = np.minimum(kp, [np.nextafter(W - 1, 0), np.nextafter(H - 1, 0)])
    else:  # a 50 x 60 image's samples read from the larger scan: normalised by the scan's size
        kp = np.stack([rng.uniform(0.01, 59 - 0.01, n), rng.uniform(0.01, 49 - 0.01, n)], 1)
    v, valid, oor = so.interpolate(scan, kp[:, 0], kp[:, 1])
    assert not oor
    rv, rvalid = so.interpolate_scan_torch(scan, kp)
    assert _same_values(v, rv), f"{(~((v.view(np.uint64) == rv.view(np.uint64)) | (np.isnan(v) & np.isnan(rv)))).sum()} values differ"
    assert np.array_equal(valid, rvalid)
    assert 0 < valid.sum() < n


def test_integer_samples_do_come_back_below_the_integer():
    """the round trip is part of the contract: some integer x unnormalise to x - 1 ulp"""
    W = 1024
    x = np.arange(1, W - 1, dtype=np.float64)
    u = (((x / (W - 1)) * 2.0 - 1.0 + 1.0) / 2.0) * (W - 1)
    assert (u < x).any() and (np.floor(u) != x).any()


def test_out_of_range_samples():
    rng = np.random.default_rng(9)
    scan = _scan(rng, 30, 40)
    _, _, oor = so.interpolate(scan, np.array([5.0, 45.0]), np.array([5.0, 5.0]))  # a 50-wide image on a 40-wide scan
    assert oor
    with pytest.raises(AssertionError):
        so.interpolate_scan_torch(scan, np.array([[5.0, 5.0], [45.0, 5.0]]))
    x = 1e-20  # x / (W - 1) * 2 - 1 rounds to -1
    _, _, oor = so.interpolate(scan, np.array([x]), np.array([5.0]))
    assert oor


def test_bilinear_sum_is_the_fma_chain():
    """probe: values on which the FMA chain, the plain sum and the other summation orders differ; torch must give the
    chain (else skip, naming the form found)"""
    import torch
    rng = np.random.default_rng(11)
    H, W = 2, 2
    found = []
    for _ in range(4000):
        scan = rng.normal(size=(H, W, 3)) * rng.choice([1.0, 1e3, 1e-3])
        x, y = rng.uniform(0.01, 0.99, 2)
        v, _, _ = so.interpolate(scan, np.array([x]), np.array([y]))
        gx, gy = (x / (W - 1)) * 2.0 - 1.0, (y / (H - 1)) * 2.0 - 1.0
        ux, uy = ((gx + 1.0) / 2.0) * (W - 1), ((gy + 1.0) / 2.0) * (H - 1)
        wx, wy = ux - np.floor(ux), uy - np.floor(uy)
        ex, ey = 1.0 - wx, 1.0 - wy
        nw, ne, sw, se = ey * ex, ey * wx, wy * ex, wy * wx
        a, b, c, d = scan[0, 0], scan[0, 1], scan[1, 0], scan[1, 1]
        plain = ((a * nw + b * ne) + c * sw) + d * se
        if not _bits_equal(plain, v[0]):
            found.append((scan, x, y, v[0], plain))
        if len(found) >= 50:
            break
    assert len(found) >= 50
    n_chain = n_plain = 0
    for scan, x, y, chain, plain in found:
        t = torch.from_numpy(scan).permute(2, 0, 1)[None]
        g = torch.from_numpy(np.array([[(x / (W - 1)) * 2 - 1, (y / (H - 1)) * 2 - 1]]))[None, None]
        r = torch.nn.functional.grid_sample(t, g, align_corners=True, mode="bilinear")[0, :, 0, 0].numpy()
        n_chain += _bits_equal(r, chain)
        n_plain += _bits_equal(r, plain)
    if n_chain != len(found):
        pytest.skip(f"this host's torch does not sum bilinear weights by the FMA chain: {n_chain} of {len(found)} probes "
                    f"match the chain, {n_plain} the plain left-to-right multiply-add")


# ---- the front half against the reference's arithmetic -------------------------------------------------------------
def _rigid(rng):
    from limap_amd import synthetic as syn
    q = rng.normal(size=4)
    T = np.eye(4)
    T[:3, :3] = syn.quat_to_rot(q / np.linalg.norm(q))
    T[:3, 3] = rng.normal(size=3) * 5
    return T


@pytest.mark.parametrize("scan_size", ["image", "larger"])
@pytest.mark.parametrize("transform", ["camera", "inloc"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_front_half_against_the_reference_formula(transform, dtype, scan_size):
    from limap_amd import base, synthetic as syn
    rng = np.random.default_rng(5)
    h, w = 60, 80
    sc = syn.make_scene(n_views=2, n_segs=30, n_neighbors=1, seed=5)
    sh, sw = (h, w) if scan_size == "image" else (h + 15, w + 25)  # samples are normalised by the scan's size
    scans = syn.render_scans(sc, sh, sw, noise=0.002, hole_frac=0.1, dtype=np.float64, seed=5)
    scs = syn.resize_scene(sc, h, w)
    i0 = int(sc.img_ids[0])
    scan = scans[i0]
    scan[3:9, 10:30, 1] = np.nan
    scan[20, :, 2] = np.inf
    scan = scan.astype(dtype)
    view = base.CameraView(scs.kvec[0], scs.qvec[0], scs.tvec[0], hw=(h, w))
    Tr = _rigid(rng) if transform == "inloc" else None
    segs = list(scs.segs_of(0)) + list(rng.uniform(-20, 100, (40, 4))) + [np.array([2.0, 20.0, 70.0, 20.0]),
                                                                          np.array([30.5, 1.5, 30.5, 50.5])]
    n_cmp = 0
    for s in segs:
        # the reference's grid_sample refuses float32 scans; float32 is widened to double exactly
        ref = so.ref_front_half_scan(s, scan.astype(np.float64), h, w, view.R(), view.T(), Tr, 5.0, 0.75)
        got = so.front_half_scan(s, scan, (h, w), view._qvec_given, view.tvec, Tr, 5.0, 0.75)
        assert got["num"] == ref["num"] and not got["oor"]
        assert _bits_equal(got["px"], ref["px"]) and _bits_equal(got["py"], ref["py"])
        assert _same_values(got["points3d"], ref["points3d"]) and _bits_equal(got["ray"], ref["ray"])
        if ref["median"] is None:
            assert got["points"] is None
            continue
        n_cmp += 1
        assert np.float64(got["median"]).tobytes() == np.float64(ref["median"]).tobytes()
        assert np.float64(0.75 * got["unc"]).tobytes() == np.float64(ref["th"]).tobytes()
        fin = np.isfinite(ref["points"]).all(1)
        scale = np.maximum(1.0, np.linalg.norm(ref["points"][fin], axis=1))[:, None]
        assert np.all(np.abs(got["points"][fin] - ref["points"][fin]) <= 1e-14 * scale * 8)
        assert np.array_equal(np.isfinite(got["points"]), np.isfinite(ref["points"]))
    assert n_cmp > 15


def test_render_scans_are_the_camera_frame_points_of_the_depths():
    from limap_amd import synthetic as syn
    sc = syn.make_scene(n_views=2, n_segs=5, n_neighbors=1, seed=1)
    d = syn.render_depths(sc, 30, 40, dtype=np.float64)
    s = syn.render_scans(sc, 30, 40, hole_frac=0.1, dtype=np.float32)
    i = int(sc.img_ids[1])
    assert s[i].shape == (30, 40, 3) and s[i].dtype == np.float32
    hole = np.isnan(s[i]).any(2)
    assert 0 < hole.mean() < 0.2 and np.isnan(s[i][hole]).all()
    assert np.allclose(s[i][~hole, 2], d[i][~hole], rtol=1e-6)


# ---- Python surface -------------------------------------------------------------------------------------------------
def test_header_and_library_symbols():
    text = open(os.path.join(ROOT, "include", "limap_amd.h")).read()
    for sig in (r"int lt_fit_scans\(lt_ctx \*ctx, int img_begin, int n_maps, const lt_scan_map \*maps, "
                r"const double \*scan_poses,", r"typedef struct lt_scan_map", r"#define LT_FIT_SCAN_OUT_OF_RANGE 3"):
        assert re.search(sig, text), sig
    from limap_amd import _capi, fitting
    L = _capi.load_library()
    assert hasattr(L, "lt_fit_scans") and "lt_fit_scans" in _capi.EXPORTED_SYMBOLS
    assert fitting.STATUS_SCAN_OUT_OF_RANGE == so.STATUS_OUT_OF_RANGE == 3
    assert [f[0] for f in _capi.LtScanMap._fields_] == ["ptr", "h", "w", "row_stride", "pix_stride", "chan_stride",
                                                        "img_h", "img_w", "dtype", "on_device"]


def test_argument_errors_before_any_context(monkeypatch):
    from limap_amd import _capi, base, fitting

    def no_context(*a, **k):
        raise AssertionError("a context was created before the arguments were checked")

    monkeypatch.setattr(_capi, "Context", no_context)
    view = base.CameraView([100.0, 100.0, 50.0, 40.0], [1.0, 0, 0, 0], [0.0, 0, 0], hw=(80, 100))
    ic = base.ImageCollection({3: view})
    segs = {3: np.array([[1.0, 2.0, 30.0, 20.0]])}
    good = np.ones((80, 100, 3))
    for bad in (np.ones((80, 100), np.float64), np.ones((80, 100, 2)), np.ones((80, 100, 3), np.float16),
                np.ones((80, 100, 3), np.int32), np.ones((1, 100, 3)), np.ones((80, 1, 3))):
        with pytest.raises(ValueError):
            fitting.fit_3d_segs_with_points3d_arrays(segs, ic, {3: bad})
    with pytest.raises(ValueError):
        fitting.fit_3d_segs_with_points3d_arrays(segs, ic, {3: good}, scan_poses={3: np.full((4, 4), np.nan)})
    with pytest.raises(ValueError):
        fitting.fit_3d_segs_with_points3d_arrays(segs, ic, {3: good}, scan_poses={3: np.eye(3)})
    with pytest.raises(KeyError):
        fitting.fit_3d_segs_with_points3d_arrays(segs, ic, {3: good}, scan_poses={4: np.eye(4)})
    with pytest.raises(ValueError):
        fitting.fit_3d_segs_with_points3d_arrays(segs, ic, {3: good}, scan_poses={3: np.eye(4)}, inloc_dataset="x")
    with pytest.raises(KeyError):
        fitting.fit_3d_segs_with_points3d_arrays(segs, ic, {4: good})
    for hw in ((1, 100), (80, 1)):
        v = base.CameraView([100.0, 100.0, 50.0, 40.0], [1.0, 0, 0, 0], [0.0, 0, 0], hw=hw)
        with pytest.raises(ValueError):
            fitting.fit_3d_segs_with_points3d_arrays(segs, base.ImageCollection({3: v}), {3: good})
    nosize = base.ImageCollection({3: base.CameraView([100.0, 100.0, 50.0, 40.0], [1.0, 0, 0, 0], [0.0, 0, 0])})
    with pytest.raises(ValueError, match="image size"):
        fitting.fit_3d_segs_with_points3d_arrays(segs, nosize, {3: good})
    with pytest.raises(ValueError):
        fitting.fit_3d_segs_with_points3d_arrays({3: np.array([[np.inf, 2.0, 30.0, 20.0]])}, ic, {3: good})
    with pytest.raises(ValueError):
        fitting.fit_3d_segs_with_points3d_arrays(segs, ic, {3: good}, dict(var2d=float("nan")))
    with pytest.raises(ValueError):
        fitting.estimate_seg3d_from_points3d(segs[3][0], np.ones((80, 100, 3), np.float16), view, "a")


def test_inloc_dataset_needs_hloc():
    import importlib.util
    from limap_amd import base, fitting
    if importlib.util.find_spec("hloc") is not None:
        pytest.skip("hloc is installed here")
    view = base.CameraView([100.0, 100.0, 50.0, 40.0], [1.0, 0, 0, 0], [0.0, 0, 0], hw=(80, 100))
    with pytest.raises(ImportError):
        fitting.estimate_seg3d_from_points3d([1.0, 2.0, 30.0, 20.0], np.ones((80, 100, 3)), view, "a", "dataset")


def test_tracks_from_fit_order_and_zero_length():
    from limap_amd import fitting
    all_2d = {7: np.array([[0.0, 0, 10, 0], [1, 1, 5, 5], [2, 2, 3, 3]]), 2: np.array([[4.0, 4, 9, 9]])}
    z = np.zeros(3)
    seg3d = {7: [(np.array([0.0, 0, 1]), np.array([1.0, 0, 1])), (z, z), (np.ones(3), np.ones(3) * 2)],
             2: np.array([[[0.0, 1, 2], [3, 4, 5]]])}
    tr = fitting.tracks_from_fit(all_2d, seg3d)
    assert [(t.image_id_list, t.line_id_list) for t in tr] == [([7], [0]), ([7], [2]), ([2], [0])]
    assert np.array_equal(tr[1].line.start, np.ones(3)) and np.array_equal(tr[2].line.end, [3.0, 4, 5])
    assert np.array_equal(tr[0].line2d_list[0].start, [0.0, 0]) and np.array_equal(tr[0].line2d_list[0].end, [10.0, 0])
    assert fitting.tracks_from_fit({}, {}) == []
