"""limap_amd.features without a GPU: the library's host path (lt_fn_patch_extract_host, lt_fn_patch_geometry,
lt_fn_patch_ranges) equals tests/patch_oracle.py -- a NumPy restatement of DESIGN.md section 24 -- bit for bit on the
case families of tests/patch_cases.py: the array, R, tvec, the shape and img_hw.  Then a known answer, the single
rounding to binary16, the Python surface (Extract, extract_track_patches, write_patch / load_patch), every refusal and
the sanitizer program of the host path."""
import ctypes as C
import os

import numpy as np
import pytest

import patch_cases as pc
import patch_oracle as po

UINT = {"float16": np.uint16, "float32": np.uint32, "float64": np.uint64}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(UINT[a.dtype.name])


def assert_same(patch, want, dtype):
    arr, R, tvec, hw = want
    assert patch.array.dtype == np.dtype(dtype) and patch.array.shape == arr.shape, (patch.array.shape, arr.shape)
    assert np.array_equal(bits(patch.array), bits(arr))
    assert patch.R.shape == (2, 2) and np.array_equal(bits(patch.R), bits(R))
    assert patch.tvec.shape == (2,) and np.array_equal(bits(patch.tvec), bits(tvec))
    assert patch.img_hw == hw


def extractor(opts=None, channels=None):
    from limap_amd import features
    return features.get_line_patch_extractor(opts or {}, channels)


# ---- 1. a known answer ----
def test_known_answer(gpu_lib):
    f = pc.feature(c=3)
    p = extractor(channels=3).ExtractLinePatch(pc.lines_array(["horizontal"])[0], f, host=True)
    assert p.array.shape == (31, 21, 3) and p.array.dtype == np.float64
    assert np.array_equal(p.R, [[0.0, -1.0], [1.0, 0.0]]) and p.tvec.tolist() == [5.0, 30.0] and p.img_hw == (40, 48)
    ys, xs = np.meshgrid(np.arange(31), np.arange(21), indexing="ij")
    assert np.array_equal(p.array, f[30 - xs, 5 + ys])
    # the configuration of cfgs/refinement/default.yaml: 31 x 17, tvec = (5, 28), patch[y, x] == feature[28 - x, 5 + y]
    p = extractor({"range_perp": 16}).ExtractLinePatch(pc.lines_array(["horizontal"])[0], f, host=True)
    assert p.array.shape == (31, 17, 3) and p.tvec.tolist() == [5.0, 28.0]
    assert np.array_equal(p.R, [[0.0, -1.0], [1.0, 0.0]])
    ys, xs = np.meshgrid(np.arange(31), np.arange(17), indexing="ij")
    assert np.array_equal(p.array, f[28 - xs, 5 + ys])


def test_option_defaults(gpu_lib):
    from limap_amd import _capi, features
    o = features.LinePatchExtractorOptions()
    assert (o.k_stretch, o.t_stretch, o.range_perp) == (1.0, 10, 20)
    cfg = _capi.LtPatchConfig()
    gpu_lib.lt_patch_config_default(C.byref(cfg))
    assert (cfg.k_stretch, cfg.t_stretch, cfg.range_perp) == (1.0, 10, 20)
    o = features.LinePatchExtractorOptions({"range_perp": 16, "unknown": 3})
    assert (o.k_stretch, o.t_stretch, o.range_perp) == (1.0, 10, 16)
    assert features.PatchInfo_f16 is features.PatchInfo_f32 is features.PatchInfo_f64 is features.PatchInfo


# ---- 2. host path == the restatement, bit for bit ----
@pytest.mark.parametrize("opt", sorted(pc.OPTIONS))
def test_lines_and_options(gpu_lib, opt):
    o = pc.OPTIONS[opt]
    f = pc.feature(c=3, seed=1)
    names = sorted(pc.LINES)
    got = extractor(o).ExtractLinePatches(pc.lines_array(names), f, host=True)
    assert len(got) == len(names)
    for name, p in zip(names, got):
        assert_same(p, po.extract(pc.LINES[name], f, **o), "float64")
    one = extractor(o).ExtractLinePatch(pc.LINES["diagonal"], f, host=True)
    assert_same(one, po.extract(pc.LINES["diagonal"], f, **o), "float64")


def test_degenerate_shapes(gpu_lib):
    f = pc.feature(c=2, seed=2)
    p = extractor(dict(t_stretch=0, range_perp=0)).ExtractLinePatch(pc.LINES["zero_length"], f, host=True)
    assert p.array.shape == (1, 1, 2)
    assert_same(p, po.extract(pc.LINES["zero_length"], f, t_stretch=0, range_perp=0), "float64")
    p = extractor().ExtractLinePatch(pc.LINES["zero_length"], f, host=True)
    # direc = (0, 0): the stretched line is still a point, one row, and every texel samples the midpoint
    assert p.array.shape == (1, 21, 2) and np.array_equal(p.R, np.zeros((2, 2))) and p.tvec.tolist() == [17.25, 9.5]
    assert (p.array == p.array[0, 0]).all()
    # every texel of a patch entirely outside the image blends four copies of the clamped corner texel: (1 - d) v + d v
    # three times, each within a few roundings of v (two products and a sum: 3 * 2^-53 relative each)
    p = extractor().ExtractLinePatch(pc.LINES["outside"], f, host=True)
    assert (np.abs(p.array - f[0, 0]) <= 9 * 2.0 ** -53 * np.abs(f[0, 0])).all()
    assert extractor().ExtractLinePatches(np.zeros((0, 4)), f, host=True) == []


@pytest.mark.parametrize("c", pc.CHANNELS)
def test_channels_and_dtypes(gpu_lib, c):
    names = ["diagonal", "over_left", "subpixel"] if c == 128 else sorted(pc.LINES)
    for din in pc.DTYPES:
        f = pc.feature(c=c, dtype=din, seed=3)
        for dout in pc.DTYPES:
            got = extractor(channels=c).ExtractLinePatches(pc.lines_array(names), f, host=True, dtype=dout)
            for name, p in zip(names, got):
                assert_same(p, po.extract(pc.LINES[name], f, dtype=dout), dout)


def test_small_map(gpu_lib):
    f = pc.feature(*pc.SMALL_HW, c=5, seed=4)
    lines = pc.mixed_lines(9, pc.SMALL_HW, seed=5)
    o = dict(k_stretch=1.0, t_stretch=0, range_perp=4)
    for line, p in zip(lines, extractor(o).ExtractLinePatches(lines, f, host=True, dtype="float32")):
        assert_same(p, po.extract(line, f, dtype="float32", **o), "float32")


def test_single_rounding_to_binary16(gpu_lib):
    """node-exact samples return the texel itself, so the output is the narrowing of the map's values alone"""
    assert np.float16(pc.TIE) == pc.TIE_F16 and np.float16(np.float32(pc.TIE)) == np.float16(1.0)
    f = np.full((pc.H, pc.W, 1), pc.TIE)
    p = extractor().ExtractLinePatch(pc.LINES["horizontal"], f, host=True, dtype="float16")
    assert p.array.dtype == np.float16 and (p.array == pc.TIE_F16).all()
    # ties, the subnormal range, the overflow threshold and magnitudes from 2^-30 to 2^17, both signs
    rng = np.random.default_rng(11)
    vals = np.ldexp(rng.uniform(1.0, 2.0, pc.H * pc.W), rng.integers(-30, 18, pc.H * pc.W)) * rng.choice([-1.0, 1.0], pc.H * pc.W)
    special = [0.0, 65504.0, 65519.999, 65520.0, -65520.0, 1e9, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -40),
               2.0 ** -26, 3 * 2.0 ** -25, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11,
               1e-320]
    vals[:len(special)] = special
    f = rng.permutation(vals).reshape(pc.H, pc.W, 1)
    for dout in ("float16", "float32"):
        with np.errstate(over="ignore", under="ignore"):
            want = po.extract(pc.LINES["horizontal"], f, dtype=dout)
        got = extractor().ExtractLinePatch(pc.LINES["horizontal"], f, host=True, dtype=dout)
        assert_same(got, want, dout)
        ys, xs = np.meshgrid(np.arange(31), np.arange(21), indexing="ij")
        with np.errstate(over="ignore", under="ignore"):
            assert np.array_equal(bits(got.array[..., 0]), bits(f[30 - xs, 5 + ys, 0].astype(dout)))


def test_strided_input_equals_its_contiguous_copy(gpu_lib):
    chw = np.ascontiguousarray(pc.feature(c=8, dtype="float32", seed=6).transpose(2, 0, 1))
    view = chw.transpose(1, 2, 0)
    assert not view.flags.c_contiguous
    lines = pc.lines_array()
    a = extractor().ExtractLinePatches(lines, view, host=True, dtype="float16")
    b = extractor().ExtractLinePatches(lines, np.ascontiguousarray(view), host=True, dtype="float16")
    for x, y in zip(a, b):
        assert np.array_equal(bits(x.array), bits(y.array))
    # a map flipped along both axes (negative strides) and a channel slice (pixel stride larger than C)
    f = pc.feature(c=6, seed=7)
    for v in (f[::-1, ::-1], f[:, :, 1:4], f[::2, 1::3]):
        got = extractor().ExtractLinePatch(pc.LINES["diagonal"], v, host=True)
        assert_same(got, po.extract(pc.LINES["diagonal"], np.ascontiguousarray(v)), "float64")


# ---- 3. GetLine2DRange ----
def make_track(sup_img, sup_seg4, line6=pc.LINE6):
    from limap_amd import base
    return base.LineTrack(base.Line3d(line6[:3], line6[3:]), list(sup_img), list(range(len(sup_img))),
                          [base.Line2d(s[:2], s[2:]) for s in sup_seg4])


def make_view(cam11=pc.CAM11):
    from limap_amd import base
    return base.CameraView(cam11[:4], cam11[4:8], cam11[8:], hw=(pc.H, pc.W))


def test_line2d_range(gpu_lib):
    scenes = pc.range_scenes(po.project)
    for name, (sup_img, segs, image_id) in scenes.items():
        want, status = po.line2d_range(pc.LINE6, sup_img, segs, image_id, pc.CAM11)
        assert status == 0, name
        got = extractor().GetLine2DRange(make_track(sup_img, segs), image_id, make_view())
        assert np.array_equal(bits(np.concatenate([got.start, got.end])), bits(want)), name
    # the clamps: supports beyond both ends give the projection itself
    gs, ge = po.project(pc.CAM11, pc.LINE6[:3])[0], po.project(pc.CAM11, pc.LINE6[3:])[0]
    sup_img, segs, image_id = scenes["beyond_both_ends"]
    got = extractor().GetLine2DRange(make_track(sup_img, segs), image_id, make_view())
    assert np.array_equal(got.start, gs) and np.allclose(got.end, ge, rtol=0, atol=1e-9)
    # a support of another image does not widen the range
    a = extractor().GetLine2DRange(make_track(*scenes["other_image_ignored"][:2]), 7, make_view())
    b = extractor().GetLine2DRange(make_track([7], [scenes["other_image_ignored"][1][1]]), 7, make_view())
    assert np.array_equal(a.start, b.start) and np.array_equal(a.end, b.end)


def test_line2d_range_errors(gpu_lib):
    scenes = pc.range_scenes(po.project)
    sup_img, segs, _ = scenes["one_support"]
    with pytest.raises(ValueError, match=r"track 0 has no supporting line in image 9"):
        extractor().GetLine2DRange(make_track(sup_img, segs), 9, make_view())
    behind = np.array([-0.2, -0.15, 6.0, 0.25, 0.2, -1.0])  # the end lies behind the camera
    assert po.line2d_range(behind, sup_img, segs, 7, pc.CAM11)[1] == 2
    with pytest.raises(ValueError, match=r"track 0 .*behind the camera plane in image 7"):
        extractor().GetLine2DRange(make_track(sup_img, segs, behind), 7, make_view())
    on_plane = pc.LINE6.copy()
    on_plane[5] = on_plane[2] = 0.0
    cam = pc.CAM11.copy()
    cam[4:8], cam[8:] = [1, 0, 0, 0], 0.0
    with pytest.raises(ValueError, match=r"image 7"):
        extractor().GetLine2DRange(make_track(sup_img, segs, on_plane), 7, make_view(cam))
    from limap_amd import features
    with pytest.raises(ValueError, match="track 1 has no supporting line in image 4"):
        features.line2d_ranges([make_track(sup_img, segs)] * 2, [(0, 7), (1, 4)], [make_view()] * 2)


# ---- 4. the Python surface ----
def test_extract_goes_over_the_sorted_image_ids(gpu_lib):
    from limap_amd import features
    scenes = pc.range_scenes(po.project)
    seg = scenes["several"][1]
    track = make_track([7, 2, 7, 5], [seg[0], seg[1], seg[2], seg[1]])
    assert track.GetSortedImageIds() == [2, 5, 7] and track.count_images() == 3
    views = [make_view()] * 3
    feats = [pc.feature(c=3, seed=20 + k) for k in range(3)]
    ext = extractor(pc.OPTIONS["perp16"], 3)
    got = ext.Extract(track, views, feats, host=True)
    assert len(got) == 3
    for k, img_id in enumerate([2, 5, 7]):
        r, status = po.line2d_range(pc.LINE6, track.image_id_list, [l.as_array().reshape(4) for l in track.line2d_list],
                                    img_id, pc.CAM11)
        assert status == 0
        assert_same(got[k], po.extract(r, feats[k], **pc.OPTIONS["perp16"]), "float64")
        one = features.extract_line_patch_one_image(pc.OPTIONS["perp16"], track, img_id, views[k], feats[k], host=True)
        assert np.array_equal(bits(one.array), bits(got[k].array))
    again = features.extract_line_patches(pc.OPTIONS["perp16"], track, views, feats, host=True)
    assert all(np.array_equal(bits(a.array), bits(b.array)) for a, b in zip(again, got))
    with pytest.raises(ValueError, match="p_views"):
        ext.Extract(track, views[:2], feats, host=True)
    with pytest.raises(ValueError, match="p_features"):
        ext.Extract(track, views, feats[:2], host=True)
    with pytest.raises(ValueError, match="made for 3 channels"):
        ext.ExtractLinePatch(pc.LINES["diagonal"], pc.feature(c=5), host=True)


@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_write_and_load_patch(gpu_lib, tmp_path, dtype):
    from limap_amd import features
    f = pc.feature(c=3, seed=8)
    p = extractor().ExtractLinePatch(pc.LINES["diagonal"], f, host=True)
    name = str(tmp_path / "track0_img0.npy")
    features.write_patch(name, p, dtype=dtype)
    with open(name, "rb") as fh:
        data = np.load(fh, allow_pickle=False)
        assert sorted(data.files) == ["R", "array", "img_hw", "tvec"] and data["array"].dtype == np.dtype(dtype)
    q = features.load_patch(name, dtype=dtype)
    assert q.array.dtype == np.dtype(dtype) and np.array_equal(bits(q.array), bits(p.array.astype(dtype)))
    assert np.array_equal(q.R, p.R) and np.array_equal(q.tvec, p.tvec) and q.img_hw == p.img_hw
    # the stored type extracted directly is the same bits as the cast of the float64 patch
    direct = extractor().ExtractLinePatch(pc.LINES["diagonal"], f, host=True, dtype=dtype)
    assert np.array_equal(bits(direct.array), bits(q.array))


def scene():
    from limap_amd import base
    scenes = pc.range_scenes(po.project)
    seg = scenes["several"][1]
    cams = {2: pc.CAM11, 5: pc.CAM11 + np.array([0, 0, 1.5, -2.0, 0, 0.01, 0, 0, 0.05, 0, 0]), 7: pc.CAM11}
    imagecols = base.ImageCollection({i: make_view(c) for i, c in cams.items()})
    tracks = [make_track([7, 2, 7], [seg[0], seg[1], seg[2]]), make_track([5, 2], [seg[2], seg[0]])]
    feats = {i: pc.feature(c=8, dtype="float16", seed=30 + i) for i in cams}
    return tracks, imagecols, feats


def test_extract_track_patches(gpu_lib, tmp_path):
    from limap_amd import features
    tracks, imagecols, feats = scene()
    cfg = {"patch": pc.OPTIONS["perp16"], "channels": 8, "dtype": "float16"}
    calls = []
    got = features.extract_track_patches(cfg, tracks, imagecols, lambda i: calls.append(i) or feats[i], host=True)
    assert calls == [2, 5, 7]  # one extraction per image
    assert sorted(got) == [(0, 2), (0, 7), (1, 2), (1, 5)]
    ext = extractor(cfg["patch"], 8)
    for (t, i), p in got.items():
        one = ext.ExtractOneImage(tracks[t], i, imagecols.camview(i), feats[i], host=True, dtype="float16")
        assert p.array.dtype == np.float16 and np.array_equal(bits(p.array), bits(one.array))
        assert np.array_equal(p.R, one.R) and np.array_equal(p.tvec, one.tvec) and p.img_hw == (pc.H, pc.W)
    out = str(tmp_path / "patches")
    assert features.extract_track_patches(cfg, tracks, imagecols, feats, output_dir=out, host=True) is None
    files = sorted(os.path.relpath(os.path.join(d, f), out) for d, _, fs in os.walk(out) for f in fs)
    assert files == ["track0/track0_img2.npy", "track0/track0_img7.npy", "track1/track1_img2.npy", "track1/track1_img5.npy"]
    for (t, i), p in got.items():
        q = features.load_patch(os.path.join(out, f"track{t}", f"track{t}_img{i}.npy"))
        assert np.array_equal(bits(q.array), bits(p.array)) and np.array_equal(q.tvec, p.tvec)
    # skip_exists keeps what is there and extracts nothing for it
    calls.clear()
    features.extract_track_patches(cfg, tracks, imagecols, lambda i: calls.append(i) or feats[i], output_dir=out,
                                   skip_exists=True, host=True)
    assert calls == []
    with pytest.raises(NotImplementedError):
        features.load_extractor("s2dnet", "cuda")


# ---- 5. refusals, before any work ----
def test_argument_errors(gpu_lib):
    from limap_amd import _capi, features
    f = pc.feature(c=3)
    line = pc.LINES["diagonal"]
    for bad, what in ((dict(range_perp=-1), "range_perp below 0"), (dict(t_stretch=-1), "t_stretch below 0"),
                      (dict(k_stretch=float("nan")), "k_stretch"), (dict(k_stretch=float("inf")), "k_stretch"),
                      (dict(range_perp=5000), "range_perp above")):
        with pytest.raises(ValueError, match=what):
            extractor(bad).ExtractLinePatch(line, f, host=True)
    with pytest.raises(ValueError, match="must be an integer"):
        features.LinePatchExtractorOptions(dict(range_perp=2.5))
    for k in range(4):
        for v in (np.nan, np.inf):
            l = np.array(line)
            l[k] = v
            with pytest.raises(ValueError, match="line 1: non-finite coordinate"):
                extractor().ExtractLinePatches(np.stack([np.array(line), l]), f, host=True)
    with pytest.raises(ValueError, match="rows"):
        extractor().ExtractLinePatch((0.0, 0.0, 1e300, 0.0), f, host=True)
    with pytest.raises(ValueError, match="rows"):
        extractor().ExtractLinePatch((0.0, 0.0, 3e6, 0.0), f, host=True)
    with pytest.raises(ValueError, match="float16, float32 or float64"):
        extractor().ExtractLinePatch(line, f.astype(np.int32), host=True)
    with pytest.raises(ValueError, match=r"\(H, W, C\)"):
        extractor().ExtractLinePatch(line, f[:, :, 0], host=True)
    with pytest.raises(ValueError, match="H, W, C >= 1"):
        extractor().ExtractLinePatch(line, f[:, :, :0], host=True)
    with pytest.raises(ValueError, match="output dtype"):
        extractor().ExtractLinePatch(line, f, host=True, dtype="int8")
    with pytest.raises(ValueError, match="device_out"):
        extractor().ExtractLinePatch(line, f, host=True, device_out=True)
    with pytest.raises(ValueError, match="channels must be >= 1"):
        features.get_line_patch_extractor({}, 0)
    # the library refuses the same on its own (a caller of the C ABI has no Python in front of it)
    L = gpu_lib
    cfg = _capi.LtPatchConfig(1.0, 10, 20)
    lines = np.array([line])
    out = np.zeros(31 * 60 * 21 * 3)

    def call(fm, cfg=cfg, out_dtype=_capi.PATCH_F64, n=1):
        rc = L.lt_fn_patch_extract_host(C.byref(cfg), C.byref(fm), n, _capi.ptr(lines), out_dtype, out.ctypes.data, 1)
        return rc, L.lt_fn_patch_host_error().decode()

    def fmap(h=pc.H, w=pc.W, c=3, dtype=_capi.PATCH_F64, ptr=f.ctypes.data, dev=0):
        return _capi.LtFeatureMap(ptr, h, w, c, w * c, c, 1, dtype, dev)

    assert call(fmap()) == (0, "")
    for fm, what in ((fmap(h=0), "below 1"), (fmap(w=0), "below 1"), (fmap(c=0), "below 1"), (fmap(dtype=3), "unknown feature map dtype"),
                     (fmap(ptr=None), "null feature map data"), (fmap(dev=1), "device feature map")):
        rc, msg = call(fm)
        assert rc == -2 and what in msg, (rc, msg)
    assert call(fmap(), out_dtype=5)[0] == -2 and "unknown output dtype" in L.lt_fn_patch_host_error().decode()
    assert call(fmap(), cfg=_capi.LtPatchConfig(1.0, 10, -3))[0] == -2
    assert call(fmap(), cfg=_capi.LtPatchConfig(1.0, -1, 3))[0] == -2
    assert call(fmap(), n=-1)[0] == -2
    assert call(fmap()) == (0, "")  # and the call after a refusal works


def test_sanitizer_program_of_the_host_path():
    """tools/patch_host_asan.cpp + lt_patch.cpp (host-only) under AddressSanitizer and UBSan, a program of its own"""
    from helpers import run_host_asan
    run_host_asan("patch_asan", "patch_host_asan")
