"""limap_amd.features on the device: k_patch_gather equals the library's host path bit for bit -- arrays, R, tvec,
shapes -- on the smallest shapes at which the kernel can go wrong (tests/patch_cases.py): both forms of the kernel,
every channel count and type, patch heights around the block table's boundaries, 0 to 65 patches in a launch, strided
and misaligned maps read in place, the single rounding to binary16, chunks, the output left on the device.  The host
path itself is pinned to tests/patch_oracle.py by test_patch_host.py; it runs first in every test here."""
import ctypes as C

import numpy as np
import pytest

import patch_cases as pc

pytestmark = pytest.mark.gpu

UINT = {"float16": np.uint16, "float32": np.uint32, "float64": np.uint64}
ITEMSIZE = {"float16": 2, "float32": 4, "float64": 8}
BLOCK_ITEMS = 2048  # lane items a block-table entry aims at


def bits(a):
    if type(a).__module__.split(".")[0] == "torch":
        a = a.detach().cpu().numpy()
    a = np.ascontiguousarray(a)
    return a.view(UINT[a.dtype.name])


def same(dev, ref):
    assert len(dev) == len(ref)
    for k, (d, r) in enumerate(zip(dev, ref)):
        assert tuple(d.array.shape) == r.array.shape, k
        assert np.array_equal(bits(d.array), bits(r.array)), k
        assert np.array_equal(bits(d.R), bits(r.R)) and np.array_equal(bits(d.tvec), bits(r.tvec)), k
        assert d.img_hw == r.img_hw


def both(opts, lines, f, f_dev=None, **kw):
    """host first, then the device (on f_dev where given): -> the host's patches, after asserting the device's are
    the same bits"""
    from limap_amd import features
    ext = features.get_line_patch_extractor(opts, None)
    ref = ext.ExtractLinePatches(lines, f, host=True, dtype=kw.get("dtype"))
    dev = ext.ExtractLinePatches(lines, f if f_dev is None else f_dev, **kw)
    same(dev, ref)
    return ref


def vector_expected(c, din):
    return c % (16 // ITEMSIZE[din]) == 0


@pytest.mark.parametrize("c", pc.CHANNELS)
def test_channels_types_and_forms(gpu_lib, c):
    """every channel count with every input and output type on both maps; a packed host map runs the vector form
    exactly where C is a multiple of the lane's channels (8, 4, 2)"""
    from limap_amd import features
    for hw, lines in ((pc.SMALL_HW, pc.mixed_lines(5, pc.SMALL_HW, seed=c)), ((pc.H, pc.W), pc.lines_array())):
        if c == 128:
            lines = lines[:4]
        for din in pc.DTYPES:
            f = pc.feature(*hw, c=c, dtype=din, seed=c)
            for dout in pc.DTYPES:
                both(pc.OPTIONS["perp16"], lines, f, dtype=dout)
                t = features.timers()
                assert t["vector_form"] == float(vector_expected(c, din)), (c, din)
                assert t["patches"] == len(lines) and t["chunks"] == 1


@pytest.mark.parametrize("opt", sorted(pc.OPTIONS))
def test_line_fixtures_and_options(gpu_lib, opt):
    for c, din in ((3, "float64"), (8, "float16")):
        both(pc.OPTIONS[opt], pc.lines_array(), pc.feature(c=c, dtype=din, seed=1), dtype="float32")
    both(dict(pc.OPTIONS[opt], t_stretch=0), [pc.LINES["zero_length"]], pc.feature(c=2, seed=2))


@pytest.mark.parametrize("n", [0, 1, 2, 65])
def test_patch_counts(gpu_lib, n):
    """patches of 1 to about 80 rows mixed in one launch, in both forms"""
    from limap_amd import features
    lines = pc.mixed_lines(n, seed=n)
    o = dict(k_stretch=1.0, t_stretch=0, range_perp=6)
    for c, din in ((8, "float16"), (5, "float32")):
        ref = both(o, lines, pc.feature(c=c, dtype=din, seed=3), dtype="float16")
        if n >= 2:
            hs = [p.array.shape[0] for p in ref]
            assert hs[0] == 1 and max(hs) >= 79
        assert features.timers()["patches"] == n


def test_rows_around_the_block_table_boundaries(gpu_lib):
    """a table entry covers max(1, 2048 // (patch_w * C / lane channels)) rows: patches one row short of an entry, of
    exactly one, one more, two and two plus one; the number of workgroups pins the table"""
    from limap_amd import features
    for c, din, perp in ((1, "float64", 20), (8, "float32", 20), (128, "float16", 16), (3, "float16", 0), (16, "float64", 4)):
        lane_c = 16 // ITEMSIZE[din] if vector_expected(c, din) else 1
        rows_per = max(1, BLOCK_ITEMS // ((perp + 1) * (c // lane_c)))
        hs = sorted({max(rows_per - 1, 1), rows_per, rows_per + 1, 2 * rows_per, 2 * rows_per + 1})
        # a horizontal line of length h - 1 with t_stretch = 0 has h rows
        lines = np.array([[2.0, 7.0, 2.0 + (h - 1), 7.0] for h in hs])
        o = dict(k_stretch=1.0, t_stretch=0, range_perp=perp)
        ref = both(o, lines, pc.feature(c=c, dtype=din, seed=4), dtype="float16")
        assert [p.array.shape[0] for p in ref] == hs
        assert features.timers()["blocks"] == sum(-(-h // rows_per) for h in hs), (c, din)


def test_single_rounding_to_binary16(gpu_lib):
    f = np.full((pc.H, pc.W, 2), pc.TIE)  # two doubles: the vector form
    ref = both({}, [pc.LINES["horizontal"]], f, dtype="float16")
    assert (ref[0].array == pc.TIE_F16).all()
    ref = both({}, [pc.LINES["horizontal"]], f[:, :, :1], dtype="float16")  # and the scalar form
    assert (ref[0].array == pc.TIE_F16).all()
    rng = np.random.default_rng(11)
    vals = np.ldexp(rng.uniform(1.0, 2.0, pc.H * pc.W), rng.integers(-30, 18, pc.H * pc.W)) * rng.choice([-1.0, 1.0], pc.H * pc.W)
    special = [0.0, 65504.0, 65519.999, 65520.0, -65520.0, 1e9, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -40),
               2.0 ** -26, 3 * 2.0 ** -25, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1e-320]
    vals[:len(special)] = special
    f = rng.permutation(vals).reshape(pc.H, pc.W, 1)
    for dout in ("float16", "float32"):
        both({}, [pc.LINES["horizontal"], pc.LINES["subpixel"]], f, dtype=dout)
        both({}, [pc.LINES["horizontal"], pc.LINES["subpixel"]], np.concatenate([f, f[::-1]], 2), dtype=dout)


def test_torch_tensors_read_in_place(gpu_lib):
    """contiguous (vector form), permuted from (C, H, W), a misaligned base, an odd pixel stride (all scalar), and a
    channel slice that keeps every alignment (vector form through strides)"""
    import torch
    from limap_amd import features
    lines = pc.lines_array()
    c = 8
    f = pc.feature(c=c, dtype="float16", seed=5)
    t = torch.from_numpy(f).cuda()
    chw = torch.from_numpy(np.ascontiguousarray(f.transpose(2, 0, 1))).cuda()
    flat = torch.zeros(f.size + 8, dtype=torch.float16, device="cuda")
    flat[1:1 + f.size] = t.reshape(-1)
    wide = torch.zeros((pc.H, pc.W, c + 1), dtype=torch.float16, device="cuda")
    wide[:, :, :c] = t
    wide2 = torch.zeros((pc.H, pc.W, 2 * c), dtype=torch.float16, device="cuda")
    wide2[:, :, c:] = t
    cases = (("contiguous", t, 1.0), ("permuted", chw.permute(1, 2, 0), 0.0),
             ("misaligned", flat[1:1 + f.size].view(pc.H, pc.W, c), 0.0), ("odd_stride", wide[:, :, :c], 0.0),
             ("aligned_slice", wide2[:, :, c:], 1.0))
    for name, dev, vec in cases:
        assert not (name == "misaligned" and dev.data_ptr() % 16 == 0)
        before = dev.clone()
        both(pc.OPTIONS["perp16"], lines, f, f_dev=dev, dtype="float16")
        assert features.timers()["vector_form"] == vec, name
        assert torch.equal(dev, before), name
    for din in ("float32", "float64"):
        g = pc.feature(c=4, dtype=din, seed=6)
        both({}, lines, g, f_dev=torch.from_numpy(g).cuda())
        both({}, lines, g, f_dev=torch.from_numpy(np.ascontiguousarray(g.transpose(2, 0, 1))).cuda().permute(1, 2, 0))


def test_device_out_equals_the_download(gpu_lib):
    import torch
    lines = pc.mixed_lines(7, seed=7)
    f = pc.feature(c=16, dtype="float16", seed=7)
    for dout in pc.DTYPES:
        ref = both(pc.OPTIONS["perp16"], lines, f, dtype=dout)
        dev = both(pc.OPTIONS["perp16"], lines, f, f_dev=torch.from_numpy(f).cuda(), dtype=dout, device_out=True)
        from limap_amd import features
        out = features.get_line_patch_extractor(pc.OPTIONS["perp16"], 16).ExtractLinePatches(lines, f, dtype=dout, device_out=True)
        assert all(p.array.is_cuda and p.array.dtype == getattr(torch, dout) for p in out)
        same(out, ref)
        same(out, dev)


def test_chunks_and_repeats(gpu_lib):
    from limap_amd import features
    f = pc.feature(c=12, dtype="float32", seed=8)
    o = dict(k_stretch=1.0, t_stretch=0, range_perp=8)
    lines = np.array([[3.0, 5.0 + k, 33.0, 9.0 + k] for k in range(3)])  # three patches of one size
    ref = both(o, lines, f, dtype="float32")
    one = ref[0].array.nbytes
    assert all(p.array.nbytes == one for p in ref)
    both(o, lines, f, dtype="float32", max_chunk_bytes=one)
    assert features.timers()["chunks"] == 3
    both(o, lines, f, dtype="float32", max_chunk_bytes=1)  # below one patch: still one patch per chunk
    assert features.timers()["chunks"] == 3
    both(o, lines, f, dtype="float32", max_chunk_bytes=2 * one)
    assert features.timers()["chunks"] == 2
    mixed = pc.mixed_lines(20, seed=9)
    ref = both(o, mixed, f, dtype="float16")
    both(o, mixed, f, dtype="float16", max_chunk_bytes=sum(p.array.nbytes for p in ref) // 3)
    assert features.timers()["chunks"] >= 3
    # two runs give the same bytes
    ext = features.get_line_patch_extractor(o, 12)
    a = ext.ExtractLinePatches(mixed, f, dtype="float16")
    b = ext.ExtractLinePatches(mixed, f, dtype="float16")
    same(a, b)


def test_timers_and_the_call_after_an_argument_error(gpu_lib):
    from limap_amd import _capi, features
    f = pc.feature(c=8, dtype="float16", seed=10)
    both({}, pc.lines_array(), f, dtype="float16")
    t = features.timers()
    assert sorted(t) == sorted(features.TIMER_KEYS) and all(v >= 0 for v in t.values())
    assert t["kernel_ms"] > 0 and t["out_bytes"] > 0 and t["blocks"] >= t["patches"] == len(pc.LINES)
    ctx = features._context(0)
    fm = _capi.LtFeatureMap(f.ctypes.data, pc.H, pc.W, 8, pc.W * 8, 8, 1, _capi.PATCH_F16, 0)
    lines = pc.lines_array()
    out = np.zeros(1 << 20, np.float16)
    for cfg, what in ((_capi.LtPatchConfig(1.0, 10, -1), "range_perp below 0"), (_capi.LtPatchConfig(1.0, -2, 4), "t_stretch below 0"),
                      (_capi.LtPatchConfig(float("inf"), 10, 4), "k_stretch")):
        rc = ctx.L.lt_patch_extract(ctx.h, C.byref(cfg), C.byref(fm), len(lines), _capi.ptr(lines), _capi.PATCH_F16,
                                    out.ctypes.data, 0, 0)
        assert rc == -2 and what in ctx.L.lt_last_error(ctx.h).decode()
    bad = lines.copy()
    bad[3, 2] = np.nan
    cfg = _capi.LtPatchConfig(1.0, 10, 4)
    rc = ctx.L.lt_patch_extract(ctx.h, C.byref(cfg), C.byref(fm), len(bad), _capi.ptr(bad), _capi.PATCH_F16, out.ctypes.data, 0, 0)
    assert rc == -2 and "line 3: non-finite coordinate" in ctx.L.lt_last_error(ctx.h).decode()
    rc = ctx.L.lt_patch_extract(ctx.h, C.byref(cfg), C.byref(fm), len(lines), _capi.ptr(lines), 7, out.ctypes.data, 0, 0)
    assert rc == -2 and "unknown output dtype" in ctx.L.lt_last_error(ctx.h).decode()
    both({}, pc.lines_array(), f, dtype="float16")
    # the output left in the context: the two getters
    rc = ctx.L.lt_patch_extract(ctx.h, C.byref(cfg), C.byref(fm), len(lines), _capi.ptr(lines), _capi.PATCH_F16, None, 0, 0)
    assert rc == 0
    ptr, nbytes = C.c_void_p(), C.c_int64()
    assert ctx.L.lt_patch_get_device_out(ctx.h, C.byref(ptr), C.byref(nbytes)) == 0 and ptr.value and nbytes.value > 0
    got = np.zeros(nbytes.value // 2, np.float16)
    assert ctx.L.lt_patch_get_out(ctx.h, got.ctypes.data) == 0
    ref = features.get_line_patch_extractor(dict(range_perp=4), 8).ExtractLinePatches(lines, f, host=True, dtype="float16")
    assert np.array_equal(bits(got), np.concatenate([bits(p.array).reshape(-1) for p in ref]))
    hs = np.zeros(len(lines), np.int32)
    assert ctx.L.lt_patch_get_geometry(ctx.h, None, None, _capi.ptr(hs, C.c_int32), None) == 0
    assert hs.tolist() == [p.array.shape[0] for p in ref]


def test_scene_call_on_the_device(gpu_lib):
    """extract_track_patches: one launch per image, equal to the host path's"""
    import torch
    from test_patch_host import scene
    from limap_amd import features
    tracks, imagecols, feats = scene()
    cfg = {"patch": pc.OPTIONS["perp16"], "channels": 8, "dtype": "float16"}
    ref = features.extract_track_patches(cfg, tracks, imagecols, feats, host=True)
    dev = features.extract_track_patches(cfg, tracks, imagecols, {i: torch.from_numpy(f).cuda() for i, f in feats.items()})
    assert sorted(ref) == sorted(dev)
    same([dev[k] for k in sorted(dev)], [ref[k] for k in sorted(ref)])
