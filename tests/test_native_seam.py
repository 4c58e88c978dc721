"""limap_amd._native: the one way from a NumPy array or a torch tensor to a pointer in a native struct.  The device rule
and `Operand` on real arrays and CPU tensors, every rewritten converter on the same data in both kinds, and a source
check that no module keeps a rule of its own.  A CUDA tensor is stood in for by `FakeCuda`; nothing here needs a GPU."""
import glob
import os
import re

import numpy as np
import pytest
import torch

from limap_amd import _capi, _native, features, fitting, line2d, matching, optimize, undistortion

RULE = dict(who="seam", what="the map")


class _Device:
    def __init__(self, index):
        self.index = index

    def __str__(self):
        return f"cuda:{self.index}"


class FakeCuda:
    """what the seam reads of a CUDA tensor: is_cuda, device.index, shape, dtype, stride(); its memory is a host array"""
    is_cuda = True

    def __init__(self, array, index=0):
        self.array, self.device, self.shape = array, _Device(index), array.shape
        self.dtype = "torch." + array.dtype.name

    def stride(self):
        return tuple(s // self.array.itemsize for s in self.array.strides)

    def data_ptr(self):
        return self.array.ctypes.data

    def detach(self):
        return self

    def cpu(self):
        return torch.from_numpy(self.array)

    def to(self, dtype):
        assert "torch." + self.array.dtype.name == str(dtype)
        return self

    def contiguous(self):
        assert self.array.flags.c_contiguous
        return self


FakeCuda.__module__ = "torch._fake"


def fields(struct):
    """every field of a native struct but its pointer"""
    return {name: getattr(struct, name) for name, _ in struct._fields_ if name != "ptr"}


# ---- the device rule ------------------------------------------------------------------------------------------------
def test_device_rule_truth_table():
    a = np.arange(6, dtype=np.float32).reshape(2, 3)
    assert _native.is_torch(torch.zeros(1)) and _native.is_torch(FakeCuda(a)) and not _native.is_torch(a)
    for x in (a, torch.from_numpy(a)):
        for host in (False, True):
            op = _native.operand(x, host=host, device=0, **RULE)
            assert op.on_device == 0 and isinstance(op.keep, np.ndarray) and np.shares_memory(op.keep, a)
    op = _native.operand(FakeCuda(a, 0), host=True, device=0, **RULE)
    assert op.on_device == 0 and isinstance(op.keep, np.ndarray)
    op = _native.operand(FakeCuda(a, 1), host=True, device=0, **RULE)  # the host path takes a copy from any device
    assert op.on_device == 0
    for d in (0, 1):
        fake = FakeCuda(a, d)
        op = _native.operand(fake, host=False, device=d, **RULE)
        assert op.on_device == 1 and op.keep is fake and op.address == a.ctypes.data
        assert op.shape == (2, 3) and op.dtype == "float32" and op.strides == (3, 1)
    with pytest.raises(ValueError) as e:
        _native.operand(FakeCuda(a, 0), host=False, device=1, **RULE)
    assert str(e.value) == "seam: the map lives on cuda:0, the call runs on cuda:1"
    with pytest.raises(ValueError, match="^seam: the map lives on cuda:1, the call runs on cuda:0$"):
        _native.check_device(FakeCuda(a, 1), host=False, device=0, **RULE)
    # a converter that runs before its context is known passes no device; its caller asks again with one
    assert _native.operand(FakeCuda(a, 1), host=False, device=None, **RULE).on_device == 1


class _StubLibrary:
    def __getattr__(self, name):
        return lambda *args: 0


class _StubContext:
    device, h, L = 1, None, _StubLibrary()

    def chk(self, rc):
        assert rc == 0


def test_optimize_refuses_a_tensor_on_another_device_than_its_context(gpu_lib):
    import refine_feature_scenes as fs
    texels = FakeCuda(np.zeros((4, 5, 128), np.float16), 0)
    fm = optimize.FeatureMaps({3: texels}, "float16")
    assert fm.on_device == 1 and fm.addr[3] == texels.data_ptr() and (int(fm.h[0]), int(fm.w[0])) == (4, 5)
    with pytest.raises(ValueError, match="^limap_amd.optimize: a feature map lives on cuda:0, the call runs on cuda:1$"):
        fm.upload(_StubContext())
    s = fs.make_scene(counts=(4,))
    rf = fs.refine_cfg()
    n_grids = len(fs.sorted_ids(s, 0))
    patch = features.PatchInfo(texels, np.eye(2), np.zeros(2), (4, 5))
    grids, nbytes = optimize._patch_grids([patch] * n_grids, np.float16, False, "the patches of track 0")
    assert nbytes == n_grids * 4 * 5 * 128 * 2 and all(g[:3] == (texels, 4, 5) and g[5] == 1 for g in grids)
    garr, n = optimize._grid_array(grids)  # a grid holds its texels; an address stands in where a caller has only that
    bare = optimize._grid_array([(texels.data_ptr(),) + grids[0][1:]])[0]
    assert n == n_grids and garr[0].data == bare[0].data == texels.data_ptr()
    cams = (s["img_ids"], s["k"], s["q"], s["t"])
    csr = (s["line6"], s["off"], s["img"], s["l2d"], s["l3d"])
    with pytest.raises(ValueError, match="^limap_amd.optimize: a patch lives on cuda:0, the call runs on cuda:1$"):
        optimize.refine_arrays(cams, csr, rf._struct(rf.num_outliers_aggregate), ctx=_StubContext(), terms=rf._terms(),
                               feature=rf._feature(None), grids=grids)


# ---- Operand on real arrays and CPU tensors -------------------------------------------------------------------------
def _views():
    base = np.arange(8 * 12, dtype=np.float32).reshape(8, 12)
    return {"transposed": base.T, "every other column": base[:, ::2],
            "fortran": np.asfortranarray(np.arange(5 * 6 * 3, dtype=np.float64).reshape(5, 6, 3))}


@pytest.mark.parametrize("kind", ["numpy", "torch"])
@pytest.mark.parametrize("name", ["transposed", "every other column", "fortran"])
def test_operand_views(kind, name):
    a = _views()[name]
    x = a if kind == "numpy" else torch.from_numpy(a)
    op = _native.operand(x, host=False, device=0, **RULE)
    assert op.shape == a.shape and op.ndim == a.ndim and op.dtype == a.dtype.name and op.on_device == 0
    assert op.strides == tuple(s // a.itemsize for s in a.strides)  # in elements, read in place
    assert op.address == a.ctypes.data and np.shares_memory(op.keep, a)
    c = op.contiguous()
    assert c is not op and c.keep.flags.c_contiguous and not np.shares_memory(c.keep, a) and np.array_equal(c.keep, a)
    assert c.address == c.keep.ctypes.data  # keep owns the memory behind address
    assert c.contiguous() is c and c.astype(a.dtype.name) is c  # a conforming input is shared, not copied
    other = "float64" if a.dtype == np.float32 else "float32"
    w = op.astype(other)
    assert w.dtype == other and w.shape == a.shape and np.array_equal(w.keep, a.astype(other))


def test_operand_reads_what_numpy_lacks_and_what_requires_grad():
    b = torch.ones(2, 3, dtype=torch.bfloat16)
    op = _native.operand(b, host=False, device=0, **RULE)
    assert op.dtype == "bfloat16" and op.shape == (2, 3) and op.on_device == 0  # readable without conversion
    w = op.astype("float32")
    assert isinstance(w.keep, np.ndarray) and w.on_device == 0  # a host Operand ends as an array, never a CPU tensor
    assert w.dtype == "float32" and w.address == w.keep.ctypes.data and w.strides == (3, 1)
    g = torch.arange(6.0).reshape(2, 3).requires_grad_()
    assert np.array_equal(_native.to_host(g), np.arange(6.0).reshape(2, 3))
    assert _native.to_host([1, 2]).tolist() == [1, 2]
    assert _native.address(g) == g.data_ptr() and _native.address(np.zeros(1)) != 0
    odd = np.zeros(3, np.dtype([("pad", "u1"), ("v", "<f4")]))["v"]  # strides of 5 bytes: no whole elements
    op = _native.operand(odd, host=False, device=0, **RULE)
    assert op.strides == (1,) and not np.shares_memory(op.keep, odd)


# ---- one check per rewritten converter: the same data as an array, as a CPU tensor, as a strided view ----------------
def _padded(a, pad=5):
    """a view of `a`'s values whose rows are `pad` elements further apart"""
    big = np.full(a.shape[:1] + (a.shape[1] + pad,) + a.shape[2:], 7, a.dtype)
    big[:, :a.shape[1]] = a
    return big[:, :a.shape[1]]


def _both_kinds(convert, a, stride_fields=()):
    """convert(x) -> dict of fields: equal for the array and the tensor, and for a strided view apart from its strides"""
    ref = convert(a)
    assert convert(torch.from_numpy(a)) == ref
    for x in (_padded(a), torch.from_numpy(_padded(a))):
        got = convert(x)
        assert {k: v for k, v in got.items() if k not in stride_fields} == \
               {k: v for k, v in ref.items() if k not in stride_fields}
    return ref, convert(_padded(a))


def test_converters_of_fitting():
    rng = np.random.default_rng(0)
    for dtype, code in ((np.float32, 0), (np.float64, 1), (np.int32, 1), (np.uint8, 1)):
        depth = rng.uniform(1, 9, (8, 12)).astype(dtype)
        ref, view = _both_kinds(lambda x: fields(fitting._map_of(x)[0]), depth, ("row_stride",))
        assert ref == dict(h=8, w=12, row_stride=12, dtype=code, on_device=0)
        assert view["row_stride"] == (17 if dtype in (np.float32, np.float64) else 12)  # read in place unless converted
    for x in (depth.astype(np.float16), torch.ones(8, 12, dtype=torch.float16), torch.ones(8, 12, dtype=torch.bfloat16)):
        with pytest.raises(ValueError, match="float16 depth maps are not supported"):
            fitting._map_of(x)
    dm, keep = fitting._map_of(depth.astype(np.float32)[::-1])  # rows backwards: copied
    assert dm.row_stride == 12 and dm.ptr == keep.ctypes.data
    scan = rng.uniform(-1, 1, (5, 6, 3))
    ref, view = _both_kinds(lambda x: fields(fitting._scan_of(x, (40, 50))[0]), scan, ("row_stride",))
    assert ref == dict(h=5, w=6, row_stride=18, pix_stride=3, chan_stride=1, img_h=40, img_w=50, dtype=1, on_device=0)
    assert view["row_stride"] == 33
    fake = FakeCuda(scan.astype(np.float32), 2)
    sm, keep = fitting._scan_of(fake, (40, 50), device=2)
    assert keep is fake and sm.ptr == fake.data_ptr() and fields(sm) == dict(ref, dtype=0, on_device=1)
    with pytest.raises(ValueError, match="^fitting: a scan lives on cuda:2, the call runs on cuda:0$"):
        fitting._scan_of(fake, (40, 50))
    with pytest.raises(ValueError, match="^fitting: a depth map lives on cuda:2, the call runs on cuda:1$"):
        fitting._map_of(FakeCuda(np.ones((8, 12), np.float32), 2), device=1)


def test_converter_of_features():
    fmap = np.random.default_rng(1).uniform(-1, 1, (5, 6, 3)).astype(np.float16)
    def conv(x):
        fm, shape, keep, on_device = features._feature_map(x, False, 0)
        assert fm.ptr == _native.address(keep) and on_device == fm.on_device
        return dict(fields(fm), shape=shape)

    ref, view = _both_kinds(conv, fmap, ("row_stride",))
    assert ref == dict(h=5, w=6, c=3, row_stride=18, pix_stride=3, chan_stride=1, dtype=_capi.PATCH_F16, on_device=0,
                       shape=(5, 6, 3))
    assert view["row_stride"] == 33
    fm, shape, keep, on_device = features._feature_map(FakeCuda(fmap, 0), True, 0)  # host=True: a host copy
    assert on_device == 0 and fields(fm) == {k: v for k, v in ref.items() if k != "shape"}
    with pytest.raises(ValueError, match="^features: the tensor lives on cuda:0, the call runs on cuda:1$"):
        features._feature_map(FakeCuda(fmap, 0), False, 1)
    with pytest.raises(ValueError, match="float16, float32 or float64"):
        features._feature_map(torch.ones(5, 6, 3, dtype=torch.bfloat16), False, 0)


def test_converter_of_optimize():
    texels = np.random.default_rng(2).uniform(-1, 1, (4, 5, 128)).astype(np.float32)
    conv = lambda x: (lambda t: dict(shape=t.shape, strides=t.strides, dtype=t.dtype, on_device=t.on_device,  # noqa: E731
                                     bits=t.keep.tobytes()))(optimize._texel_array(x, np.float16, False, "a map"))
    ref, view = _both_kinds(conv, texels)
    assert view == ref and ref["bits"] == texels.astype(np.float16).tobytes()
    assert (ref["shape"], ref["strides"], ref["dtype"], ref["on_device"]) == ((4, 5, 128), (640, 128, 1), "float16", 0)
    same = optimize._texel_array(texels, np.float32, False, "a map")
    assert same.keep is texels  # nothing to convert: shared
    with pytest.raises(ValueError, match=r"a map must be \(h, w, 128\), got shape \(4, 5, 3\)"):
        optimize._texel_array(texels[:, :, :3], np.float16, False, "a map")


def test_converters_of_matching():
    desc = np.random.default_rng(3).uniform(-1, 1, (3, 8))

    def gathered(rows, dim=8):
        keep, ptr, on_dev = matching._gather([rows], dim, 0)
        assert ptr.value == keep.ctypes.data and keep.flags.c_contiguous
        return dict(shape=keep.shape, dtype=keep.dtype.name, on_device=on_dev, bits=keep.tobytes())

    ref, view = _both_kinds(lambda x: gathered(matching._rows_of({"line_descriptors": x}, 0)), desc)
    assert view == ref == dict(shape=(3, 8), dtype="float32", on_device=0, bits=desc.astype(np.float32).tobytes())
    ends = np.ascontiguousarray(desc.T)  # limap keeps the endpoint descriptors as (dim, 2 M)
    ref, view = _both_kinds(lambda x: gathered(matching._rows_of(x, 1)), ends, ())
    assert ref["bits"] == desc.astype(np.float32).tobytes() and ref["shape"] == (3, 8)
    valid = np.ones((3, 1), bool)
    for v in (valid, torch.from_numpy(valid), valid[None]):
        ref, view = _both_kinds(lambda x: gathered(matching._sold2_parts([x, v], 1)[0]), ends)
        assert ref["bits"] == desc.astype(np.float32).tobytes() and matching._sold2_parts([ends, v], 1)[1].shape == (3, 1)
    assert matching._rows_of(np.zeros(0), 0).shape == (0, 0) and matching._rows_of(torch.zeros(0), 0).shape == (0, 0)
    for x in (np.zeros(3), torch.zeros(3)):
        with pytest.raises(ValueError, match=r"descriptors must be 2-D, got shape \(3,\)"):
            matching._rows_of(x, 0)
    with pytest.raises(ValueError, match="^matching: a descriptor array lives on cuda:0, the call runs on cuda:1$"):
        matching._gather([FakeCuda(desc.astype(np.float32), 0)], 8, 1)
    warp, cert = np.random.default_rng(4).uniform(-1, 1, (8, 12, 2)), np.ones((8, 12))
    for quad in ((warp, cert, warp, cert), tuple(torch.from_numpy(a) for a in (warp, cert, warp, cert)),
                 (_padded(warp), cert, torch.from_numpy(warp), _padded(cert))):
        out = matching._dense_maps(quad, 0)
        assert [a.shape for a in out] == [(8, 12, 2), (8, 12)] * 2
        assert all(isinstance(a, np.ndarray) and a.dtype == np.float32 and a.flags.c_contiguous for a in out)
        assert out[0].tobytes() == warp.astype(np.float32).tobytes()
    with pytest.raises(ValueError, match="^matching: a warp lives on cuda:0, the call runs on cuda:1$"):
        matching._dense_maps((FakeCuda(warp.astype(np.float32), 0),) * 4, 1)
    # CPU tensors of a type NumPy lacks end as host arrays too: nothing on the host may reach the call as a tensor,
    # whose address the device path would read
    bf = tuple(torch.from_numpy(a).to(torch.bfloat16) for a in (warp, cert, warp, cert))
    out = matching._dense_maps(bf, 0)
    assert all(isinstance(a, np.ndarray) and a.dtype == np.float32 and a.flags.c_contiguous for a in out)
    assert np.array_equal(out[0], bf[0].to(torch.float32).numpy()) and not any(_native.is_torch(a) for a in out)
    rows = matching._rows_of(torch.from_numpy(desc).to(torch.bfloat16), 0)
    assert isinstance(rows, np.ndarray) and rows.dtype == np.float32 and matching._gather([rows], 8, 0)[2] == 0
    assert isinstance(optimize._texel_array(torch.zeros(4, 5, 128, dtype=torch.bfloat16), np.float16, False, "m").keep,
                      np.ndarray)


def test_converters_of_line2d_and_undistortion():
    heat = np.random.default_rng(5).uniform(0, 1, (8, 12)).astype(np.float32)
    junc = np.array([[1.0, 2.0], [5.0, 9.0]])

    def prepared(h):
        jn, hm = line2d._prepare_image(junc, h, True, 0)
        assert jn.address == jn.keep.ctypes.data and hm.address == hm.keep.ctypes.data
        return dict(junc=(jn.shape, jn.dtype, jn.strides, jn.on_device, jn.keep.tobytes()),
                    heat=(hm.shape, hm.dtype, hm.strides, hm.on_device, hm.keep.tobytes()))

    ref, view = _both_kinds(prepared, heat)
    assert view == ref and ref["heat"] == ((8, 12), "float32", (12, 1), 0, heat.tobytes())
    assert ref["junc"] == ((2, 2), "float32", (2, 1), 0, junc.astype(np.float32).tobytes())
    assert line2d._prepare_image(np.zeros(0), heat, True, 0)[0].shape == (0, 2)
    with pytest.raises(ValueError, match="^line2d: the heatmap lives on cuda:0, the call runs on cuda:1$"):
        line2d.detect_scene(line2d.SHIPPED_CFG, [junc], [FakeCuda(heat, 0)], device=1)
    img = np.random.default_rng(6).integers(0, 255, (8, 12, 3), dtype=np.uint8)

    def rows(x):
        assert undistortion._check_image(x) == (8, 12, 3)
        r = undistortion._rows(_native.operand(x, host=False, device=0, who="undistortion", what="the tensor"), 3)
        return dict(shape=r.shape, strides=r.strides, on_device=r.on_device, bits=r.keep.tobytes())

    ref, view = _both_kinds(rows, img, ("strides",))
    assert ref["strides"] == (36, 3, 1) and view["strides"] == (51, 3, 1)  # rows further apart are read in place
    assert rows(img[:, ::-1])["strides"] == (36, 3, 1) and rows(torch.from_numpy(img).flip(1))["strides"] == (36, 3, 1)
    for x in (img.astype(np.int16), torch.from_numpy(img).to(torch.int16)):
        with pytest.raises(ValueError, match="an image must be uint8"):
            undistortion._check_image(x)


# ---- the small helpers ----------------------------------------------------------------------------------------------
def test_raise_host_error_and_module_timers():
    class Lib:
        def lt_fn_x_host_error(self):
            return b"bad \xff input"

        def lt_x_get_timers(self, h, out):
            assert h == 42
            for i in range(5):
                out[i] = i + 0.5
            return 0

    with pytest.raises(ValueError, match="^module: bad � input$"):
        _native.raise_host_error(Lib(), "lt_fn_x_host_error", "module: ")
    with pytest.raises(ValueError, match="^bad"):
        _native.raise_host_error(Lib(), "lt_fn_x_host_error")
    ctx = _capi.Context.__new__(_capi.Context)
    ctx.L, ctx.h, ctx.chk = Lib(), 42, lambda rc: None
    tm = ctx.module_timers("lt_x_get_timers", 5)
    assert isinstance(tm, np.ndarray) and tm.dtype == np.float64 and tm.tolist() == [0.5, 1.5, 2.5, 3.5, 4.5]
    ctx.h = None  # (nothing for __del__ to destroy)
    off, flat = _native.csr([np.ones((2, 4)), np.zeros((0, 4)), np.full((1, 4), 2.0)], 4)
    assert off.tolist() == [0, 2, 2, 3] and off.dtype == np.int64 and flat.shape == (3, 4) and flat.flags.c_contiguous
    off, flat = _native.csr([np.zeros((0, 2))], 2)
    assert off.tolist() == [0, 0] and flat.shape == (1, 2)
    assert [_native.host_threads(h, t) for h, t in ((False, None), (True, None), (False, 3), (True, 0))] == [None, 0, 3, 0]


def test_no_module_keeps_a_rule_of_its_own():
    """torch's pointers, device flags and synchronisation are spelled in _native.py (and in dist.py, whose exchange
    buffers are its own) and nowhere else in the package"""
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "limap_amd")
    files = sorted(glob.glob(os.path.join(root, "*.py")))
    assert len(files) > 20
    for path in files:
        text = open(path).read()
        assert not re.search(r"def _is_torch", text), path
        if os.path.basename(path) in ("_native.py", "dist.py"):
            continue
        for name in ("data_ptr(", ".is_cuda", "cuda.synchronize", "current_stream"):
            assert name not in text, (path, name)
