"""-m gpu: the global point-line association on the device (lt_kernels_assoc.hip) equals the host path
(lt_fn_assoc_host) bit for bit -- points, line parameters, vanishing points, both costs, iterations, CG iteration totals
and the code -- on the smallest shapes at which each kernel can go wrong.  Iteration caps of 30 or
less."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import assoc_scenes as sc
from limap_amd import _capi
from test_assoc_host import GOLDEN, load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    return _capi.Context()


def both(ctx, s, what="", **kw):
    cfg = sc.cfg_of(**kw)
    rc_d, d = sc.run_device(ctx, s, cfg)
    rc_h, h = sc.run_host(s, cfg, 8)
    assert rc_d == 0 and rc_h == 0, (what, rc_d, rc_h)
    for k in h:
        assert np.array_equal(d[k].view(np.uint8), h[k].view(np.uint8)), (what, k, d[k], h[k])
    return d


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "*.npz"))))
def test_device_reproduces_the_goldens(ctx, path):
    """against the recorded bytes, not against the twin"""
    s, cfg, want = load_golden(path)
    rc, d = sc.run_device(ctx, s, sc.cfg_of(**cfg))
    assert rc == 0 and set(d) == set(want)
    for k in d:
        assert np.array_equal(d[k], want[k]), (os.path.basename(path), k)


# the scenes of the CPU tests
@pytest.mark.parametrize("kw", [dict(), dict(parallel=True), dict(orth_exact=True), dict(identical=True)], ids=str)
def test_small_scenes(ctx, kw):
    d = both(ctx, sc.small_scene(0, **kw), kw, max_num_iterations=30, lw_vp_collinearity=0.5)
    assert d["cost"][1] < d["cost"][0] and d["cg_iterations"][0] > 0


def test_structured_scene(ctx):
    d = both(ctx, sc.structured_scene(n_cams=5, seed=3), max_num_iterations=30)
    assert d["cost"][1] < d["cost"][0]


# a vanishing point's wave64: its edge list around the wave and past two rounds of it
@pytest.mark.parametrize("n_edges", [63, 64, 65, 129])
def test_vp_with_many_line_edges(ctx, n_edges):
    s = sc.graph_scene(4, n_edges + 2, 2, pl=[(0, 0), (1, 1)], vl=[(0, n) for n in range(n_edges)] + [(1, n_edges)], seed=21)
    both(ctx, s, n_edges, max_num_iterations=6, min_num_images=1)


# a line's serial edge walk after its 16-lane R1 sums
@pytest.mark.parametrize("n_edges", [0, 1, 17])
def test_line_with_point_edges(ctx, n_edges):
    s = sc.graph_scene(20, 3, 1, pl=[(p, 0) for p in range(n_edges)] + [(19, 1)], vl=[(0, 1)], seed=22)
    both(ctx, s, n_edges, max_num_iterations=8, min_num_images=1)


# the chunks of the dot products: unknown counts around 256, and more chunks than the lanes of the wave that sums them
@pytest.mark.parametrize("n_points", [255 - 7, 256 - 7, 257 - 7])
def test_unknown_counts_around_a_chunk(ctx, n_points):
    s = sc.graph_scene(n_points, 5, 2, pl=[(p, p % 5) for p in range(0, n_points, 3)], vl=[(0, 0), (1, 1), (1, 2)], seed=23,
                       orth=[(0, 1)])
    assert n_points + 5 + 2 in (255, 256, 257)
    both(ctx, s, n_points, max_num_iterations=5, min_num_images=1)


def test_more_than_64_chunks(ctx):
    n = 64 * 256 + 40
    s = sc.graph_scene(n, 6, 2, pl=[(p, p % 6) for p in range(0, n, 5)], vl=[(0, 0), (1, 1)], seed=24, n_cams=2)
    d = both(ctx, s, max_num_iterations=3, min_num_images=1)
    assert d["iterations"][0] == 3


# every constant_* switch, point-line only and VP only
@pytest.mark.parametrize("kw", [dict(constant_point=1), dict(constant_line=1), dict(constant_vp=1),
                                dict(constant_point=1, constant_line=1), dict(constant_line=1, constant_vp=1),
                                dict(constant_point=1, constant_line=1, constant_vp=1),
                                dict(enable_vpline=0), dict(enable_pointline=0), dict(lw_point=0.0),
                                dict(lw_pointline_association=0.0, lw_vpline_association=0.0)], ids=str)
def test_switches(ctx, kw):
    both(ctx, sc.structured_scene(n_cams=4, seed=5), kw, max_num_iterations=12, **kw)


# both early ends
def test_zero_gradient_end(ctx):
    d = both(ctx, sc.stationary_vp_scene(), **sc.STATIONARY)
    assert d["code"][0] == 2 and d["iterations"][0] == 0


def test_iteration_cap_zero_and_no_residuals(ctx):
    s = sc.structured_scene(n_cams=4, seed=5)
    d = both(ctx, s, max_num_iterations=0)
    assert d["code"][0] == 0 and d["iterations"][0] == 0 and d["cost"][0] == d["cost"][1]
    d = both(ctx, s, constant_point=1, constant_line=1, enable_vpline=0)
    assert d["code"][0] == 7


def test_start_that_is_not_finite_in_cost(ctx):
    """a point in a camera's plane: the cost at the start is not finite, code 6, nothing moves"""
    d = both(ctx, sc.depth_zero_scene(), max_num_iterations=5)
    assert d["code"][0] == 6 and d["iterations"][0] == 0


def test_rejected_cg_attempt(ctx):
    """a cap of one CG iteration at a tiny eta: attempts whose steps the ratio test rejects run through the device"""
    s = sc.structured_scene(n_cams=4, seed=6, struct_sigma=0.2, vp_sigma=0.3)
    cfg = dict(max_num_iterations=25, cg_max_iterations=1, cg_eta=1e-12)
    d = both(ctx, s, **cfg)
    _, _, tr = sc.run_host(s, sc.cfg_of(**cfg), 1, trace=64)
    assert (tr["rec"][:, 2] == 0).any(), "no attempt was rejected"
    assert d["iterations"][0] == 25


@pytest.mark.parametrize("name", ["breakdown", "pivot"])
def test_failed_linear_solves(ctx, name):
    """every attempt's linear solve fails -- at p.Ap in k_as_alpha in the middle of a batch, or at a pivot in k_as_precond
    -- so k_as_backsub and k_as_cost return on the flag and k_as_decide rejects over stale totals: the same rejected steps,
    radii and end as the host twin, at two batch sizes"""
    import test_assoc_host as th
    _, s, kw = next(c for c in th.failing_solves() if c[0] == name)
    d = both(ctx, s, name, **kw)
    assert (int(d["iterations"][0]), int(d["code"][0]), int(d["cg_iterations"][0])) == (15, 1, 0) and d["cost"][0] == d["cost"][1]
    rc, e = sc.run_device(ctx, s, sc.cfg_of(poll_interval=1, cg_batch=1, **kw))
    assert rc == 0 and sc.same_bits(d, e)


def test_repeated_runs_and_batch_sizes(ctx):
    s = sc.structured_scene(n_cams=4, seed=7)
    base = both(ctx, s, max_num_iterations=20, cg_eta=1e-6)
    assert base["cg_iterations"][0] > 2 * base["iterations"][0]  # more than one batch of two CG iterations per attempt
    # the CG iterations of every attempt (host twin): with kernel_timers the record is read after every batch, and an
    # attempt of n iterations takes max(1, ceil(n / cg_batch)) batches
    _, _, tr = sc.run_host(s, sc.cfg_of(max_num_iterations=20, cg_eta=1e-6), 1, trace=64)
    cg = tr["rec"][:, 5].astype(np.int64)
    assert len(cg) == base["iterations"][0]
    # kernel_timers at cg_batch 1 and 64: 14 and 329 events, the smallest and the largest count of the event holder
    for kw in (dict(), dict(poll_interval=1, cg_batch=1), dict(poll_interval=3, cg_batch=2), dict(poll_interval=7, cg_batch=64),
               dict(kernel_timers=1), dict(kernel_timers=1, cg_batch=1), dict(kernel_timers=1, cg_batch=64)):
        rc, d = sc.run_device(ctx, s, sc.cfg_of(max_num_iterations=20, cg_eta=1e-6, **kw))
        assert rc == 0 and sc.same_bits(d, base), kw
        if kw.get("kernel_timers"):
            tm = np.zeros(20)
            ctx.chk(ctx.L.lt_assoc_get_timers(ctx.h, _capi.ptr(tm, C.c_double)))
            batch = kw.get("cg_batch", 4)  # kAsCgBatchDefault
            assert np.isfinite(tm[4:17]).all() and (tm[4:17] >= 0.0).all(), (kw, tm)
            assert tm[3] == np.maximum(1, -(-cg // batch)).sum(), (kw, tm[3], cg)


def test_python_surface_on_the_device(ctx):
    """GlobalAssociator through the device equals its host_threads path"""
    import test_assoc_host as th
    a = th.associator_of(sc.structured_scene(n_cams=4, seed=8), host_threads=None, max_num_iterations=15)
    b = th.associator_of(sc.structured_scene(n_cams=4, seed=8), host_threads=2, max_num_iterations=15)
    for ka, kb in zip(sorted(a.GetOutputPoints().items()), sorted(b.GetOutputPoints().items())):
        assert ka[0] == kb[0] and np.array_equal(ka[1], kb[1])
    for k, v in a.GetOutputVPs().items():
        assert np.array_equal(v, b.GetOutputVPs()[k])
    la, lb = a.GetOutputLineTracks(), b.GetOutputLineTracks()
    for k in la:
        assert np.array_equal(la[k].line.as_array(), lb[k].line.as_array())
