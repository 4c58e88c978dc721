"""-m gpu: the geometric line refinement on the device (lt_kernels_refine.hip) equals the host path
(lt_fn_refine_host) bit for bit -- parameters, segments, costs, iterations, termination codes -- on every fixture of
tests/test_refine_host.py and on a scene-sized run; TrackSet.refine equals lt_refine_arrays on the downloaded tracks;
two runs and a permuted track order give identical per-track results."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import refine_scenes as rs
from helpers import run_product
from limap_amd import _capi, synthetic as syn
from test_refine_host import GOLDEN, REFINEMENT_CFG, _cut_scene, _linetracks, cfg_of, run_host

pytestmark = pytest.mark.gpu
p = _capi.ptr
KEYS = ("params", "segments", "cost", "iterations", "codes")


def run_device(ctx, s, cfg):
    from limap_amd import optimize
    cams = (s["img_ids"], s["k"], s["q"], s["t"])
    csr = (s["line6"], s["off"], s["img"], s["l2d"], s["l3d"])
    return optimize.refine_arrays(cams, csr, cfg, ctx=ctx)


def same(a, b, what):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), (what, k, np.flatnonzero(np.any(np.atleast_2d(a[k].T != b[k].T), 0))[:5])


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    return _capi.Context()


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "*.npz"))))
def test_device_reproduces_the_goldens(gpu_lib, ctx, path):
    z = np.load(path)
    s = {k: np.ascontiguousarray(z[k]) for k in ("img_ids", "k", "q", "t", "line6", "off", "img", "l2d", "l3d")}
    c = cfg_of(gpu_lib, **{k[4:]: z[k].item() for k in z.files if k.startswith("cfg_")})
    r = run_device(ctx, s, c)
    same(r, {k: z["out_" + k] for k in KEYS}, os.path.basename(path))


@pytest.mark.parametrize("scene_kw,cfg_kw", [
    (dict(n_tracks=200, seed=12, noise_px=0.1, init_sigma=0.002), dict(max_num_iterations=200)),
    (dict(n_tracks=200, seed=11, noise_px=0.5, init_sigma=0.02), dict(max_num_iterations=200)),
    (dict(n_tracks=60, seed=1), dict()),
    (dict(n_tracks=40, seed=31, k_max=90, n_views=50), dict(max_num_iterations=200)),  # K above the group width
    (dict(n_tracks=40, seed=32), dict(constant_line=1)),
    (dict(n_tracks=60, seed=33), dict(min_num_images=6, max_num_iterations=200)),      # mixed constant / free
    (dict(n_tracks=40, seed=34), dict(num_outliers_aggregator=0, geometric_alpha=3.0)),
])
def test_device_equals_host_bit_for_bit(gpu_lib, ctx, scene_kw, cfg_kw):
    s = rs.make_tracks(**scene_kw)
    c = cfg_of(gpu_lib, **cfg_kw)
    rc, h = run_host(gpu_lib, s, c, 8)
    assert rc == 0
    same(run_device(ctx, s, c), h, str(scene_kw))
    if scene_kw.get("k_max", 0) > 16:
        assert np.diff(s["off"]).max() > 16


def test_device_equals_host_on_edge_shapes(gpu_lib, ctx):
    s = _cut_scene()  # ties in the cut
    kmin = int(np.diff(s["off"]).min())
    for n_out in (0, 2 * kmin - 1):
        c = cfg_of(gpu_lib, num_outliers_aggregator=n_out, max_num_iterations=200)
        same(run_device(ctx, s, c), run_host(gpu_lib, s, c)[1], f"num_outliers {n_out}")
    # the edge fixtures (line through the origin: the fallback basis of rf_minimal in k_refine_prep, wvec = (1, 0), the
    # |x| kink, parallel / perpendicular / clamped supports, two supports in one image) as one-track scenes
    e = rs.edge_scene()
    for kw in (dict(min_num_images=1, max_num_iterations=200, num_outliers_aggregator=0), dict(num_outliers_aggregator=1)):
        c = cfg_of(gpu_lib, **kw)
        same(run_device(ctx, e, c), run_host(gpu_lib, e, c)[1], f"edge {kw}")
    # tracks of one image with a single support each
    one = rs.make_tracks(8, seed=35)
    keep = [int(one["off"][n]) for n in range(8)]
    one = dict(one, off=np.arange(9, dtype=np.int64), img=np.ascontiguousarray(one["img"][keep]),
               l2d=np.ascontiguousarray(one["l2d"][keep]), l3d=np.ascontiguousarray(one["l3d"][keep]))
    c = cfg_of(gpu_lib, min_num_images=1, num_outliers_aggregator=0, max_num_iterations=50)
    same(run_device(ctx, one, c), run_host(gpu_lib, one, c)[1], "single support")
    with pytest.raises(ValueError, match="num_outliers"):
        run_device(ctx, one, cfg_of(gpu_lib, num_outliers_aggregator=2))
    bad = dict(one, img=one["img"] + 10 ** 6)
    with pytest.raises(ValueError, match="not in the collection"):
        run_device(ctx, bad, c)


def _scene_tracks(n_views, n_segs, nn, seed):
    from limap_amd import merging
    sc = syn.make_scene(n_views=n_views, n_segs=n_segs, n_neighbors=nn, seed=seed)
    T = run_product(sc, syn.default_triangulation_cfg())
    T.ComputeLineTracks()
    return sc, T, merging.TrackSet.from_triangulator(T)


def _csr_of(sc, a):
    return dict(img_ids=sc.img_ids.astype(np.int32), k=np.ascontiguousarray(sc.kvec), q=np.ascontiguousarray(sc.qvec),
                t=np.ascontiguousarray(sc.tvec), line6=np.ascontiguousarray(a["line"][:, :6]), off=a["off"],
                img=np.ascontiguousarray(a["image_ids"]), l2d=np.ascontiguousarray(a["line2d"]),
                l3d=np.ascontiguousarray(a["line3d"][:, :6]))


def test_scene_sized_run_equals_host(gpu_lib, ctx):
    """100 views x 500 segments, triangulated by this package"""
    sc, T, ts = _scene_tracks(100, 500, 20, 0)
    s = _csr_of(sc, ts.arrays())
    assert len(s["line6"]) > 1000
    c = cfg_of(gpu_lib, max_num_iterations=200)
    d = run_device(ctx, s, c)
    same(d, run_host(gpu_lib, s, c, 16)[1], "scene")
    assert np.all(d["cost"][:, 1] <= d["cost"][:, 0])
    print("scene:", len(s["line6"]), "tracks", len(s["img"]), "supports, codes", np.bincount(d["codes"], minlength=6),
          "iterations max", d["iterations"].max(), d["timers"])


def test_trackset_refine_equals_arrays_on_the_downloaded_tracks(gpu_lib, ctx):
    from test_gpu_postprocess import F2D, REMERGE_LINKER
    sc, T, ts = _scene_tracks(30, 200, 10, 0)
    ts.filter_by_reprojection(F2D["th_angular_2d"], F2D["th_perp_2d"]).remerge(REMERGE_LINKER)
    ts.filter_by_reprojection(F2D["th_angular_2d"], F2D["th_perp_2d"])
    ts.filter_by_sensitivity(F2D["th_sv_angular_3d"], F2D["th_sv_num_supports"])
    ts.filter_by_overlap(F2D["th_overlap"], F2D["th_overlap_num_supports"])
    before = ts.arrays()
    assert len(before["off"]) - 1 > 20
    ts.refine(dict(REFINEMENT_CFG), max_num_iterations=200)
    after = ts.arrays()
    r = run_device(ctx, _csr_of(sc, before), cfg_of(gpu_lib, max_num_iterations=200))
    same(ts.refine_result, r, "TrackSet.refine")
    assert np.array_equal(after["line"][:, :6], r["segments"]) and np.all(after["line"][:, 6] == -1.0)
    for k in ("off", "image_ids", "line_ids", "line2d", "line3d"):
        assert np.array_equal(before[k], after[k]), k
    # the LineTrack-list surface on the device gives the same lines
    from limap_amd import optimize
    from limap_amd.base import ImageCollection
    ic = ImageCollection.from_arrays(sc.img_ids, sc.kvec, sc.qvec, sc.tvec)
    s = _csr_of(sc, before)
    eng = optimize.solve_line_bundle_adjustment(dict(REFINEMENT_CFG), ic, _linetracks(s), max_num_iterations=200)
    m = eng.GetOutputLineTracks(num_outliers=2)
    assert np.array_equal(np.array([np.concatenate([m[n].line.start, m[n].line.end]) for n in sorted(m)]), r["segments"])


def test_determinism_two_runs_and_a_permuted_track_order(gpu_lib, ctx):
    s = rs.make_tracks(150, seed=41, k_max=50)
    c = cfg_of(gpu_lib, max_num_iterations=200)
    a = run_device(ctx, s, c)
    same(run_device(ctx, s, c), a, "second run")
    T = len(s["line6"])
    perm = np.random.default_rng(0).permutation(T)
    cnt = np.diff(s["off"])[perm]
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    idx = np.concatenate([np.arange(s["off"][n], s["off"][n + 1]) for n in perm])
    sp = dict(s, line6=np.ascontiguousarray(s["line6"][perm]), off=off, img=np.ascontiguousarray(s["img"][idx]),
              l2d=np.ascontiguousarray(s["l2d"][idx]), l3d=np.ascontiguousarray(s["l3d"][idx]))
    b = run_device(ctx, sp, c)
    same(b, {k: a[k][perm] for k in KEYS}, "permuted")
