"""The timer arrays of the modules around the triangulation core (lt_*_get_timers), after one smallest-shape call each:
every slot finite and non-negative; every slot that include/limap_amd.h documents as device milliseconds from HIP events
positive, and no larger than the host wall-clock slot of the same call that the header says encloses it.  Guards the
event indices of the modules' shared event timing (lt_hostutil.h)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = [20.0, 20.0, 8.0, 8.0]  # fx, fy, cx, cy of a 16 x 16 image
DEPTH = 2.0


def _p(a, t=C.c_double):
    return a.ctypes.data_as(C.POINTER(t))


def _timers(ctx, name, n=4):
    out = np.full(n, np.nan)
    assert getattr(ctx.L, name)(ctx.h, _p(out)) == 0
    print(name, out.tolist())
    assert np.all(np.isfinite(out)) and np.all(out >= 0.0), (name, out)
    return out


def _device_within(tm, device_slot, wall_slot):
    assert 0.0 < tm[device_slot] <= tm[wall_slot], (device_slot, wall_slot, tm)


def _backproject(seg2d, tx):
    """the 3D segments (n, 6) that a camera at rotation I, translation (tx, 0, 0) sees as seg2d at depth DEPTH"""
    out = np.zeros((len(seg2d), 6))
    for e in (0, 1):
        out[:, 3 * e + 0] = (seg2d[:, 2 * e] - K[2]) / K[0] * DEPTH - tx
        out[:, 3 * e + 1] = (seg2d[:, 2 * e + 1] - K[3]) / K[1] * DEPTH
        out[:, 3 * e + 2] = DEPTH
    return out


def _project(seg3d, tx):
    out = np.zeros((len(seg3d), 4))
    for e in (0, 1):
        out[:, 2 * e] = K[0] * (seg3d[:, 3 * e] + tx) / seg3d[:, 3 * e + 2] + K[2]
        out[:, 2 * e + 1] = K[1] * seg3d[:, 3 * e + 1] / seg3d[:, 3 * e + 2] + K[3]
    return out


def _two_view_context(n_segs):
    """2 images of n_segs horizontal segments each: the same 3D lines seen from two cameras 0.1 apart"""
    from limap_amd import _capi
    y = np.linspace(2.0, 13.0, n_segs)
    seg0 = np.stack([np.full(n_segs, 2.0), y, np.full(n_segs, 13.0), y], 1)
    seg3d = _backproject(seg0, 0.0)
    seg1 = _project(seg3d, 0.1)
    ctx = _capi.Context()
    kvec = np.array([K, K]); qvec = np.array([[1.0, 0, 0, 0]] * 2); tvec = np.array([[0.0, 0, 0], [0.1, 0, 0]])
    ctx.init([0, 1], kvec, qvec, tvec, [0, n_segs, 2 * n_segs], np.concatenate([seg0, seg1], 0))
    return ctx, np.ascontiguousarray(np.concatenate([seg3d, seg3d], 0))


def test_fit_timers(gpu_lib):
    """lt_fit_get_timers: [0] device ms of the fit kernel, [1] device ms of the depth-map upload, [2] host ms of the call"""
    from limap_amd import _capi
    ctx, _ = _two_view_context(8)
    depth = [np.full((16, 16), DEPTH, np.float32) for _ in range(2)]
    maps = (_capi.LtDepthMap * 2)(*[_capi.LtDepthMap(C.c_void_p(d.ctypes.data), 16, 16, 16, 0, 0) for d in depth])
    cfg = _capi.LtFitConfig()
    ctx.L.lt_fit_config_default(C.byref(cfg))
    seg = np.zeros((16, 6)); status = np.zeros(16, np.int32)
    ctx.chk(ctx.L.lt_fit_segs(ctx.h, 0, 2, maps, C.byref(cfg), _p(seg), _p(status, C.c_int32), None))
    tm = _timers(ctx, "lt_fit_get_timers")
    _device_within(tm, 0, 2)
    _device_within(tm, 1, 2)
    assert tm[3] == 1
    ctx.close()


def test_merge_timers(gpu_lib):
    """lt_merge_get_timers: [0] device ms of the pair kernels, [1] host ms of the whole call"""
    ctx, seg3d = _two_view_context(4)
    seg_off = np.array([0, 4, 8], np.int64); nb_off = np.array([0, 1, 2], np.int64); nb = np.array([1, 0], np.int32)
    out = C.c_void_p()
    ctx.chk(ctx.L.lt_merge_to_tracks(ctx.h, _p(seg_off, C.c_int64), _p(seg3d), _p(nb_off, C.c_int64), _p(nb, C.c_int32),
                                     C.byref(ctx.cfg), 5.0, C.byref(out)))
    ctx.L.lt_ts_destroy(out)
    tm = _timers(ctx, "lt_merge_get_timers")
    _device_within(tm, 0, 1)
    assert tm[2] == 1
    ctx.close()


def test_eval_timers(gpu_lib):
    """lt_eval_get_timers: [0] device ms of the call's kernels, [1] host ms of the call"""
    from limap_amd import _capi
    rng = np.random.default_rng(0)
    pts = rng.uniform(-1.0, 1.0, (64, 3))
    lines = rng.uniform(-1.0, 1.0, (4, 6))
    ctx = _capi.Context()
    pcd = C.c_void_p()
    ctx.chk(ctx.L.lt_pcd_build(ctx.h, C.c_void_p(pts.ctypes.data), 64, 1, 0, None, C.byref(pcd)))
    _device_within(_timers(ctx, "lt_eval_get_timers"), 0, 1)
    dists = np.zeros((4, 10))
    ctx.chk(ctx.L.lt_pcd_line_samples(ctx.h, pcd, _p(lines), 4, 0, 10, None, 0, 0, _p(dists), None))
    _device_within(_timers(ctx, "lt_eval_get_timers"), 0, 1)
    ctx.L.lt_pcd_free(pcd)
    ctx.close()


def test_vp_timers(gpu_lib):
    """lt_vp_get_timers: host ms of [1] the kernels; device ms of [4] the preference kernel, [5] the clustering kernel"""
    from limap_amd import _capi
    lines = []
    for vp, starts in (((2000.0, 100.0), [(10.0, 15.0 * k) for k in range(12)]),
                       ((100.0, -2000.0), [(15.0 * k, 190.0) for k in range(12)])):
        for x, y in starts:  # 60 px towards the vanishing point: above the default min_length of 40
            d = np.array([vp[0] - x, vp[1] - y])
            d = 60.0 * d / np.linalg.norm(d)
            lines.append([x, y, x + d[0], y + d[1]])
    lines = np.array(lines)
    off = np.array([0, 24], np.int64)
    cfg = _capi.LtVpConfig()
    ctx = _capi.Context()
    ctx.L.lt_vp_config_default(C.byref(cfg))
    ctx.chk(ctx.L.lt_vp_detect(ctx.h, 1, _p(off, C.c_int64), _p(lines), C.byref(cfg), None))
    tm = _timers(ctx, "lt_vp_get_timers", 6)
    _device_within(tm, 4, 1)
    _device_within(tm, 5, 1)
    ctx.close()


def test_refine_timers(gpu_lib):
    """lt_refine_get_timers: host ms of [1] the kernels; device ms of [3] k_refine_lm"""
    from limap_amd import _capi
    tx = [0.0, 0.1, 0.2]
    line6 = _backproject(np.array([[2.0, 4.0, 13.0, 5.0], [3.0, 12.0, 12.0, 9.0]]), 0.0)
    img = np.array([0, 1, 2, 0, 1, 2], np.int32)
    l2d = np.concatenate([_project(line6[n:n + 1], t) for n in range(2) for t in tx], 0) + 0.25
    l3d = np.repeat(line6, 3, 0)
    off = np.array([0, 3, 6], np.int64)
    ids = np.array([0, 1, 2], np.int32)
    kvec = np.array([K] * 3); qvec = np.array([[1.0, 0, 0, 0]] * 3); tvec = np.array([[t, 0.0, 0.0] for t in tx])
    cfg = _capi.LtRefineConfig()
    ctx = _capi.Context()
    ctx.L.lt_refine_config_default(C.byref(cfg))
    cfg.min_num_images = 3
    ctx.chk(ctx.L.lt_refine_arrays(ctx.h, 3, _p(ids, C.c_int32), _p(kvec), _p(qvec), _p(tvec), 2, _p(line6),
                                   _p(off, C.c_int64), _p(img, C.c_int32), _p(l2d), _p(l3d), C.byref(cfg)))
    tm = _timers(ctx, "lt_refine_get_timers")
    _device_within(tm, 3, 1)
    ctx.close()


def test_bipartite_and_matching_timers(gpu_lib):
    """lt_bpt_get_timers, lt_match_get_timers: host wall-clock in every slot"""
    from limap_amd import _capi
    ctx = _capi.Context()
    lines = np.array([[0.0, 0.0, 10.0, 0.0], [5.0, -5.0, 5.0, 5.0], [0.0, 4.0, 10.0, 4.0]])
    pts = np.array([[5.0, 0.5], [20.0, 20.0]])
    loff = np.array([0, 3], np.int64); poff = np.array([0, 2], np.int64)
    cfg = _capi.LtBptConfig()
    ctx.L.lt_bpt_config_default(C.byref(cfg))
    ctx.chk(ctx.L.lt_bpt_associate(ctx.h, 1, _p(loff, C.c_int64), _p(lines), _p(poff, C.c_int64), _p(pts), C.byref(cfg),
                                   None))
    _timers(ctx, "lt_bpt_get_timers")
    sizes = np.zeros(4, np.int64)
    ctx.chk(ctx.L.lt_bpt_junctions(ctx.h, 1, _p(loff, C.c_int64), _p(lines), _p(poff, C.c_int64), _p(pts), C.byref(cfg),
                                   _p(sizes, C.c_int64)))
    _timers(ctx, "lt_bpt_get_timers")
    desc = np.random.default_rng(1).standard_normal((8, 8)).astype(np.float32)
    doff = np.array([0, 4, 8], np.int64); pair_off = np.array([0, 1, 1], np.int64); nb = np.array([1], np.int32)
    mcfg = _capi.LtMatchConfig(0, 2, 0, 0)
    ctx.chk(ctx.L.lt_match_scene(ctx.h, 2, _p(doff, C.c_int64), C.c_void_p(desc.ctypes.data), 8, _p(pair_off, C.c_int64),
                                 _p(nb, C.c_int32), C.byref(mcfg), None))
    _timers(ctx, "lt_match_get_timers")
    ctx.close()
