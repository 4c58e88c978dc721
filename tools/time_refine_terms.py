"""Times the line refinement with the VP and the heatmap term (limap_amd.optimize) on a scene in
the shape of upstream's refinement runner: 100 images with 480x640 FP16 heatmaps (Gaussian ridges along the true
projections), N_TRACKS (3000) tracks of 2..40 supports from tests/refine_scenes.make_tracks, 10 samples.  Warm process
(two untimed calls per configuration), median / min / max of ten calls: the device time of k_refine_lm_terms and of
k_refine_lm (HIP events, lt_refine_get_timers[3]), the upload of the heatmaps (host clock around
lt_refine_set_heatmaps, which ends in a synchronise), lt_fn_refine_host_terms on 16 threads, checked to give the same
bits.  Writes profiles/refine_terms_timing.json (OUT) and prints it.

usage: python tools/time_refine_terms.py
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import refine_scenes as rs
import refine_terms_scenes as ts
from limap_amd import _capi, synthetic as syn

N_TRACKS, N_VIEWS, H, W = int(os.environ.get("N_TRACKS", 3000)), 100, 480, 640
t0 = time.time()
s = rs.make_tracks(N_TRACKS, n_views=N_VIEWS, seed=3, noise_px=0.5, init_sigma=0.01)
sc = np.array([W / 800.0, H / 600.0])
s["k"] = np.ascontiguousarray(s["k"] * np.array([sc[0], sc[1], sc[0], sc[1]]))
s["l2d"] = np.ascontiguousarray(s["l2d"] * np.array([sc[0], sc[1], sc[0], sc[1]]))
s["hw"] = np.tile(np.array([H, W], np.int32), (N_VIEWS, 1))
idx = {int(i): k for k, i in enumerate(s["img_ids"])}
rng = np.random.default_rng(0)
heat = {int(i): np.zeros((H, W), np.float32) for i in s["img_ids"]}
flag, vp3 = [], []
T = len(s["off"]) - 1
for n in range(T):
    d = s["gt6"][n, 3:] - s["gt6"][n, :3]
    for j in range(int(s["off"][n]), int(s["off"][n + 1])):
        v = idx[int(s["img"][j])]
        K3 = np.array([[s["k"][v, 0], 0, s["k"][v, 2]], [0, s["k"][v, 1], s["k"][v, 3]], [0, 0, 1.0]])
        R = syn.quat_to_rot(s["q"][v])
        vp = K3 @ R @ d
        flag.append(int(rng.random() < 0.7)); vp3.append(vp / np.linalg.norm(vp))
        # the ridge of the true projection inside the support's padded box
        xa = ts._project(s["k"][v], s["q"][v], s["t"][v], s["gt6"][n, :3]); xb = ts._project(s["k"][v], s["q"][v], s["t"][v], s["gt6"][n, 3:])
        nrm = np.array([xa[1] - xb[1], xb[0] - xa[0]]); nrm /= np.linalg.norm(nrm)
        x0, x1 = np.sort(s["l2d"][j, [0, 2]]); y0, y1 = np.sort(s["l2d"][j, [1, 3]])
        c0, c1 = int(max(0, x0 - 8)), int(min(W, x1 + 9)); r0, r1 = int(max(0, y0 - 8)), int(min(H, y1 + 9))
        if c1 <= c0 or r1 <= r0:
            continue
        yy, xx = np.mgrid[r0:r1, c0:c1]
        dd = nrm[0] * xx + nrm[1] * yy - nrm @ xa
        a = heat[int(s["img"][j])]
        a[r0:r1, c0:c1] = np.maximum(a[r0:r1, c0:c1], np.exp(-dd * dd / 8.0))
s["vp_flag"], s["vp3"], s["heatmaps"] = np.array(flag, np.int32), np.array(vp3), heat
tex = ts.texels(s, np.float16)
K = np.diff(s["off"])
print(f"scene: {T} tracks, {int(s['off'][-1])} supports ({K.min()}..{K.max()} per track), {N_VIEWS} heatmaps of {H}x{W} FP16, "
      f"built in {time.time() - t0:.1f} s", flush=True)

L = _capi.load_library()
ctx = _capi.Context()
cfg = ts.cfg_struct(L)
res = dict(tracks=T, supports=int(s["off"][-1]), images=N_VIEWS, h=H, w=W)


def med(xs):
    xs = sorted(xs)
    return dict(median=xs[len(xs) // 2], min=xs[0], max=xs[-1], n=len(xs))


up = []
for _ in range(6):
    t = time.perf_counter()
    assert L.lt_refine_set_heatmaps(ctx.h, *ts.heatmap_args(tex), 0) == 0
    up.append((time.perf_counter() - t) * 1e3)
res["heatmap_upload_ms"] = med(up[1:])
tm = np.zeros(4)


def device(terms_kw, reps=10, warm=2):
    terms = ts.terms_struct(L, **terms_kw)
    out, r = [], None
    for k in range(warm + reps):
        rc, r = ts.run_device(ctx, s, cfg, terms)
        assert rc == 0, L.lt_last_error(ctx.h)
        assert L.lt_refine_get_timers(ctx.h, ts.p(tm)) == 0
        if k >= warm:
            out.append(float(tm[3]))
    return med(out), r


res["k_refine_lm_ms"], r_geo = device(dict())
res["k_refine_lm_terms_all_ms"], r_all = device(dict(use_vp=1, use_heatmap=1))
res["k_refine_lm_terms_heatmap_ms"], _ = device(dict(use_heatmap=1))
res["k_refine_lm_terms_vp_ms"], _ = device(dict(use_vp=1))
res["iterations_all"] = dict(median=float(np.median(r_all["iterations"])), max=int(r_all["iterations"].max()))
res["iterations_geometric"] = dict(median=float(np.median(r_geo["iterations"])), max=int(r_geo["iterations"].max()))
res["codes_all"] = np.bincount(r_all["codes"], minlength=7).tolist()
host = []
terms = ts.terms_struct(L, use_vp=1, use_heatmap=1)
for _ in range(3):
    t = time.perf_counter()
    rc, rh = ts.run_host(L, s, cfg, terms, tex, threads=16)
    host.append((time.perf_counter() - t) * 1e3)
    assert rc == 0
res["host_terms_16_threads_ms"] = med(host)
res["device_equals_host"] = bool(all(np.array_equal(rh[k], r_all[k], equal_nan=True) for k in rh))
out = os.environ.get("OUT", os.path.join(ROOT, "profiles", "refine_terms_timing.json"))
with open(out, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
