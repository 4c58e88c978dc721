"""Times the line refinement with the feature-consistency term (limap_amd.optimize) on a scene of
upstream's default shape: n_samples_feature 100, N_TRACKS (64) tracks of 4 to 8 images out of 12 of 192x256 with 128
channels (tests/refine_feature_scenes.make_scene), the patches from features.extract_track_patches at range_perp 16,
max_num_iterations 100.  Warm process (one untimed call per configuration), median / min / max of five calls, for the
patch and the map form with binary16 and float texels: the device time of k_refine_lm_feat (HIP events,
lt_refine_get_timers[3]) and the host milliseconds of the whole native call; the same tracks through
lt_fn_refine_host_feature on 16 threads, checked to give the same bits; as yardsticks k_refine_lm (geometric term alone)
and k_refine_lm_terms with the heatmap term on the same tracks.  Writes profiles/refine_feature_timing.json (OUT) and
prints it.

usage: python tools/time_refine_feature.py
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import refine_feature_scenes as fs
from limap_amd import features, optimize

N_TRACKS, HW, N_CAMS = int(os.environ.get("N_TRACKS", 64)), (192, 256), 12
REPS = int(os.environ.get("REPS", 5))
t0 = time.time()
rng = np.random.default_rng(7)
s = fs.make_scene(counts=tuple(int(c) for c in rng.integers(4, 9, N_TRACKS)), seed=7, n_cams=N_CAMS, hw=HW, noise_px=0.05,
                  init_sigma=0.002, map_dtype=np.float32)
tracks, ic = fs.tracks_of(s), fs.imagecols(s)
patch_cfg = dict(patch=dict(k_stretch=1.0, t_stretch=10, range_perp=16), channels=128)
res = dict(tracks=N_TRACKS, images=N_CAMS, h=HW[0], w=HW[1], n_samples_feature=100, max_num_iterations=100,
           supports=int(s["off"][-1]))
print(f"scene built in {time.time() - t0:.1f} s", flush=True)


def med(xs):
    xs = sorted(xs)
    return dict(median=xs[len(xs) // 2], min=xs[0], max=xs[-1], n=len(xs))


def timed(rf, form, src, host_threads=None, reps=REPS, warm=1, **kw):
    kern, call, r = [], [], None
    for k in range(warm + reps):
        t = time.perf_counter()
        r = fs.run(s, rf, form, src, host_threads=host_threads, **kw)
        ms = (time.perf_counter() - t) * 1e3
        if k >= warm:
            call.append(ms)
            if r["timers"] is not None:
                kern.append(r["timers"]["lm_device_ms"])
    return (med(kern) if kern else None), med(call), r


for dt in ("float16", "float32"):
    rf = fs.refine_cfg(n_samples_feature=100, max_num_iterations=100, dtype=dt)
    pat = features.extract_track_patches(dict(patch_cfg, dtype=dt), tracks, ic, s["maps"], host=True, dtype=dt)
    maps = optimize.FeatureMaps(s["maps"], dt)
    if dt == "float16":
        res["patch_texels_mib"] = sum(p.array.nbytes for p in pat.values()) / 2 ** 20
        res["patch_rows"] = med([p.array.shape[0] for p in pat.values()])
    for form, src in (("patch", pat), ("map", maps)):
        kern, call, r = timed(rf, form, src)
        res[f"{form}_{dt}"] = dict(k_refine_lm_feat_ms=kern, native_call_ms=call,
                                   iterations=dict(median=float(np.median(r["iterations"])), max=int(r["iterations"].max())),
                                   codes=np.bincount(r["codes"], minlength=7).tolist())
        if dt == "float16":
            hsrc = pat if form == "patch" else fs.texel_maps(s, dt)
            _, hcall, rh = timed(rf, form, hsrc, host_threads=16, reps=2, warm=0)
            res[f"{form}_{dt}"]["host_16_threads_ms"] = hcall
            res[f"{form}_{dt}"]["device_equals_host"] = bool(all(np.array_equal(rh[k], r[k], equal_nan=True) for k in fs.RESULT_KEYS))
        print(form, dt, json.dumps(res[f"{form}_{dt}"]), flush=True)
rf_geo = fs.refine_cfg(use_feature=False, max_num_iterations=100)
res["k_refine_lm_ms"], _, _ = timed(rf_geo, None, None)
rf_hm = fs.refine_cfg(use_feature=False, use_heatmap=True, max_num_iterations=100)
res["k_refine_lm_terms_heatmap_ms"], _, _ = timed(rf_hm, None, None, heatmaps=optimize.Heatmaps(fs.some_heatmaps(s), "float16"))
out = os.environ.get("OUT", os.path.join(ROOT, "profiles", "refine_feature_timing.json"))
with open(out, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
