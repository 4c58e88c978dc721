"""Writes tests/golden/refine_feature/*.npz: the inputs of small refinement scenes with the feature-consistency term
(tests/refine_feature_scenes.py) and the results of the host path (lt_fn_refine_host_feature) recorded -- parameters,
segments, both costs, iterations, codes -- so that a change of the minimiser or of the jet (DESIGN.md sections 19 and 26)
shows up as a diff of these files even where the device and its host twin move together.
tests/test_refine_feature_host.py replays them on the host, tests/test_gpu_refine_feature.py on the device.

    python tests/golden/make_refine_feature_golden.py

A feature map is 48 x 64 x 128 texels, 768 KiB in binary16, and a scene has seven: they are not stored.  A file holds
the recipe of the maps (the arguments of refine_feature_scenes.make_scene, whose maps are a closed form of the cameras)
and the SHA-256 of every map's texels, which the replay checks before it solves; everything else the solve reads is
stored.

`mixed_*`: four tracks of one call -- two with feature blocks, one whose supports lie 0.3 + 1e-9 px beside the projection
(no kept sample: no feature block), one whose first half is covered by a single support (fewer kept samples) -- in
binary16, in float32, and in binary16 with the VP and the heatmap term.  `failing`: the reference intersection fails at
the initial line.
Termination codes reached: 0 (iteration cap) and 1 (radius) by the tracks of mixed_*, 6 by failing.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import refine_feature_scenes as fs  # noqa: E402
from test_refine_feature_host import GOLDEN_IN, golden_maps, run_golden  # noqa: E402

SCENE_KW = dict(counts=(5, 4, 6, 4, 5), seed=2)  # the scene of tests/test_gpu_refine_feature.py


def mixed():
    scene = fs.make_scene(**SCENE_KW)
    exact = fs.projected_supports(scene, 0)
    K = len(exact["img"])
    return fs.merge(fs.subset(scene, [1]), fs.shifted(exact, 0.3 + 1e-9), fs.subset(scene, [2]),
                    fs.trimmed(exact, [(0.0, 0.5)] + [(0.6, 1.0)] * (K - 1)))


def main():
    os.makedirs(os.path.join(HERE, "refine_feature"), exist_ok=True)
    m = mixed()
    vp_flag, vp3 = fs.some_vps(m)
    cases = {
        "mixed_f16": (m, dict(SCENE_KW), dict(dtype="float16"), None),
        "mixed_f32": (m, dict(SCENE_KW), dict(dtype="float32"), None),
        "mixed_vp_hm_f16": (m, dict(SCENE_KW), dict(dtype="float16", use_vp=True, use_heatmap=True, vp_multiplier=0.1,
                                                     n_samples_heatmap=5), (vp_flag, vp3)),
        "failing": (fs.failing_scene(), None, dict(dtype="float16"), None),
    }
    for name, (s, scene_kw, cfg_kw, vp) in cases.items():
        data = {k: s[k] for k in GOLDEN_IN}
        if scene_kw is not None:
            data.update(maps_counts=np.array(scene_kw["counts"]), maps_seed=np.array(scene_kw["seed"]))
        data.update({"cfg_" + k: np.array(v) for k, v in cfg_kw.items()})
        if vp is not None:
            data.update(vp_flag=vp[0], vp3=vp[1])
        maps = golden_maps(data, cfg_kw["dtype"])
        data["maps_sha256"] = np.array([fs.texel_digest(maps[int(i)]) for i in s["img_ids"]])
        r = run_golden(data, maps, host_threads=4)
        data.update({"out_" + k: r[k] for k in fs.RESULT_KEYS})
        np.savez_compressed(os.path.join(HERE, "refine_feature", f"refine_feature_{name}.npz"), **data)
        print(name, len(s["line6"]), "tracks, codes", r["codes"], "iterations", r["iterations"])


if __name__ == "__main__":
    main()
