"""Writes tests/golden/refine_terms/*.npz: small scenes with the VP and the heatmap term (tests/refine_terms_scenes.py),
their texels, the configuration and the results of the host path (lt_fn_refine_host_terms), which the host test and the
device test reproduce bit for bit.  Run from the repository root: python tests/golden/make_refine_terms_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import refine_terms_scenes as ts  # noqa: E402
from limap_amd import _capi  # noqa: E402

OUT = os.path.join(HERE, "refine_terms")
SCENE_KEYS = ("img_ids", "k", "q", "t", "hw", "line6", "off", "img", "l2d", "l3d", "vp_flag", "vp3")


def cases():
    base = ts.make_scene([1, 4, 5, 15, 16, 17, 33], seed=1)
    yield ("all_terms_f16", ts.merge(base, ts.failing_track()), np.float16, dict(num_outliers_aggregator=0),
           dict(use_vp=1, use_heatmap=1))
    yield ("heatmap_only_f32", ts.make_scene([4, 16, 17], seed=2), np.float32, dict(num_outliers_aggregator=1),
           dict(use_geometric=0, use_heatmap=1, n_samples_heatmap=11, texel_type=_capi.TEXEL_F32))
    yield ("vp_only", ts.make_scene([5, 33], seed=3), np.float16, dict(max_num_iterations=60),
           dict(use_vp=1, vp_multiplier=0.1))
    yield ("clamped_two_samples_f16", ts.long_supports(ts.make_scene([4, 6, 17], seed=4)), np.float16, dict(),
           dict(use_heatmap=1, n_samples_heatmap=2, heatmap_multiplier=2.0, sample_range_min=0.0, sample_range_max=1.0))


def main():
    L = _capi.load_library()
    os.makedirs(OUT, exist_ok=True)
    for name, s, dtype, cfg, terms in cases():
        tex = ts.texels(s, dtype)
        rc, r = ts.run_host(L, s, ts.cfg_struct(L, **cfg), ts.terms_struct(L, **terms), tex, threads=1)
        assert rc == 0, (name, L.lt_fn_refine_host_error())
        data = {k: s[k] for k in SCENE_KEYS}
        data.update(hm_ids=tex[0], hm_h=tex[1], hm_w=tex[2], **{f"hm_{int(i)}": a for i, a in zip(tex[0], tex[3])})
        data.update({"cfg_" + k: np.array(v) for k, v in cfg.items()}, **{"terms_" + k: np.array(v) for k, v in terms.items()})
        data.update({"out_" + k: v for k, v in r.items()})
        np.savez_compressed(os.path.join(OUT, name + ".npz"), **data)
        print(name, "codes", np.bincount(r["codes"], minlength=7), "iterations", r["iterations"])


if __name__ == "__main__":
    main()
