"""Writes tests/golden/refine/*.npz: inputs of small refinement scenes (tests/refine_scenes.py) with the results of the
host path (lt_fn_refine_host) recorded, so that a change of the definition shows up as a diff of
these files.  tests/test_refine_host.py replays them on the host, tests/test_gpu_refine.py on the device.

    python tests/golden/make_refine_golden.py
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import refine_scenes as rs  # noqa: E402
from limap_amd import _capi  # noqa: E402
from test_refine_host import cfg_of, run_host  # noqa: E402

CASES = {
    "small": (dict(n_tracks=40, seed=21), dict(max_num_iterations=200)),
    "wide": (dict(n_tracks=12, seed=22, k_max=70, n_views=40), dict(max_num_iterations=200, num_outliers_aggregator=1)),
    "constant": (dict(n_tracks=12, seed=23), dict(constant_line=1)),
    "mixed_min_images": (dict(n_tracks=30, seed=24), dict(min_num_images=7, max_num_iterations=100)),
    "capped": (dict(n_tracks=12, seed=25), dict(max_num_iterations=3, geometric_alpha=5.0)),
}


def main():
    L = _capi.load_library()
    os.makedirs(os.path.join(HERE, "refine"), exist_ok=True)
    cases = dict(CASES, edge=(None, dict(min_num_images=1, max_num_iterations=200, num_outliers_aggregator=0)),
                 edge_constant=(None, dict(min_num_images=4, num_outliers_aggregator=1)))
    for name, (scene_kw, cfg_kw) in cases.items():
        s = rs.edge_scene() if scene_kw is None else rs.make_tracks(**scene_kw)
        rc, r = run_host(L, s, cfg_of(L, **cfg_kw))
        assert rc == 0, name
        data = {k: s[k] for k in ("img_ids", "k", "q", "t", "line6", "off", "img", "l2d", "l3d")}
        data.update({"cfg_" + k: np.array(v) for k, v in cfg_kw.items()})
        data.update({"out_" + k: v for k, v in r.items()})
        np.savez_compressed(os.path.join(HERE, "refine", f"refine_{name}.npz"), **data)
        print(name, len(s["line6"]), "tracks", np.bincount(r["codes"], minlength=6))


if __name__ == "__main__":
    main()
