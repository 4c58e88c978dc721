"""Writes tests/golden/assoc/*.npz: the inputs of small association scenes (tests/assoc_scenes.py) with the full output
of the host path (lt_fn_assoc_host) recorded -- points, line parameters, vanishing points, both costs, iterations, CG
iterations, code -- so that a change of the minimiser, of the linear solve or of a reduction order
shows up as a diff of these files even where the device and its host twin move together.  tests/test_assoc_host.py
replays them on the host, tests/test_gpu_assoc.py on the device.

    python tests/golden/make_assoc_golden.py

`small` (the evaluation scene with both clamp cases), `structured` (three direction classes, a junction), `vp_only`
(no point-line edges), `pl_only` (no vanishing-point residuals), `tight_cg` (eta 1e-6: several CG iterations per attempt),
`zero_gradient` (orthogonality edges between the coordinate axes alone: code 2), `depth_zero` (a point of depth 0 in a
camera: code 6), `breakdown` and `pivot` (every attempt's linear solve fails, at p.Ap and at a pivot: fifteen rejected
steps, code 1).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import assoc_scenes as sc  # noqa: E402
from test_assoc_host import GOLDEN_IN as IN_KEYS  # noqa: E402


def cases():
    st = sc.structured_scene(n_cams=4, seed=7)
    return {
        "small": (sc.small_scene(0, orth_exact=True, identical=True), dict(max_num_iterations=30, lw_vp_collinearity=0.5)),
        "structured": (sc.structured_scene(n_cams=5, seed=3), dict(max_num_iterations=30)),
        "vp_only": (st, dict(max_num_iterations=20, enable_pointline=0)),
        "pl_only": (st, dict(max_num_iterations=20, enable_vpline=0)),
        "tight_cg": (st, dict(max_num_iterations=20, cg_eta=1e-6)),
        "zero_gradient": (sc.stationary_vp_scene(), dict(sc.STATIONARY)),
        "depth_zero": (sc.depth_zero_scene(), dict(max_num_iterations=5)),
        "breakdown": (sc.structured_scene(n_cams=4, seed=5), dict(sc.BREAKDOWN, max_num_iterations=20)),
        "pivot": (sc.pivot_scene(), dict(sc.PIVOT, max_num_iterations=20)),
    }


def main():
    os.makedirs(os.path.join(HERE, "assoc"), exist_ok=True)
    for name, (s, cfg_kw) in cases().items():
        rc, o = sc.run_host(s, sc.cfg_of(**cfg_kw), 4)
        assert rc == 0, name
        data = {k: s[k] for k in IN_KEYS}
        data.update({"cfg_" + k: np.array(v) for k, v in cfg_kw.items()})
        data.update({"out_" + k: v for k, v in o.items()})
        np.savez_compressed(os.path.join(HERE, "assoc", f"assoc_{name}.npz"), **data)
        print(name, "cost", o["cost"], "iterations", o["iterations"][0], "cg", o["cg_iterations"][0], "code", o["code"][0])


if __name__ == "__main__":
    main()
