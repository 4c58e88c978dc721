"""Writes tests/golden/ba/*.npz: the inputs of small bundle-adjustment scenes (tests/ba_scenes.py) with the full output
of the host path (lt_fn_ba_host) recorded -- poses, points, line parameters, segments, both costs, iterations, code --
so that a change of the minimiser, of the damped step or of a reduction order (DESIGN.md sections 19 and 27) shows up as a
diff of these files even where the device and its host twin move together.  tests/test_ba_host.py replays them on the
host, tests/test_gpu_ba.py on the device.

    python tests/golden/make_ba_golden.py

Free poses: `hybrid` (4 images, points and lines), `two_cameras` (one point), `lines_only`, `radius` (a scene without
noise that starts at its minimum: steps are rejected until the radius ends the solve), `depth_zero` (a point in a
camera's plane).  Constant poses: `cp_points` (point tracks of 33, 1, 15, 16 and 17 blocks: the 16-lane group and its
loop), `cp_failing` (the failing track of depth_zero among moving ones).
Termination codes reached: 0 (hybrid, lines_only), 1 (radius), 2 (two_cameras, cp_points), 6 (depth_zero, cp_failing).
Codes 3 and 4 end no solve here: with free poses they are rejected steps, and no point track of ba_scenes.py meets them.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import ba_scenes as bs  # noqa: E402
from test_ba_host import GOLDEN_IN as IN_KEYS  # noqa: E402


def depth_zero():
    s = bs.make_scene(n_cams=3, n_points=5, n_lines=0, seed=5)
    s["q"][0] = [1.0, 0.0, 0.0, 0.0]
    s["t"][0] = [0.0, 0.0, 5.0]
    s["p3"][2] = [0.3, 0.2, -5.0]
    return s


def cases():
    return {
        "hybrid": (bs.make_scene(n_cams=4, n_points=24, n_lines=6, seed=0), dict(max_num_iterations=30)),
        "two_cameras": (bs.make_scene(n_cams=2, n_points=1, n_lines=0, seed=11), dict(max_num_iterations=20)),
        "lines_only": (bs.make_scene(n_cams=5, n_points=0, n_lines=7, seed=13), dict(max_num_iterations=25)),
        "radius": (bs.make_scene(n_cams=3, n_points=6, n_lines=0, seed=16, noise_px=0.0, pose_sigma=0.0, struct_sigma=0.0),
                   dict(max_num_iterations=30)),
        "depth_zero": (depth_zero(), dict()),
        "cp_points": (bs.make_scene(n_cams=6, n_points=5, n_lines=0, seed=55, point_obs=[33, 1, 15, 16, 17]),
                      dict(constant_pose=1, max_num_iterations=30)),
        "cp_failing": (depth_zero(), dict(constant_pose=1, max_num_iterations=20)),
    }


def main():
    os.makedirs(os.path.join(HERE, "ba"), exist_ok=True)
    for name, (s, cfg_kw) in cases().items():
        rc, o = bs.run_host(s, bs.cfg_of(**cfg_kw), 4)
        assert rc == 0, name
        data = {k: s[k] for k in IN_KEYS}
        data.update({"cfg_" + k: np.array(v) for k, v in cfg_kw.items()})
        data.update({"out_" + k: v for k, v in o.items()})
        np.savez_compressed(os.path.join(HERE, "ba", f"ba_{name}.npz"), **data)
        print(name, "cost", o["cost"], "iterations", o["iterations"][0], "code", o["code"][0])


if __name__ == "__main__":
    main()
