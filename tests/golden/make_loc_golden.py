"""Writes tests/golden/loc/*.npz: the CSR inputs of small pose-refinement batches (tests/loc_scenes.py) with the results
of the host path (lt_fn_loc_host) recorded -- poses, both costs, residual counts, iterations, codes -- so that a change
of the minimiser (DESIGN.md sections 19 and 25) shows up as a diff of these files even where the device and its host
twin move together.  tests/test_loc_host.py replays them on the host, tests/test_gpu_loc.py on the device.

    python tests/golden/make_loc_golden.py

Termination codes reached: 1 (radius) by most problems, 2 (zero gradient) by `edge_huber` and one problem of `blocks`,
0 (iteration cap) by `capped`, by the perpendicular fixture of `edge_2d` and by two problems of `blocks`, 7 (no
residuals) by the empty problem of `blocks`.  Codes 3, 4 and 6 are not reached: no scene of loc_scenes.py produces them.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import loc_scenes as ls  # noqa: E402
from limap_amd import hybrid_localization as hl  # noqa: E402
from test_loc_host import CSR_KEYS, OUT_KEYS, ocfg, struct_of  # noqa: E402


def sized(n_blocks, seed, share=0.4):
    nl = int(round(n_blocks * share))
    return ls.make_problem(nl, n_blocks - nl, seed=seed, multi=0.0)


def cases():
    edge = {n: (o, p) for n, o, p in ls.edge_problems()}
    empty = dict(ls.make_problem(1, 1, seed=1), l3ds=np.zeros((0, 2, 3)), l2ds=[], p3ds=[], p2ds=[])
    some = [ls.make_problem(3 + n % 5, 4 + n % 7, seed=500 + n) for n in range(5)]
    return {
        # the edge fixtures: the clamps of the sine and the cosine, the parallel ray of the 3D distance, both sides of Huber
        "edge_2d": ([edge["parallel"][1], edge["perpendicular"][1]], ocfg(2, 1, 0), 100),
        "edge_ray": ([edge["ray_parallel_to_line"][1]], ocfg(**edge["ray_parallel_to_line"][0]), 100),
        "edge_huber": ([edge["huber_sides"][1]], ocfg(**edge["huber_sides"][0]), 100),
        # block counts around the 64-lane width (two residuals per block), one block of either kind, an empty problem
        "blocks": ([sized(1, 601, 0.0), sized(1, 601, 1.0), empty] + [sized(n, 600 + n) for n in (2, 63, 64, 65, 129)],
                   ocfg(2, 0, 1, loss_a=2.0), 100),
        # three and four residuals per line block
        "angle3": (some, ocfg(1, 1, 3, loss_a=2.0, weight_line=0.6), 100),
        "perp4": (some, ocfg(3, 3, 2, loss_a=1.0), 100),
        "capped": (some[:3], ocfg(2, 0, 0), 1),
    }


def main():
    os.makedirs(os.path.join(HERE, "loc"), exist_ok=True)
    for name, (probs, cfg, max_iter) in cases().items():
        csr = hl._problem_arrays(probs)
        s = struct_of(cfg)
        s.max_num_iterations = max_iter
        r = hl.loc_arrays(csr, s, 4)
        data = {"in_" + k: np.asarray(v) for k, v in zip(CSR_KEYS, csr)}
        data.update({"cfg_" + k: np.array(v) for k, v in cfg.items()})
        data["max_num_iterations"] = np.array(max_iter)
        data.update({"out_" + k: r[k] for k in OUT_KEYS})
        np.savez_compressed(os.path.join(HERE, "loc", f"loc_{name}.npz"), **data)
        print(name, len(probs), "problems, codes", np.bincount(r["codes"], minlength=8), "iterations", r["iterations"])


if __name__ == "__main__":
    main()
