"""Depth scenes of the line-fitter tests: small synthetic rooms (limap_amd.synthetic.render_depths) plus hand-made
segments at the edges of the contract, and the comparison of a device result with tests/fit_oracle.py."""
import numpy as np

import fit_oracle as fo


def cams_of(sc):
    return {int(i): (sc.kvec[n], sc.qvec[n], sc.tvec[n]) for n, i in enumerate(sc.img_ids)}


def edge_segments(h, w):
    """segments partly / fully outside, negative coordinates, zero length, horizontal, vertical, |dx| == |dy|, long"""
    L = max(h, w)
    return np.array([
        [-20.3, 10.7, 40.2, 30.9],          # starts left of the image
        [w - 30.5, h - 5.2, w + 40.0, h + 9.0],  # leaves at the bottom right
        [-50.0, -40.0, -10.0, -3.0],        # fully outside (negative)
        [w + 5.0, 3.0, w + 60.0, 40.0],     # fully outside (right)
        [12.9, 17.2, 12.1, 17.8],           # truncates to one pixel
        [5.0, 20.0, w - 6.0, 20.0],         # horizontal
        [30.0, 2.0, 30.0, h - 3.0],         # vertical
        [3.0, 4.0, 3.0 + 40.0, 4.0 + 40.0],  # |dx| == |dy|
        [w - 2.0, 1.0, w - 2.0 - 45.0, 46.0],  # |dx| == |dy| leftwards
        [-0.7, -0.2, w + L * 0.5, h + L * 0.4],  # long diagonal, longer than the LDS path
        [w - 1.0, h - 1.0, 0.0, 0.0],       # the full diagonal backwards
    ])


def compare(dev_seg, dev_status, dev_stats, ref, where):
    """device (seg (2, 3), status, stats (5,)) against one fit_oracle.fit_segment result, bit for bit"""
    assert int(dev_status) == ref["status"], f"{where}: status {dev_status}, oracle {ref['status']}"
    assert int(dev_stats[0]) == ref["kept"], f"{where}: kept {dev_stats[0]}, oracle {ref['kept']}"
    assert int(dev_stats[1]) == ref["inliers"], f"{where}: inliers {dev_stats[1]}, oracle {ref['inliers']}"
    assert int(dev_stats[2]) == ref["num_iterations"], f"{where}: iterations {dev_stats[2]}, oracle {ref['num_iterations']}"
    assert int(dev_stats[3]) == ref["number_lo_iterations"], f"{where}: LO {dev_stats[3]}, oracle {ref['number_lo_iterations']}"
    assert bool(dev_stats[4]) == ref["from_lo"], f"{where}: from_lo"
    a = np.ascontiguousarray(dev_seg, np.float64).reshape(6).view(np.uint64)
    b = np.ascontiguousarray(ref["seg"], np.float64).reshape(6).view(np.uint64)
    assert np.array_equal(a, b), f"{where}: endpoints {np.asarray(dev_seg).reshape(6)} oracle {ref['seg'].reshape(6)}"


def oracle_scene(all_2d, sc, depths, opt=None, ransac_th=0.75, min_pct=0.6, var2d=5.0, seed=0):
    opt = opt or fo.Options()
    opt.random_seed_ = seed
    return fo.fit_scene(all_2d, cams_of(sc), depths, opt, ransac_th, min_pct, var2d)
