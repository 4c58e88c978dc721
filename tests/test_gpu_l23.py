"""2D-3D line matching for localization on the device (lt_kernels_l23.hip): the device equals the
host twin and the restatement bit for bit on every scene, mode and filter of tests/l23_scenes.py -- rows, order,
offsets, winning losses --, is deterministic, grows its buffers, and batches queries; the runner gives the same poses
on the device as on the host.  Every input is valid: refusals happen on the host before any launch
(tests/test_l23_host.py)."""
import numpy as np
import pytest

import l23_scenes as S
from limap_amd import _capi
from limap_amd import localization as loc

pytestmark = pytest.mark.gpu

CASES = S.cases()


def same(a, b):
    return (np.array_equal(a["q_off"], b["q_off"]) and np.array_equal(a["rows"], b["rows"])
            and np.array_equal(a["loss"].view(np.int64), b["loss"].view(np.int64)))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_equals_twin_and_restatement(gpu_lib, oracle, case):
    dev = S.product(loc, case)
    twin = S.product(loc, case, host=True)
    q_off, rows, loss = S.reference(oracle, case)
    print(f"{case['name']}: {len(rows)} rows, timers {dev['timers']}")
    assert same(dev, twin)
    assert np.array_equal(dev["q_off"], q_off) and np.array_equal(dev["rows"], rows)
    assert np.array_equal(dev["loss"].view(np.int64), loss.view(np.int64))


def test_two_runs_give_identical_bytes(gpu_lib):
    for name in ("sizes-all_pairs-None", "sizes-all_pairs-Midpoint_Perpendicular", "filter-listed-Midpoint-dist_thres10.0"):
        case = next(c for c in CASES if c["name"] == name)
        a, b = S.product(loc, case), S.product(loc, case)
        assert a["rows"].tobytes() == b["rows"].tobytes() and a["loss"].tobytes() == b["loss"].tobytes()
        assert a["q_off"].tobytes() == b["q_off"].tobytes() and len(a["rows"]) > 0


def test_a_larger_call_after_a_small_one(gpu_lib):
    """a fresh context sizes its buffers for the small call; the larger one must grow every one of them"""
    ctx = _capi.Context()
    try:
        for name in ("order-all_pairs-Perpendicular", "sizes-all_pairs-Perpendicular", "order-listed-None",
                     "filter-listed-Perpendicular-dist_thres10.0", "sizes-all_pairs-None"):
            case = next(c for c in CASES if c["name"] == name)
            assert same(S.product(loc, case, ctx=ctx), S.product(loc, case, host=True)), name
    finally:
        ctx.close()


@pytest.mark.parametrize("filt", [None, "Midpoint_Perpendicular"])
def test_a_batch_equals_single_query_calls(gpu_lib, filt):
    sc = S.sizes_scene()
    batch = loc.match_lines_arrays(loc.scene_arrays(*S.args(sc)), "all_pairs", dist_func=filt)
    for q in (0, 2, 4):
        one = dict(sc, q_cams=[sc["q_cams"][q]], q_segs=[sc["q_segs"][q]], tasks=[sc["tasks"][q]])
        res = loc.match_lines_arrays(loc.scene_arrays(*S.args(one)), "all_pairs", dist_func=filt)
        lo, hi = batch["q_off"][q], batch["q_off"][q + 1]
        assert np.array_equal(res["rows"], batch["rows"][lo:hi]) and hi > lo
        assert np.array_equal(res["loss"].view(np.int64), batch["loss"][lo:hi].view(np.int64))


def test_runner_on_the_device_equals_the_host(gpu_lib, tmp_path):
    sc = S.loc_scene()
    db, qr, db_segs, q_segs, linemap, retrieval, corresp = S.collections(sc)
    poses = {}
    for host in (False, True):
        poses[host] = loc.hybrid_localization(S.cfg(), db, qr, corresp, linemap, retrieval, tmp_path / f"results_{host}.txt",
                                              all_db_segs=db_segs, all_query_segs=q_segs, host=host, seed=3)
    for qid in (100, 101):
        assert np.array_equal(poses[False][qid].qvec, poses[True][qid].qvec)
        assert np.array_equal(poses[False][qid].tvec, poses[True][qid].tvec)
    assert (tmp_path / "results_False.txt").read_text() == (tmp_path / "results_True.txt").read_text()
