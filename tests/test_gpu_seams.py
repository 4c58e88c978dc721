"""-m gpu: the seams between the stages of the matched step in the line-slot form.

k_node_prefix writes every candidate's scoring record for the candidates of its own nodes and the placement launch
lists the tiles by cost class beside the placement; LT_TEST_SEPARATE_CAND_META=1 selects the earlier sequence
(placement, then k_cand_meta) in the same path.  Both forms must give the same bits -- support scores, best
candidates, valid edges, the candidate count and the pair statistic (which depends on the tiles' windows, so it
catches a wrong window bound that the scores alone might not) -- at the shapes where the node-side fill and the
tile lists can go wrong.  The placement launch also carries the event in front of the scoring stage as its stop event:
pipelined runs, their result scalars and the pairing of the stage events."""
import os

import numpy as np
import pytest

from limap_amd import synthetic as syn

from helpers import compare_best, compare_candidates, compare_valid_edges

pytestmark = pytest.mark.gpu

SWITCH = "LT_TEST_SEPARATE_CAND_META"


@pytest.fixture
def clean_env():
    keys = (SWITCH, "LT_SCORE_TWO_KERNELS", "LT_SCORE_FUSED", "LT_FINE_TIMERS", "LT_TIMER_SAMPLE", "LT_EV_MARKERS",
            "LT_TEST_PLACE_COPY", "LT_TEST_SYNC_COUNT", "LT_GEN_ROW_SLOTS", "LT_TEST_NO_TILE_CLASSES")
    saved = {k: os.environ.pop(k, None) for k in keys}
    yield
    for k in keys:
        os.environ.pop(k, None)
        if saved[k] is not None:
            os.environ[k] = saved[k]


# ---- the cases: (scene, segments per image, matches per image, cfg) ----

def _case(sc, cfg=None, matches=None, segs=None):
    cfg = syn.default_triangulation_cfg(debug_mode=True, **(cfg or {}))
    if segs is None:
        segs = [sc.segs_of(i) for i in range(sc.n_images)]
    if matches is None:
        matches = {int(i): sc.matches_of(int(i)) for i in sc.img_ids}
    return sc, segs, matches, cfg


def case_general():
    """320 nodes (two workgroups of k_node_prefix, a tile across their border), C no multiple of 64, the last node has
    candidates."""
    return _case(syn.make_scene(n_views=8, n_segs=40, n_neighbors=5, seed=5))


def case_gap():
    """Image 5 and the last image get no match rows: 90 consecutive empty nodes between two non-empty ones, and a job
    whose last node is empty."""
    sc = syn.make_scene(n_views=12, n_segs=90, n_neighbors=5, seed=33)
    matches = {int(i): sc.matches_of(int(i)) for i in sc.img_ids}
    for i in (5, 11):
        matches[i] = {nb: np.zeros((0, 2), np.int32) for nb in matches[i]}
    return _case(sc, matches=matches)


def case_tiny():
    """Fewer than 64 candidates: a single partial tile."""
    return _case(syn.make_scene(n_views=4, n_segs=12, n_neighbors=3, seed=2))


def case_wide():
    """Few lines, as many match rows per line and neighbour as the neighbour has lines (30: the line-slot form takes
    runs of up to 32 rows), every other view a neighbour, permissive gates: nodes whose candidates cover three or more
    tiles."""
    sc = syn.make_scene(n_views=16, n_segs=30, n_neighbors=15, seed=2, topk=30)
    return _case(sc, cfg=dict(min_length_2d=0.0, IoU_threshold=0.0, line_tri_angle_threshold=0.0,
                              sensitivity_threshold=90.0))


def case_none():
    """Match rows, but no line passes the length gate: nodes without a single candidate."""
    return _case(syn.make_scene(n_views=4, n_segs=30, n_neighbors=2, seed=6), cfg=dict(min_length_2d=1e9))


def case_no_nodes():
    """No image has a segment: G == 0."""
    sc = syn.make_scene(n_views=3, n_segs=10, n_neighbors=2, seed=0)
    return _case(sc, segs=[np.zeros((0, 4)) for _ in range(3)], matches={int(i): {} for i in sc.img_ids})


def _longest_inner_gap(n):
    """longest run of empty nodes that has a non-empty node on either side"""
    nz = np.nonzero(n)[0]
    return int(np.max(np.diff(nz)) - 1) if len(nz) > 1 else 0


# what each case is there for, as a predicate on the candidates-per-node CSR `off` (asserted on the results)
CONDITIONS = {
    "general": lambda off: (off[-1] % 64 != 0 and len(off) - 1 > 256 and off[-1] > off[-2]
                            and any(off[g] % 64 != 0 and off[g - 1] < off[g] < off[-1]
                                    for g in range(256, len(off) - 1, 256))),   # a tile straddles two workgroups' nodes
    "gap": lambda off: _longest_inner_gap(np.diff(off)) > 64 and off[-1] == off[-2] and off[-1] > 0,
    "tiny": lambda off: 0 < off[-1] < 64,
    "wide": lambda off: bool(np.any(((off[1:] - 1) // 64 - off[:-1] // 64 + 1 >= 3) & (np.diff(off) > 0))),
    "none": lambda off: len(off) - 1 > 0 and off[-1] == 0,
    "no_nodes": lambda off: len(off) - 1 == 0,
}
CASES = {"general": case_general, "gap": case_gap, "tiny": case_tiny, "wide": case_wide, "none": case_none,
         "no_nodes": case_no_nodes}


def _run(case):
    from limap_amd import triangulation as tri
    sc, segs, matches, cfg = case
    T = tri.GlobalLineTriangulator(cfg)
    T.SetRanges(sc.ranges)
    T.InitArrays(sc.img_ids, sc.kvec, sc.qvec, sc.tvec, segs)
    for i in sc.img_ids:
        T.TriangulateImage(int(i), matches[int(i)])
    return T


def _results(T):
    ctx = T.context()
    return dict(all=ctx.get_all_tris(), best=ctx.get_best(), edges=ctx.get_valid_edges(), stats=ctx.stats(),
                timers=ctx.timers())


def _same(a, b):
    for k in ("off", "src", "line", "score"):
        assert np.array_equal(a["all"][k], b["all"][k]), f"all_tris[{k}] differs"
    for k in ("has_best", "src", "line", "score"):
        assert np.array_equal(a["best"][k], b["best"][k]), f"best[{k}] differs"
    assert np.array_equal(a["edges"][0], b["edges"][0]) and np.array_equal(a["edges"][1], b["edges"][1]), "valid edges differ"
    assert a["stats"]["candidates"] == b["stats"]["candidates"], (a["stats"], b["stats"])
    assert a["stats"]["pairs"] == b["stats"]["pairs"], (a["stats"], b["stats"])
    assert a["stats"]["valid_edges"] == b["stats"]["valid_edges"]


def _ab(case, **env):
    """the same job in the default form and with k_cand_meta behind the placement"""
    os.environ.update(env)
    try:
        new = _results(_run(case))
        os.environ[SWITCH] = "1"
        old = _results(_run(case))
    finally:
        for k in (SWITCH, *env):
            os.environ.pop(k, None)
    _same(new, old)
    return new


@pytest.mark.parametrize("name", list(CASES))
def test_node_side_records_and_lists_equal_cand_meta(gpu_lib, clean_env, name):
    case = CASES[name]()
    res = _ab(case)
    off = res["all"]["off"].astype(np.int64)
    assert CONDITIONS[name](off), "the scene no longer has the shape this case is there for"
    assert res["stats"]["candidates"] == off[-1]
    if name in ("none", "no_nodes"):
        assert res["stats"]["candidates"] == 0 and res["stats"]["pairs"] == 0 and res["stats"]["valid_edges"] == 0
        assert not res["best"]["has_best"].any()
    else:
        assert res["timers"]["line_slots"] == 1.0   # the path under test


def test_general_case_matches_oracle(gpu_lib, oracle, clean_env):
    sc, segs, matches, cfg = case_general()
    T = _run((sc, segs, matches, cfg))
    O = oracle.OracleTriangulator(cfg, faithful=False)
    O.SetRanges(sc.ranges)
    O.Init(sc.img_ids, sc.kvec, sc.qvec, sc.tvec, sc.seg_off, sc.segs)
    for i in sc.img_ids:
        O.TriangulateImage(int(i), matches[int(i)])
    compare_candidates(T.context().get_all_tris(), O.get_all_tris())
    compare_best(T.context().get_best(), O.get_best())
    compare_valid_edges(T.context().get_valid_edges(), O.get_valid_edges())


@pytest.mark.parametrize("form", ["LT_SCORE_TWO_KERNELS", "LT_SCORE_FUSED"])
def test_fallback_scoring_forms_read_the_same_lists(gpu_lib, clean_env, form):
    res = _ab(case_general(), **{form: "1"})
    assert res["stats"]["candidates"] > 0 and res["stats"]["pairs"] > 0
    base = _results(_run(case_general()))
    for k in ("off", "src", "line", "score"):
        assert np.array_equal(res["all"][k], base["all"][k])


def test_pipelined_runs_and_stage_event_pairing(gpu_lib, clean_env):
    case = case_general()
    sync_T = _run(case)
    ctx = sync_T.context()
    ctx.upload()
    ctx.timer_sums(reset=True)
    for _ in range(30):
        ctx.run_device()
    sync_sums, sync_n = ctx.timer_sums()
    sync_res = _results(sync_T)

    T = _run(case)
    ctx = T.context()
    ctx.upload()
    ctx.timer_sums(reset=True)
    for _ in range(30):
        ctx.run_device(wait=False)
    ctx.sync()
    sums, n = ctx.timer_sums()
    assert n == sync_n == 30
    assert ctx.timers()["run"] > 0 and sums["run"] > 0
    res = _results(T)
    _same(res, sync_res)
    assert res["stats"]["candidates"] > 0 and res["stats"]["pairs"] > 0

    # a sampled run (the first one on an idle context carries the stage events): every stage >= 0 and together they
    # are the run, within 10 % -- a bound against a wrong event pairing, not a performance figure
    for fine in (None, "1"):
        if fine:
            os.environ["LT_FINE_TIMERS"] = fine
        ctx.sync()
        ctx.run_device()
        t = ctx.timers()
        stages = [t[k] for k in ("gen", "compact", "score", "select")]
        print("stage timers (LT_FINE_TIMERS=%s): run %.4f ms, stages %s" % (fine, t["run"], stages))
        assert all(s >= 0.0 for s in stages), t
        assert abs(sum(stages) - t["run"]) <= 0.1 * t["run"], t
    os.environ.pop("LT_FINE_TIMERS", None)
