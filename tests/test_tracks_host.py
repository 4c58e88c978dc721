"""The cases of tests/connect_cases.py without a GPU: every builder with the assertions it makes on the oracle, and the
restated pair loop (merging/merging.cc:519-556) plus union / label rule (:557-600) of that module against one pass of the
oracle's RemergeLineTracks on whole scenes -- in both regimes, every track active (parity rule) and not.  This ties what
tests/test_gpu_track_connect.py expects of k_track_connect to the oracle, which tests/test_oracle_vs_ref.py ties to the
reference's own sources."""
import numpy as np
import pytest

from limap_amd import synthetic as syn

import connect_cases as cc
from helpers import run_oracle

REMERGE_LINKER = dict(score_th=0.5, th_angle=5.0, th_overlap=0.001, th_smartoverlap=0.1, th_smartangle=1.0,
                      th_perp=1.0, th_innerseg=1.0)


@pytest.mark.parametrize("k", range(len(cc.BUILDERS)))
def test_builder(oracle, k):
    name, line7, active, linker, capacity0, facts = cc.BUILDERS[k]()
    e = cc.expected((name, line7, active, linker))
    assert facts["n_unique"] == len(e["edges"]) and facts["n_raw"] >= facts["n_unique"]
    assert len(line7) <= 600 and np.array_equal(e["edges"], cc.expected_edges(line7, active, linker))


def test_case_names_are_unique(oracle):
    assert len(cc.all_cases()) == len(cc.BUILDERS) == 47


def test_union_rule_on_hand_made_edges():
    """union by size, the larger root stays; on a tie the first; labels count the roots in index order"""
    lab = cc.groups_from_edges(6, [(0, 5), (1, 2), (2, 5), (3, 4)])
    # (0,5): 0 root; (1,2): 1 root; (2,5): roots 1 and 0, equal sizes -> 0 joins 1; (3,4): 3 root
    assert lab.tolist() == [0, 0, 0, 1, 1, 0]
    assert cc.groups_as_lists(lab) == [[0, 1, 2, 5], [3, 4]]
    assert cc.groups_from_edges(3, np.zeros((0, 2), np.int64)).tolist() == [0, 1, 2]


def groups_of_pass(before, after):
    """the input tracks of every output track of a remerge pass, through the (image, line) ids of the members"""
    owner = {}
    for t in range(len(before["off"]) - 1):
        for m in range(int(before["off"][t]), int(before["off"][t + 1])):
            owner[(int(before["image_ids"][m]), int(before["line_ids"][m]))] = t
    assert len(owner) == len(before["image_ids"])
    out = []
    for g in range(len(after["off"]) - 1):
        ms = range(int(after["off"][g]), int(after["off"][g + 1]))
        seq = [owner[(int(after["image_ids"][m]), int(after["line_ids"][m]))] for m in ms]
        out.append(sorted(set(seq), key=seq.index))
    return out


@pytest.mark.parametrize("seed,views,segs,nn,merges", [(3, 16, 110, 7, [True, True]), (0, 20, 150, 8, [True, False])])
def test_restated_loop_reproduces_the_oracles_remerge_pass(oracle, seed, views, segs, nn, merges):
    sc = syn.make_scene(n_views=views, n_segs=segs, n_neighbors=nn, seed=seed)
    O = run_oracle(oracle, sc, syn.default_triangulation_cfg())
    O.ComputeLineTracks()
    ts = oracle.OracleTrackSet(O)
    ts.filter_by_reprojection(8.0, 5.0)
    regimes = []
    # the first pass sees only active tracks and leaves the groups of one inactive; the second, with wider gates so that
    # it still finds pairs, sees both kinds
    for linker in (REMERGE_LINKER, dict(REMERGE_LINKER, th_angle=12.0, th_innerseg=4.0, th_smartangle=4.0)):
        before = ts.get()
        T = len(before["line"])
        active = before["active"].astype(bool)
        regimes.append(bool(active.all()))
        edges = cc.expected_edges(before["line"], active, linker)
        labels = cc.groups_from_edges(T, edges)
        ts.remerge_once(linker)
        after = ts.get()
        want = cc.groups_as_lists(labels)
        assert groups_of_pass(before, after) == want
        assert (len(want) < T) == merges[len(regimes) - 1]         # (what each pass is here for: it merges something)
        assert after["active"].tolist() == [len(g) > 1 for g in want]
    assert regimes == [True, False]
