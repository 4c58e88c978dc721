"""ora_linker3d_check_pairs (oracle.linker3d_check_pairs), the batched form of the predicate inside the oracle's
RemergeLineTracks, against that function itself: on a small scene the grouping rebuilt from the predicate alone equals
one pass of ora_ts_remerge_once, which tests/test_oracle_vs_ref.py::test_post_triangulation_chain pins to oracle/_ref.
CPU only."""
import numpy as np

from limap_amd import synthetic as syn

from helpers import run_oracle

LINKER = dict(score_th=0.5, th_angle=5.0, th_overlap=0.001, th_smartoverlap=0.1, th_smartangle=1.0, th_perp=1.0,
              th_innerseg=1.0)


def test_predicate_rebuilds_the_remerge_pass(oracle):
    sc = syn.make_scene(n_views=20, n_segs=150, n_neighbors=8, seed=0)
    O = run_oracle(oracle, sc, syn.default_triangulation_cfg())
    O.ComputeLineTracks()
    ts = oracle.OracleTrackSet(O)
    ts.filter_by_reprojection(8.0, 5.0)
    before = ts.get()
    line, T = before["line"], len(before["line"])
    assert T > 50 and before["active"].all()
    i, j = np.nonzero(~np.eye(T, dtype=bool))
    hit = oracle.linker3d_check_pairs(LINKER, line[i], line[j]).reshape(T, T - 1)
    assert hit.any()
    # every track active: the pair {a < b} is tested as (a, b) when a + b is odd, as (b, a) when it is even
    # (merging/merging.cc:535-540); then union by size in the order of the sorted edges, labels by root index (:557-600)
    full = np.zeros((T, T), bool)
    full[i, j] = hit.reshape(-1)
    parent, size = [-1] * T, [1] * T

    def root(x):
        while parent[x] != -1:
            x = parent[x]
        return x
    for a in range(T):
        for b in range(a + 1, T):
            if full[a, b] if (a + b) % 2 else full[b, a]:
                r1, r2 = root(a), root(b)
                if r1 == r2:
                    continue
                if size[r1] < size[r2]:
                    r1, r2 = r2, r1
                parent[r2] = r1; size[r1] += size[r2]; size[r2] = 0
    roots = [t for t in range(T) if parent[t] == -1]
    want = [[t for t in range(T) if root(t) == r] for r in roots]
    ts.remerge_once(LINKER)
    after = ts.get()
    assert len(want) == len(after["off"]) - 1 < T
    sizes = np.diff(before["off"])
    for g, members in enumerate(want):
        a, b = int(after["off"][g]), int(after["off"][g + 1])
        ids = np.concatenate([before["line_ids"][before["off"][t]:before["off"][t + 1]] for t in members])
        img = np.concatenate([before["image_ids"][before["off"][t]:before["off"][t + 1]] for t in members])
        assert b - a == sizes[members].sum()
        assert np.array_equal(after["line_ids"][a:b], ids) and np.array_equal(after["image_ids"][a:b], img)
    assert after["active"].tolist() == [len(m) > 1 for m in want]


def test_batch_of_a_600_track_case_is_one_call(oracle):
    """360 000 pairs in one call; each agrees with the same pair asked alone"""
    rng = np.random.default_rng(0)
    s = rng.uniform(-1, 1, (600, 3))
    line = np.concatenate([s, s + rng.normal(0, 0.3, (600, 3)), np.ones((600, 1))], 1)
    i, j = np.meshgrid(np.arange(600), np.arange(600), indexing="ij")
    lk = dict(LINKER, th_angle=30.0, th_innerseg=0.5)
    out = oracle.linker3d_check_pairs(lk, line[i.ravel()], line[j.ravel()])
    assert out.shape == (360000,) and 0 < out.sum() < out.size
    for k in rng.integers(0, out.size, 50).tolist() + np.nonzero(out)[0][:50].tolist():
        assert oracle.linker3d_check_pairs(lk, line[i.ravel()[k]], line[j.ravel()[k]])[0] == out[k]
