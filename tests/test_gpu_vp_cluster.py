"""-m gpu: k_vp_cluster alone, through lt_vp_cluster_sets, on preference sets the tests choose (tests/vp_cluster_cases.py).
The reference is tests/vp_oracle.py: cluster, the brute-force restatement over a full ratio matrix; equality with the host
twin (lt_fn_vp_cluster_host) is asserted next to it, never instead of it.  Zero tolerance: np.array_equal on the roots.
Every image of more than 2048 rows keeps its state in global memory (`n <= kVpLdsClusters ? s_state : g_state + ...` in
lt_kernels_vp.hip); the tests assert that size on their inputs."""
import ctypes as C

import numpy as np
import pytest

import vp_cluster_cases as vcc
import vp_oracle as vo
from test_vp_host import KAT, _sets, host_cluster

pytestmark = pytest.mark.gpu

CASES = vcc.all_cases()
BY_NAME = dict(CASES)
_oracle_memo = {}


def oracle_roots(name):
    if name not in _oracle_memo:
        _oracle_memo[name] = vo.cluster(BY_NAME[name])
    return _oracle_memo[name]


def words_of(pref, w=None):
    """the packed rows, padded with zero words to w words (zero bits belong to no set: the clustering is the same)"""
    words = vcc.pack(pref)
    if w is not None and w > words.shape[1]:
        words = np.concatenate([words, np.zeros((words.shape[0], w - words.shape[1]), np.uint64)], 1)
    return words


def device_cluster(prefs):
    """one lt_vp_cluster_sets call for the list of bool matrices -> list of roots"""
    from limap_amd import vplib
    w = max(vcc.pack(p[:0]).shape[1] for p in prefs)
    return vplib._cluster_sets([words_of(p, w) for p in prefs])


def test_the_large_cases_leave_the_lds(gpu_lib):
    big = [name for name, p in CASES if p.shape[0] > vcc.LDS_CLUSTERS]
    assert len(big) == 8 and {BY_NAME[n].shape[0] for n in big} == {2049, 2600}
    assert any(p.shape[0] == vcc.LDS_CLUSTERS for _, p in CASES) and any(p.shape[0] == 2047 for _, p in CASES)


@pytest.mark.parametrize("sets,want", KAT)
def test_known_answers_on_the_device(gpu_lib, sets, want):
    pref = _sets(sets)
    assert vo.cluster(pref).tolist() == want
    got, = device_cluster([pref])
    assert got.tolist() == want


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_case_families_device_equals_oracle(gpu_lib, name):
    pref = BY_NAME[name]
    got, = device_cluster([pref])
    assert got.shape == (pref.shape[0],)
    assert np.array_equal(got, oracle_roots(name))
    assert np.array_equal(got, host_cluster(gpu_lib, pref))


def batch_order():
    """all cases, the images above 2048 rows spread among the small ones: 2049, small, 2600, small, ... and one pair of
    large images side by side -- either way their slices of the global state are neighbours or one small image apart"""
    big = sorted((n for n, p in CASES if p.shape[0] > vcc.LDS_CLUSTERS), key=lambda n: (n.split("_p")[1], n))
    small = [n for n, p in CASES if p.shape[0] <= vcc.LDS_CLUSTERS]
    order = small[:3]
    rest = small[3:]
    for k, b in enumerate(big):
        order.append(b)
        if k != 4:  # big[4] and big[5] stay adjacent
            order.append(rest.pop(0))
    return order + rest


def test_one_batch_of_all_families(gpu_lib):
    order = batch_order()
    assert sorted(order) == sorted(BY_NAME)
    rows = [BY_NAME[n].shape[0] for n in order]
    big = [k for k, r in enumerate(rows) if r > vcc.LDS_CLUSTERS]
    assert any(rows[a] == 2049 and rows[a + 2] == 2600 and rows[a + 1] < 100 for a in big if a + 2 < len(rows))
    assert any(b - a == 1 for a, b in zip(big, big[1:])) and min(rows) <= 1
    got = device_cluster([BY_NAME[n] for n in order])
    for name, g in zip(order, got):
        assert np.array_equal(g, oracle_roots(name)), name
        one, = device_cluster([BY_NAME[name]])
        assert np.array_equal(g, one), name


def test_more_workgroups_than_compute_units(gpu_lib):
    rng = np.random.default_rng(41)
    prefs = [rng.random((int(rng.integers(20, 81)), 100)) < rng.choice(vcc.RANDOM_P) for _ in range(600)]
    got = device_cluster(prefs)
    assert len(got) == 600
    for k, (p, g) in enumerate(zip(prefs, got)):
        assert np.array_equal(g, host_cluster(gpu_lib, p)), k
    for k in range(0, 600, 20):  # 30 of them against the oracle
        assert np.array_equal(got[k], vo.cluster(prefs[k])), k
    assert len({tuple(g.tolist()) for g in got}) > 100  # not all trivial


def test_no_state_leaks_between_workgroups_or_calls(gpu_lib):
    a, b, c = BY_NAME["random_n2049_p0.05"], BY_NAME["random_n65_p0.3"], BY_NAME["random_n2600_p0.3"]
    assert a.shape[0] > vcc.LDS_CLUSTERS and c.shape[0] > vcc.LDS_CLUSTERS
    want = [oracle_roots("random_n2049_p0.05"), oracle_roots("random_n65_p0.3"), oracle_roots("random_n2600_p0.3")]
    got = device_cluster([a, b, a, c, b, c, a])  # the same images more than once in one batch
    for g, k in zip(got, (0, 1, 0, 2, 1, 2, 0)):
        assert np.array_equal(g, want[k])
    # a large call, a small one, the large one again: one context, buffers and global state reused
    first = device_cluster([c, a])
    small, = device_cluster([b])
    again = device_cluster([c, a])
    assert np.array_equal(small, want[1])
    for x, y, w in zip(first, again, (want[2], want[0])):
        assert np.array_equal(x, w) and np.array_equal(y, w)


def test_images_of_no_rows_and_one_row(gpu_lib):
    b = BY_NAME["random_n65_p0.3"]
    empty, one = np.zeros((0, 100), bool), np.ones((1, 100), bool)
    got = device_cluster([empty, one, b, empty, one, empty])
    assert [g.tolist() for g in got[:2]] == [[], [0]] and [g.tolist() for g in got[3:]] == [[], [0], []]
    assert np.array_equal(got[2], oracle_roots("random_n65_p0.3"))
    assert [g.tolist() for g in device_cluster([empty, empty])] == [[], []]


def test_rejections_leave_a_working_context(gpu_lib):
    from limap_amd import vplib
    ctx = vplib._context()
    good = BY_NAME["random_n64_p0.3"]
    words = words_of(good)
    n, w = words.shape
    i64p, u64p, i32p = C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
    roots = np.zeros(n, np.int32)
    P, R = words.ctypes.data_as(u64p), roots.ctypes.data_as(i32p)

    def off(*v):
        a = np.array(v, np.int64)
        return a, a.ctypes.data_as(i64p)

    o_good, _ = off(0, n)
    o_two, _ = off(0, 40, n)
    o_dec, _ = off(0, 50, 40, n)
    o_start, _ = off(1, n)
    o_huge, _ = off(0, (1 << 30) - 1)   # 2^30 - 1 rows of 8 words: above 2^32 words, refused before pref is read
    o_rows, _ = off(0, 1 << 30)         # more rows than an image may have
    o_neg, _ = off(0, -1)
    bad = [
        (1, o_good, w, None, R), (1, o_good, w, P, None), (1, None, w, P, R),
        (3, o_dec, w, P, R), (1, o_neg, w, P, R), (1, o_start, w, P, R), (-1, o_good, w, P, R),
        (1, o_good, 0, P, R), (1, o_good, -3, P, R), (1, o_good, (1 << 14) + 1, P, R),
        (1, o_huge, 8, P, R), (1, o_rows, 1, P, R),
    ]
    for n_img, o, nw, p, r in bad:
        op = None if o is None else o.ctypes.data_as(i64p)
        rc = ctx.L.lt_vp_cluster_sets(ctx.h, n_img, op, nw, p, r)
        assert rc == -2, (n_img, None if o is None else o.tolist(), nw)  # LT_ERR_ARGUMENT
        with pytest.raises(ValueError, match=r"^lt_vp_cluster_sets: "):
            ctx.chk(rc)
        roots[:] = -7
        assert ctx.L.lt_vp_cluster_sets(ctx.h, 2, o_two.ctypes.data_as(i64p), w, P, R) == 0
        assert np.array_equal(roots[:40], vo.cluster(good[:40])) and np.array_equal(roots[40:], vo.cluster(good[40:]))
    assert ctx.L.lt_vp_cluster_sets(None, 1, o_good.ctypes.data_as(i64p), w, P, R) == -2
    # n_words at its upper limit is legal
    wide = np.zeros((3, 1 << 14), np.uint64)
    wide[0, -1] = wide[2, -1] = np.uint64(1) << np.uint64(63)
    assert [g.tolist() for g in vplib._cluster_sets([wide])] == [[0, 1, 0]]
