"""Preference matrices for the J-Linkage clustering, shared by tests/test_vp_host.py (the host
twin lt_fn_vp_cluster_host) and tests/test_gpu_vp_cluster.py (k_vp_cluster through lt_vp_cluster_sets).  Plain numpy, no
GPU, every input from a seeded generator.  Each family returns a list of (name, bool matrix n x M); tests/vp_oracle.py:
cluster is the reference for all of them.

The constants the shapes aim at (limap_amd/csrc/lt_vp.h): a wave has 64 lanes and scan_row strides the partners of a row
by 64; k_vp_cluster has 512 lanes = 8 waves and strides rows by 512 (arg-max, merge pass) or by 8 (scans); the
per-cluster state moves from LDS to global memory above kVpLdsClusters = 2048 rows; a preference set is W = ceil(M / 64)
words."""
import numpy as np

LDS_CLUSTERS = 2048  # kVpLdsClusters: images with more rows keep the state in global memory
LARGE_N = 2047       # from here on the oracle takes seconds per case


def pack(pref):
    """(n, M) bool -> (n, ceil(M / 64)) uint64, bit m of a row in word m // 64 at position m % 64"""
    pref = np.asarray(pref, bool)
    n, m = pref.shape
    w = max((m + 63) // 64, 1)
    padded = np.zeros((n, 64 * w), bool)
    padded[:, :m] = pref
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view("<u8").reshape(n, w).astype(np.uint64)


def _from_sets(sets, m):
    p = np.zeros((len(sets), m), bool)
    for k, s in enumerate(sets):
        p[k, list(s)] = True
    return p


def ties():
    """n identical non-empty sets: every pair has ratio 1, so vp_better's index order decides every step alone -- in
    the lanes of scan_row, in wave_best and across the waves in block_best"""
    out = []
    for n in (2, 3, 64, 65, 130):
        p = np.zeros((n, 8), bool)
        p[:, [0, 3, 5]] = True
        out.append((f"ties_n{n}", p))
    return out


def nested_chain():
    """S_k = {0..k}: (0, 1) at 1/2 is not the first merge, the greatest ratio is (n - 2, n - 1) at (n - 1) / n, and every
    merge shrinks a late row, so rows k < i take the new pair (k, i) over their record (the `k < i` update branch)"""
    return [(f"chain_n{n}", np.tril(np.ones((n, n), bool))) for n in (5, 70, 130)]


def ring():
    """S_k = {k, k + 1 mod n}: every neighbouring pair at 1/3; row 0 meets row 1 and row n - 1 (the last lane of
    scan_row's last stride), the rest merge in index order"""
    out = []
    for n in (64, 65, 513):
        p = np.zeros((n, n), bool)
        p[np.arange(n), np.arange(n)] = True
        p[np.arange(n), (np.arange(n) + 1) % n] = True
        out.append((f"ring_n{n}", p))
    return out


def rescan():
    """The worst case of the "scan this row again" marks.

    `hub_high`: a leaf rows, then L hub rows.  Leaf k and hub l share the private bit l * a + k; leaves are disjoint from
    each other, hubs too.  Every pair (leaf, hub) has ratio 1 / (a + L - 1), so every leaf records hub 0, the smallest j.
    Step l merges (leaf l, hub l): hub l is j and goes, and every other leaf has `p == j` with k > i: it is marked -2,
    passes through the intersection with the merged set (0) and is scanned again in the final loop over the marked
    rows, where it finds hub l + 1.  L steps, a - 1 re-scans each.

    `hub_low`: a leaf rows, then L pairs (hub l, mate l).  Hub l = its private bits with the leaves + C common bits, mate
    l = the C common bits + one bit of its own: ratio C / (a + C + 1), far above a leaf's 1 / (a + L + C).  Step l
    merges (hub l, mate l) -> the C common bits, which no leaf has: every leaf has `p == i` with k < i, takes the
    `again && k < i` exit before the intersection and is scanned again, finding hub l + 1.  A last row shares a private
    bit with every leaf and has C + 1 bits of its own, so its ratio with a leaf is below every hub's: once the hubs are
    gone the re-scans find it, and leaf 0 merges with it -- a re-scan that is skipped or finds the wrong row shows."""
    out = []
    for a, L in ((30, 4), (200, 12), (600, 3)):
        p = np.zeros((a + L, a * L), bool)
        for l in range(L):
            p[np.arange(a), l * a + np.arange(a)] = True
            p[a + l, l * a:(l + 1) * a] = True
        out.append((f"rescan_hub_high_a{a}_L{L}", p))
    C_ = 5
    for a, L in ((30, 4), (200, 12), (600, 3)):
        m = a * L + (C_ + 1) * L + a + C_ + 1
        p = np.zeros((a + 2 * L + 1, m), bool)
        for l in range(L):
            common = a * L + (C_ + 1) * l
            p[np.arange(a), l * a + np.arange(a)] = True
            p[a + 2 * l, l * a:(l + 1) * a] = True
            p[a + 2 * l, common:common + C_] = True
            p[a + 2 * l + 1, common:common + C_ + 1] = True
        last = a * L + (C_ + 1) * L
        p[np.arange(a), last + np.arange(a)] = True
        p[a + 2 * L, last:] = True
        out.append((f"rescan_hub_low_a{a}_L{L}", p))
    return out


def far_partner():
    """the only intersecting partner of a row sits in a late lane of scan_row's stride and in a late wave of the
    arg-max: rows 0 and n - 1 are equal, rows 1 and n - 2 share one bit of two, the rest are private singletons"""
    out = []
    for n in (34, 64, 65, 66, 130, 600):
        p = np.zeros((n, n + 3), bool)
        p[np.arange(n), np.arange(n)] = True
        p[[0, n - 1], n] = True
        p[n - 1, n - 1] = False
        p[n - 1, 0] = True
        p[[1, n - 2], n + 1] = True
        out.append((f"far_n{n}", p))
    return out


def empty_sets():
    """empty preference sets (never merge) at row 0, at the last row and in runs, among sets that do merge"""
    rng = np.random.default_rng(31)
    out = [("empty_all_n5", np.zeros((5, 70), bool))]
    for n, m, dens in ((50, 40, 0.2), (140, 130, 0.1), (600, 64, 0.05)):
        p = rng.random((n, m)) < dens
        p[0] = False
        p[n - 1] = False
        p[10:20] = False
        p[n // 2:n // 2 + 3] = False
        out.append((f"empty_n{n}_m{m}", p))
    p = rng.random((70, 20)) < 0.3  # everything empty but two late rows
    p[:64] = False
    p[66:] = False
    p[64, 0] = p[65, 0] = True
    out.append(("empty_but_two", p))
    return out


def word_edges():
    """sets that live on the edges of the 64-bit words: only bit 63, only bit 64, only bit M - 1 (pairs of equal rows,
    so each bit must be seen to merge them), and a random matrix at every M"""
    rng = np.random.default_rng(32)
    out = []
    for m in (1, 63, 64, 65, 128, 5000):
        bits_ = sorted({min(63, m - 1), min(64, m - 1), m - 1, 0})
        sets = [{b} for b in bits_] + [{b} for b in reversed(bits_)]
        out.append((f"edge_bits_m{m}", _from_sets(sets, m)))
        n = 40
        p = rng.random((n, m)) < (0.5 if m == 1 else 0.08)
        p[:, m - 1] |= rng.random(n) < 0.3  # the last bit of the last word is in use
        out.append((f"edge_random_m{m}", p))
    return out


def disjoint_blocks():
    """40 groups of 5 to 60 rows that intersect only within their group (16 columns each), rows of all groups
    interleaved: many survivors, many rows without a partner"""
    rng = np.random.default_rng(33)
    sizes = rng.integers(5, 61, 40)
    n = int(sizes.sum())
    p = np.zeros((n, 16 * 40), bool)
    group = np.repeat(np.arange(40), sizes)[rng.permutation(n)]
    for k in range(n):
        cols = 16 * group[k] + np.nonzero(rng.random(16) < 0.4)[0]
        p[k, cols if cols.size else 16 * group[k]] = True
    return [("disjoint_40_groups", p)]


RANDOM_N = (1, 2, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 2600)
RANDOM_P = (0.01, 0.05, 0.3, 0.9)
# columns of the large members: fewer where the density makes the oracle's merge loop long (n - 1 merges at 0.9)
RANDOM_M_LARGE = {0.01: 320, 0.05: 200, 0.3: 130, 0.9: 65}


def random_density(large=True):
    """random bits at four densities, row counts on the edges of a wave (64), of the workgroup (512) and of the LDS
    state (2048).  large=False leaves out the members of LARGE_N rows and more"""
    out = []
    for n in RANDOM_N:
        if n >= LARGE_N and not large:
            continue
        for dens in RANDOM_P:
            m = RANDOM_M_LARGE[dens] if n >= LARGE_N else 100
            rng = np.random.default_rng([34, n, int(dens * 100)])
            out.append((f"random_n{n}_p{dens}", rng.random((n, m)) < dens))
    return out


FAMILIES = dict(ties=ties, nested_chain=nested_chain, ring=ring, rescan=rescan, far_partner=far_partner,
                empty_sets=empty_sets, word_edges=word_edges, disjoint_blocks=disjoint_blocks,
                random_density=random_density)


def all_cases(large=True):
    """every family's cases in one list, names unique"""
    out = []
    for name, fn in FAMILIES.items():
        out += fn(large) if name == "random_density" else fn()
    assert len({c[0] for c in out}) == len(out)
    return out
