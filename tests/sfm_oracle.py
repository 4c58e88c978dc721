"""DESIGN.md section 21 (limap_amd.pointsfm) restated in NumPy with every float32 / float64 step explicit: written from
the definition, not from the library's C++.  A model here is a dict: ``R`` (N, 3, 3), ``T`` (N, 3), ``xyz`` (P, 3) in any
float type (narrowed to float32 as the model stores them), ``tracks`` a list of P integer sequences of image indices,
``img_ids`` the N registered ids."""
import math

import numpy as np

PERCENTILE = 0.75


def centres(R, T):
    """C = -R^T T in float32, then widened"""
    R = np.asarray(R, np.float64).astype(np.float32).reshape(-1, 3, 3)
    T = np.asarray(T, np.float64).astype(np.float32).reshape(-1, 3)
    C = np.zeros((R.shape[0], 3), np.float32)
    for c in range(3):
        s = (-R[:, 0, c]) * T[:, 0]
        s = s + (-R[:, 1, c]) * T[:, 1]
        s = s + (-R[:, 2, c]) * T[:, 2]
        assert s.dtype == np.float32
        C[:, c] = s
    return C.astype(np.float64)


def sq_norm(d):
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]


def angles(ci, cj, x):
    """triangulation angles of the points x seen from the centres ci, cj (float64 arrays) -> float32"""
    b2, r1, r2 = sq_norm(ci - cj), sq_norm(x - ci), sq_norm(x - cj)
    den = 2.0 * np.sqrt(r1 * r2)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.clip((r1 + r2 - b2) / den, -1.0, 1.0)
        a = np.abs(np.arccos(q))
    a = np.minimum(a, np.pi - a)
    return np.where(den == 0.0, 0.0, a).astype(np.float32)


def percentile_index(n):
    idx = int(math.floor(PERCENTILE * (n - 1) + 0.5))  # round, halves away from zero (the argument is >= 0)
    assert idx == (3 * (n - 1) + 2) // 4
    return idx


def num_points(model):
    n = len(model["img_ids"])
    out = [0] * n
    for t in model["tracks"]:
        for i in t:
            if not 0 <= int(i) < n:
                raise IndexError(int(i))
            out[int(i)] += 1
    return out


def pair_table(model, want_lists=True):
    """-> ij (U, 2) ascending with i < j, shared (U,), percentile angle (U,) float32, and the per-pair ascending angle
    lists (for the tests of the percentile pick; None without want_lists)"""
    n = len(model["img_ids"])
    C = centres(model["R"], model["T"])
    X = np.asarray(model["xyz"], np.float64).astype(np.float32).astype(np.float64).reshape(-1, 3)
    num_points(model)  # raises on a bad index
    keys, angs = [np.zeros(0, np.int64)], [np.zeros(0, np.float32)]
    for p, t in enumerate(model["tracks"]):
        t = np.asarray(t, np.int64).reshape(-1)
        if t.size < 2:
            continue
        a, b = np.tril_indices(t.size, -1)  # every a > b
        i, j = t[a], t[b]
        keep = i != j
        i, j = i[keep], j[keep]
        keys.append(np.minimum(i, j) * n + np.maximum(i, j))
        angs.append(angles(C[i], C[j], X[p][None, :]))
    keys, angs = np.concatenate(keys), np.concatenate(angs)
    order = np.lexsort((angs, keys))
    keys, angs = keys[order], angs[order]
    uniq, first, count = np.unique(keys, return_index=True, return_counts=True)
    ij = np.stack([uniq // n, uniq % n], 1).astype(np.int64) if uniq.size else np.zeros((0, 2), np.int64)
    idx = np.floor(PERCENTILE * (count - 1) + 0.5).astype(np.int64)  # round, halves away from zero
    assert np.array_equal(idx, (3 * (count - 1) + 2) // 4)
    assert all(percentile_index(c) == i for c, i in zip(count[:64].tolist(), idx[:64].tolist()))
    pick = angs[first + idx].astype(np.float32)
    lists = {(int(u // n), int(u % n)): angs[f:f + c] for u, f, c in zip(uniq, first, count)} if want_lists else None
    return ij, count.astype(np.int64), pick, lists


def gate_threshold(min_triangulation_angle):
    return np.float32(float(min_triangulation_angle) * (math.pi / 180.0))


def scores(kind, shared, n_i, n_j):
    """int64 arrays -> the score of every (image, partner) entry: an integer for "overlap", else a float64 quotient.
    A track that names its images more than once can make shared exceed n_i + n_j: the IoU is then negative, or +inf
    (IEEE division; shared >= 1, so never NaN)"""
    if kind == "overlap":
        return shared.astype(np.int64)
    if kind == "iou":
        with np.errstate(divide="ignore"):
            return shared.astype(np.float64) / (n_i + n_j - shared).astype(np.float64)
    if kind == "dice":
        return (2 * shared).astype(np.float64) / (n_i + n_j).astype(np.float64)
    raise NotImplementedError(kind)


def neighbors_idx(model, num_images, min_triangulation_angle, kind, table=None):
    """per image index the ordered neighbour indices"""
    n = len(model["img_ids"])
    ij, shared, pick, _ = table if table is not None else pair_table(model)
    npts = np.asarray(num_points(model), np.int64)
    kept = pick.astype(np.float32) >= gate_threshold(min_triangulation_angle)
    ij, shared = ij[kept], shared[kept]
    img = np.concatenate([ij[:, 0], ij[:, 1]])       # every kept pair is an entry of both of its images
    partner = np.concatenate([ij[:, 1], ij[:, 0]])
    sc = scores(kind, np.concatenate([shared, shared]), npts[img], npts[partner])
    order = np.lexsort((partner, -sc, img))          # per image: score descending, equal scores by ascending index
    img, partner = img[order], partner[order]
    first = np.searchsorted(img, np.arange(n + 1))
    return [partner[first[k]:first[k] + min(first[k + 1] - first[k], int(num_images))].tolist() for k in range(n)]


def neighbors(model, num_images, min_triangulation_angle, kind, table=None):
    """-> dict registered id -> list of registered ids, keys ascending"""
    ids = [int(i) for i in model["img_ids"]]
    lists = neighbors_idx(model, num_images, min_triangulation_angle, kind, table)
    out = {i: [] for i in sorted(ids)}
    for k, lst in enumerate(lists):
        out[ids[k]].extend(ids[j] for j in lst)
    return out


def shared_points(model, table=None):
    ij, shared, _, _ = table if table is not None else pair_table(model)
    out = [dict() for _ in model["img_ids"]]
    for (i, j), s in zip(ij.tolist(), shared.tolist()):
        out[i][j] = s
        out[j][i] = s
    return [dict(sorted(d.items())) for d in out]


def robust_index(size, p):
    """size_t(float(size) * float(p)), None where it is undefined (negative, NaN) or past the data"""
    v = np.float32(size) * np.float32(p)
    assert v.dtype == np.float32
    if not (v >= 0) or not (v < np.float32(size)) or int(v) >= size:
        return None
    return int(v)


def ranges(model, range_robust, k_stretch):
    X = np.asarray(model["xyz"], np.float64).astype(np.float32).reshape(-1, 3)
    size = X.shape[0]
    if size == 0 or not np.isfinite(X).all():
        raise ValueError("undefined")
    i_lo, i_hi = robust_index(size, range_robust[0]), robust_index(size, range_robust[1])
    if i_lo is None or i_hi is None:
        raise ValueError("undefined")
    k = np.float32(k_stretch)
    lo, hi = np.zeros(3), np.zeros(3)
    for c in range(3):
        data = np.sort(X[:, c])
        first, second = data[i_lo], data[i_hi]
        diff = second - first
        first = first - k * diff
        second = second + k * diff
        assert first.dtype == np.float32 and second.dtype == np.float32
        lo[c], hi[c] = float(first), float(second)
    return lo, hi
