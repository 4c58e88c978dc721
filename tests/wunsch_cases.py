"""Inputs shared by tests/test_match_wunsch_host.py and tests/test_gpu_match_wunsch.py: random SOLD2 descinfos
[desc (dim, S N), valid (N, S)] and the hand-made cases that pin the definitions of DESIGN section 17 ("SOLD2")."""
import numpy as np


def rand_descinfo(rng, n, S=5, dim=128, prefix=True, min_valid=2, scale=1.0):
    """unit descriptors (times `scale`); valid: a prefix of min_valid..S samples per line (what the sampler writes), or
    an arbitrary non-empty subset.  The padded samples carry descriptors like any other: only the mask hides them."""
    d = rng.standard_normal((dim, S * n))
    d /= np.maximum(np.linalg.norm(d, axis=0, keepdims=True), 1e-30)
    d *= scale
    if prefix:
        v = np.arange(S)[None, :] < rng.integers(min(min_valid, S), S + 1, n)[:, None]
    else:
        v = rng.random((n, S)) < 0.6
        v[np.arange(n), rng.integers(0, S, n)] = True
    return [np.ascontiguousarray(d, np.float32), np.ascontiguousarray(v.reshape(n, S))]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def one_hot(dim, k, sign=1.0):
    e = np.zeros(dim, np.float32)
    e[k] = sign
    return e


def pack(lines, S, dim):
    """lines: per line a list of S entries, each a (dim,) vector (valid sample) or None (padded: a descriptor of ones)"""
    n = len(lines)
    d = np.ones((dim, S * n), np.float32)
    v = np.zeros((n, S), bool)
    for i, ln in enumerate(lines):
        assert len(ln) == S
        for s, x in enumerate(ln):
            if x is not None:
                d[:, i * S + s] = x
                v[i, s] = True
    return [d, v]


def tie_case(rng, S=5, dim=128):
    """image 2 repeats whole lines, so line scores tie exactly, within a tile of 4 lines and across tiles"""
    a = rand_descinfo(rng, 21, S, dim)
    base = rand_descinfo(rng, 6, S, dim)
    pick = rng.integers(0, 6, 40)
    d = base[0].reshape(dim, 6, S)[:, pick, :].reshape(dim, -1)
    return a, [np.ascontiguousarray(d), base[1][pick].copy()]


def antipodal_case(dim=8):
    """S = 2.  Image 1: line 0 = (e0, e1), line 1 = (e0, padded).  Image 2: line 0 = (-e0, padded) -- the point scores of
    line 0 against it are exactly -1.0f (valid, dropped like a masked one) and 0; of line 1 only -1.0f: an all -1 block.
    Line 1 = (e1, e0) for contrast."""
    e0, e1 = one_hot(dim, 0), one_hot(dim, 1)
    img1 = pack([[e0, e1], [e0, None]], 2, dim)
    img2 = pack([[-e0, None], [e1, e0]], 2, dim)
    return img1, img2


def below_minus_one_case(rng, S, masked, dim=16):
    """descriptors that are not unit vectors, so that point scores go far below -1.0f: a maximum of real scores below
    -1.0f is a real term of the mean (only a maximum that EQUALS -1.0f is dropped), and no padded slot may replace it.
    Image 1 holds lines of one direction scaled by 2 to 4, image 2 lines of roughly the opposite direction, so whole
    blocks are below -1; the first lines are the reviewer-sized example: 2 e0 in every sample against -e0 in every
    sample, L = -2.0f.  masked: some samples are hidden (arbitrary subsets), else all are valid."""
    n1, n2 = 9, 11
    base_dir = rng.standard_normal(dim)
    base_dir /= np.linalg.norm(base_dir)
    d1 = (base_dir[:, None] + 0.1 * rng.standard_normal((dim, S * n1))) * rng.uniform(2.0, 4.0, S * n1)
    d2 = (-base_dir[:, None] + 0.1 * rng.standard_normal((dim, S * n2))) * rng.uniform(1.5, 2.5, S * n2)
    d1[:, :S] = 2.0 * one_hot(dim, 0)[:, None]
    d2[:, :S] = -one_hot(dim, 0)[:, None]
    d2[:, S * (n2 - 3):] *= -1.0  # the last three lines score far above 1 instead
    v1, v2 = np.ones((n1, S), bool), np.ones((n2, S), bool)
    if masked:
        v1[1:] = rng.random((n1 - 1, S)) < 0.6
        v1[np.arange(n1), rng.integers(0, S, n1)] = True
        v2[1:] = rng.random((n2 - 1, S)) < 0.6
        v2[np.arange(n2), rng.integers(0, S, n2)] = True
    return [np.ascontiguousarray(d1, np.float32), v1], [np.ascontiguousarray(d2, np.float32), v2]


DEFINITION_CASES = ("ties", "antipodal", "few_lines", "masks_S2", "masks_S5", "masks_S8", "below_S2", "below_S5",
                    "below_S2_masked", "below_S5_masked", "below_S8_masked")


def definition_case(name):
    """-> (descinfo1, descinfo2, S, topk, top_k_candidates)"""
    rng = np.random.default_rng([31, DEFINITION_CASES.index(name)])
    if name == "ties":
        a, b = tie_case(rng)
        return a, b, 5, 10, 10
    if name == "antipodal":
        a, b = antipodal_case()
        return a, b, 2, 10, 10
    if name == "few_lines":  # N2 < topk and N2 < top_k_candidates
        return rand_descinfo(rng, 19), rand_descinfo(rng, 3), 5, 10, 10
    if name.startswith("below"):
        S = int(name.split("_")[1][1:])
        a, b = below_minus_one_case(rng, S, name.endswith("masked"))
        return a, b, S, 10, 10
    S = int(name[-1])
    return rand_descinfo(rng, 18, S, 128, prefix=False), rand_descinfo(rng, 23, S, 128, prefix=False), S, 10, 10
