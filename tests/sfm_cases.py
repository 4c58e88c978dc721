"""Case generators of the limap_amd.pointsfm tests (test_sfm_host.py against sfm_oracle.py, test_gpu_sfm.py device
against host).  A case is a model dict as sfm_oracle.py takes it.  Geometry: "far" cameras stand on a ring or a grid
with baselines >= 0.5 m around points at most 10 m away (triangulation angles of degrees); a "coincident" camera stands
1 mm from another one (<= 0.02 degrees); the gate of the tests is 1 degree.  `checked` asserts that no percentile angle
lies within 1e-5 rad of that gate, so the last bit of an arccosine cannot decide a list."""
import math

import numpy as np

import sfm_oracle as so

GATE_DEG = 1.0


def rotations(rng, n):
    """random rotation matrices (the centres, not the axes, matter: T = -R C)"""
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).reshape(n, 3, 3)


def model_of(rng, centres, xyz, tracks, img_ids=None):
    centres = np.asarray(centres, float).reshape(-1, 3)
    n = centres.shape[0]
    R = rotations(rng, n)
    T = -np.einsum("nij,nj->ni", R, centres)
    return {"img_ids": list(range(n)) if img_ids is None else [int(i) for i in img_ids], "R": R, "T": T,
            "xyz": np.asarray(xyz, float).reshape(-1, 3), "tracks": [np.asarray(t, np.int32).reshape(-1) for t in tracks]}


def checked(model, want_lists=True):
    """the condition on the inputs: every percentile angle is at least 1e-5 rad away from the gate"""
    table = so.pair_table(model, want_lists)
    th = float(so.gate_threshold(GATE_DEG))
    if table[2].size:
        assert np.abs(table[2].astype(np.float64) - th).min() > 1e-5
    model["table"] = table
    return model


def sites(n, n_sites, radius=5.0):
    """n cameras spread over n_sites places on a ring (metres apart); the cameras of one place stand within 1 mm, 0.01 mm
    from one another"""
    c = ring(n_sites, radius)[np.arange(n) % n_sites]
    c[:, 0] += 1e-5 * (np.arange(n) // n_sites)
    return c


def ring(n, radius=4.0, z=0.0):
    a = 2 * math.pi * np.arange(n) / max(n, 1)
    return np.stack([radius * np.cos(a), radius * np.sin(a), np.full(n, z)], 1)


def cloud(rng, p, spread=1.0):
    return rng.uniform(-spread, spread, size=(p, 3))


def to_arrays(model):
    tracks = model["tracks"]
    off = np.zeros(len(tracks) + 1, np.int64)
    if tracks:
        off[1:] = np.cumsum([len(t) for t in tracks])
    img = np.concatenate(tracks).astype(np.int32) if off[-1] else np.zeros(0, np.int32)
    return model["img_ids"], model["R"], model["T"], model["xyz"], off, img


# ---- empty and degenerate ----
def no_points(seed=0):
    rng = np.random.default_rng(seed)
    return checked(model_of(rng, ring(3), np.zeros((0, 3)), []))


def degenerate(seed=1):
    """tracks of length 0 and 1, image 4 in no track, a track naming image 2 twice, one naming only image 1, one with a
    repeat next to a real pair"""
    rng = np.random.default_rng(seed)
    tracks = [[], [0], [2, 2], [1, 1, 1], [0, 1, 0], [0, 3], [3, 1, 2], []]
    return checked(model_of(rng, ring(5), cloud(rng, len(tracks)), tracks))


def single_image(seed=2):
    rng = np.random.default_rng(seed)
    return checked(model_of(rng, ring(1), cloud(rng, 3), [[0], [0, 0], []]))


def all_skipped(seed=3):
    """every slot is skipped: no pair record at all although E > 0"""
    rng = np.random.default_rng(seed)
    return checked(model_of(rng, ring(3), cloud(rng, 3), [[1, 1], [2, 2, 2], [0, 0]]))


def repeated(tracks, seed=10):
    """tracks that name their images more than once: shared exceeds n_i + n_j and an IoU is negative ([0, 0, 0, 1, 1, 2]:
    6 / (3 + 2 - 6)) or +inf ([0, 0, 1, 1, 2]: 4 / (2 + 2 - 4)); image 2 gives images 0 and 1 a second partner to rank"""
    rng = np.random.default_rng(seed)
    return checked(model_of(rng, ring(5), cloud(rng, len(tracks)), tracks))


def repeated_negative():
    return repeated([[0, 0, 0, 1, 1, 2], [3, 4]])


def repeated_infinite():
    return repeated([[0, 0, 1, 1, 2], [3, 4], [4, 3, 3]])


# ---- percentile rounding ----
PERCENTILE_COUNTS = (1, 2, 3, 4, 7, 15, 16)


def percentile(seed=4):
    """image pair (2 k, 2 k + 1) shares exactly PERCENTILE_COUNTS[k] points, with distinct angles"""
    rng = np.random.default_rng(seed)
    n = 2 * len(PERCENTILE_COUNTS)
    tracks = []
    for k, c in enumerate(PERCENTILE_COUNTS):
        tracks += [[2 * k, 2 * k + 1]] * c
    m = checked(model_of(rng, ring(n), cloud(rng, len(tracks)), tracks))
    lists = m["table"][3]
    for k, c in enumerate(PERCENTILE_COUNTS):
        a = lists[(2 * k, 2 * k + 1)]
        assert len(a) == c and len(set(a.tolist())) == c
    # a pick by rint (halves to even) would return another value at n = 7 and n = 15
    assert lists[(8, 9)][5] != lists[(8, 9)][4] and lists[(10, 11)][11] != lists[(10, 11)][10]
    return m


# ---- triangular decode ----
def landmark(seed=5, n=2100, extra=200):
    """one point seen by all n images (n (n - 1) / 2 = 2.2 M slots) and `extra` ordinary points; the images stand at 21
    places, so a pair is either metres or a fraction of a millimetre apart"""
    rng = np.random.default_rng(seed)
    tracks = [rng.permutation(n)]
    for _ in range(extra):
        tracks.append(rng.choice(n, size=int(rng.integers(2, 13)), replace=False))
    return checked(model_of(rng, sites(n, 21), cloud(rng, len(tracks)), tracks), want_lists=False)


def slot_boundary(delta, seed=6):
    """E = 256 + delta slots (delta in -1, 0, 1): the last slot ends below, on and above a workgroup boundary"""
    rng = np.random.default_rng(seed)
    tracks = [rng.permutation(24)[:23], [3, 7, 11]]     # 253 + 3 slots
    if delta == -1:
        tracks[1] = [3, 7]                              # 253 + 1
        tracks.append([5, 9])                           # + 1
    elif delta == 1:
        tracks.append([5, 9])
    m = checked(model_of(rng, ring(24), cloud(rng, len(tracks)), tracks))
    assert sum(len(t) * (len(t) - 1) // 2 for t in m["tracks"]) == 256 + delta
    return m


# ---- ties ----
def tie_ring(seed=7, n=12, per_pair=3):
    """image k shares per_pair points with each of k +- 1 and k +- 2 and sees nothing else: four partners, one score"""
    rng = np.random.default_rng(seed)
    tracks = []
    for k in range(n):
        for d in (1, 2):
            tracks += [[k, (k + d) % n]] * per_pair
    m = checked(model_of(rng, ring(n), cloud(rng, len(tracks), 0.5), tracks))
    assert (m["table"][1] == per_pair).all() and len(set(so.num_points(m))) == 1
    return m


# ---- select rounds, gate ----
def star(partners, seed=8, coincident=0):
    """image 0 shares 1 .. 5 points with every image 1 .. partners; the last `coincident` of them stand 1 mm from
    image 0 and are gated out"""
    rng = np.random.default_rng(seed + partners)
    c = ring(partners + 1, radius=5.0)
    c[0] = (0.0, 0.0, 6.0)
    for k in range(partners + 1 - coincident, partners + 1):
        c[k] = c[0] + (0.001, 0.0, 0.0)
    tracks = []
    for k in range(1, partners + 1):
        tracks += [[0, k]] * int(rng.integers(1, 6))
    return checked(model_of(rng, c, cloud(rng, len(tracks)), tracks))


def all_gated(seed=9):
    """images 1 .. 3 stand 1 mm from image 0 and are its only partners; they also see the far images 4 .. 6"""
    rng = np.random.default_rng(seed)
    c = ring(7)
    for k in (1, 2, 3):
        c[k] = c[0] + (0.001 * k, 0.0, 0.0)
    tracks = [[0, 1], [0, 2], [0, 3], [0, 1, 2], [1, 4], [2, 5, 4], [3, 6], [1, 5], [4, 5, 6], [2, 6]]
    m = checked(model_of(rng, c, cloud(rng, len(tracks)), tracks))
    assert so.neighbors_idx(m, 10, GATE_DEG, "iou", m["table"])[0] == []
    return m


# ---- randomised ----
def random_model(seed, n=None, p=None):
    """n in [2, 64] images on a jittered grid 0.6 m apart, every fourth one 1 mm from its predecessor; p in [1, 2000]
    points 3 - 10 m in front with tracks of 2 - 12 images"""
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(2, 65)) if n is None else n
    p = int(rng.integers(1, 2001)) if p is None else p
    c = np.stack([0.6 * (np.arange(n) % 8), 0.6 * (np.arange(n) // 8), np.zeros(n)], 1) + rng.uniform(-0.02, 0.02, (n, 3))
    for k in range(3, n, 4):
        c[k] = c[k - 1] + (0.001, 0.0, 0.0)
    xyz = np.stack([rng.uniform(0, 4.2, p), rng.uniform(0, 4.2, p), rng.uniform(3, 10, p)], 1)
    tracks = [rng.choice(n, size=min(n, int(rng.integers(2, 13))), replace=False) for _ in range(p)]
    ids = rng.permutation(3 * n)[:n]
    return checked(model_of(rng, c, xyz, tracks, img_ids=ids))


def hand_built():
    """4 images, 6 points; image 3 stands 1 mm from image 0.  Registered ids 5, 3, 8, 1.
    ComputeNumPoints 4, 5, 3, 2.  shared: (0,1) 3, (0,2) 1, (0,3) 2, (1,2) 3, (1,3) 1; (0,3) is gated out.
    IoU      image 0: 1 -> 3/6, 2 -> 1/6            image 1: 2 -> 3/5, 0 -> 3/6, 3 -> 1/6
             image 2: 1 -> 3/5, 0 -> 1/6            image 3: 1 -> 1/6
    Dice     image 0: 1 -> 6/9, 2 -> 2/7            image 1: 2 -> 6/8, 0 -> 6/9, 3 -> 2/7
    overlap  image 1: 0 -> 3 and 2 -> 3 tie: the smaller index first"""
    eye = np.tile(np.eye(3), (4, 1, 1))
    c = np.array([[0.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0], [0.001, 0, 0]])
    xyz = np.array([[0.2, 0.1, 5], [1.0, -0.2, 5], [1.6, 0.3, 5], [0.1, 0.2, 5], [0.4, -0.1, 5], [1.4, 0.0, 5]])
    tracks = [[0, 1], [0, 1, 2], [1, 2], [0, 3], [0, 1, 3], [2, 1]]
    model = {"img_ids": [5, 3, 8, 1], "R": eye, "T": -c, "xyz": xyz, "tracks": [np.array(t, np.int32) for t in tracks]}
    expect = {
        "num_points": [4, 5, 3, 2],
        "shared": [{1: 3, 2: 1, 3: 2}, {0: 3, 2: 3, 3: 1}, {0: 1, 1: 3}, {0: 2, 1: 1}],
        "iou": {1: [3], 3: [8, 5, 1], 5: [3, 8], 8: [3, 5]},
        "dice": {1: [3], 3: [8, 5, 1], 5: [3, 8], 8: [3, 5]},
        "overlap": {1: [3], 3: [5, 8, 1], 5: [3, 8], 8: [3, 5]},
    }
    return model, expect
