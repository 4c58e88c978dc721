"""Track-line sets for the device half of RemergeLineTracks (k_track_connect through lt_fn_track_connect; DESIGN.md section
4, *Post-processing*), shared by tests/test_tracks_host.py (every builder and its assertions, no GPU) and
tests/test_gpu_track_connect.py.
Plain numpy plus the CPU oracle's batched predicate (oracle.linker3d_check_pairs: LineLinker3d::check_connection in
spatial-merging mode); every input from fixed constants or a seeded generator.

A case is (name, line7 (T, 7), active (T,) bool, linker dict, capacity0, facts dict).  `expected_edges` restates the pair
loop of merging/merging.cc:519-556 and is the reference for all of them; every builder asserts on it the property the case
exists for, so a case cannot silently stop being the case it claims.

The constants the shapes aim at (limap_amd/csrc/lt_kernels.hip, lt_tracks.cpp): a workgroup holds 256 tracks i (four waves
of 64) and sweeps a chunk of 64 tracks j; a wave queues its cosine-test survivors in 64 x 64 = 4096 slots; the host reads
the edge counter and the first 4095 edges in one copy, the rest in a second; the first launch has room for
max(65536, 32 T) edges unless capacity0 says otherwise.

Symmetry.  In spatial-merging mode (angle, bi-directional overlap, smart angle, inner-segment distance) every term of
check_connection is a symmetric function of the two lines bit for bit -- products commute, max / max_element over the same
values -- as long as no operand is NaN: short segments inside long ones and partial overlaps near th_overlap /
th_smartoverlap give check(a, b) == check(b, a), and `orientation` asserts that.  The one operand that breaks it is the
uncertainty: std::min(u1, u2) returns its FIRST argument when either is NaN, so a line with a NaN uncertainty is rejected
as l1 (sigma NaN) and judged on its geometry as l2.  Those are the asymmetric pairs of `orientation`."""
import functools
import math

import numpy as np

from oracle import oracle as ora

CHUNK = 64        # kTrackChunk: tracks j per workgroup column
BLOCK = 256       # tracks i per workgroup
QUEUE = 4096      # s_q entries per wave
FIRST = 4095      # kFirst of lt_tracks.cpp: edges that come back with the counter

# angle / overlap / inner-segment gates of ordinary size; every line below has uncertainty 1 unless it says otherwise, so
# the inner-segment gate is dist <= th_innerseg
LINKER = dict(score_th=0.5, th_angle=5.0, th_overlap=0.1, th_smartoverlap=0.3, th_smartangle=1.0, th_perp=1.0,
              th_innerseg=0.1, use_smartangle=True)

_EXPECTED = {}


def directed_pairs(T, active):
    """the (i, j) that merging.cc:523-540 tests: active i, j != i, one side per unordered pair by the parity of i + j
    when every track is active"""
    active = np.asarray(active, bool)
    i, j = np.meshgrid(np.arange(T), np.arange(T), indexing="ij")
    m = active[:, None] & (i != j)
    if active.all():
        even = ((i + j) & 1) == 0
        m &= ~((i < j) & even) & ~((i > j) & ~even)
    return i[m], j[m]


def directed_hits(line7, active, linker):
    """(i, j) of directed_pairs with check_connection(l_i, l_j), in that order"""
    line7 = np.asarray(line7, np.float64).reshape(-1, 7)
    i, j = directed_pairs(len(line7), active)
    ok = ora.linker3d_check_pairs(linker, line7[i], line7[j]) if len(i) else np.zeros(0, bool)
    return i[ok], j[ok]


def edges_of(i, j):
    e = np.stack([np.minimum(i, j), np.maximum(i, j)], 1).astype(np.int64).reshape(-1, 2)
    return np.unique(e, axis=0) if len(e) else e


def expected_edges(line7, active, linker):
    """merging.cc:519-556: (E, 2) int64 (min, max), sorted and unique"""
    return edges_of(*directed_hits(line7, active, linker))


def expected(case):
    """dict(edges, n_raw) of a case, computed once per name and never modified by its users; n_raw = hits of the directed
    loop = what the device counter must hold"""
    name, line7, active, linker = case[:4]
    if name not in _EXPECTED:
        i, j = directed_hits(line7, active, linker)
        e = edges_of(i, j)
        e.setflags(write=False)
        _EXPECTED[name] = dict(edges=e, n_raw=int(len(i)))
    return _EXPECTED[name]


def groups_from_edges(T, edges):
    """merging.cc:557-600: union by size over the edges in std::set order, then labels in index order of the roots.
    -> labels (T,) int64; group g of the output holds the inputs with label g in ascending order"""
    parent = [-1] * T
    size = [1] * T

    def root(x):
        while parent[x] != -1:
            x = parent[x]
        return x
    for a, b in np.asarray(edges, np.int64).reshape(-1, 2).tolist():
        r1, r2 = root(a), root(b)
        if r1 == r2:
            continue
        if size[r1] < size[r2]:
            parent[r1] = r2; size[r2] += size[r1]; size[r1] = 0
        else:
            parent[r2] = r1; size[r1] += size[r2]; size[r2] = 0
    labels = [-1] * T
    n = 0
    for t in range(T):
        if parent[t] == -1:
            labels[t] = n; n += 1
    for t in range(T):
        if labels[t] == -1:
            labels[t] = labels[root(t)]
    return np.asarray(labels, np.int64)


def groups_as_lists(labels):
    out = [[] for _ in range(int(labels.max()) + 1 if len(labels) else 0)]
    for t, g in enumerate(np.asarray(labels).tolist()):
        out[g].append(t)
    return out


def _case(name, line7, active, linker=LINKER, capacity0=0, **facts):
    line7 = np.ascontiguousarray(np.asarray(line7, np.float64).reshape(-1, 7))
    active = np.ascontiguousarray(np.asarray(active, bool).reshape(-1))
    assert len(active) == len(line7)
    case = (name, line7, active, dict(linker), int(capacity0), facts)
    e = expected(case)
    facts.update(n_unique=int(len(e["edges"])), n_raw=e["n_raw"], all_active=bool(active.all()))
    if facts["all_active"]:
        # every pair is tested once: each hit is its own edge
        assert facts["n_raw"] == facts["n_unique"], name
    return case


def _segs(s, e, unc=1.0):
    s, e = np.asarray(s, np.float64).reshape(-1, 3), np.asarray(e, np.float64).reshape(-1, 3)
    return np.concatenate([s, e, np.full((len(s), 1), unc)], 1)


# ---- bundles: chains of near-collinear half-overlapping segments ----------------------------------------------------------
def bundles(T, seed, n_bundles=3):
    """T segments of length 1 in n_bundles far-apart chains: member k of a chain covers [k / 2, k / 2 + 1] of its axis
    (overlap 0.5 with its neighbours -> connected, 0 with the next but one -> not), a few 1e-3 off the axis and a few
    0.1 degrees off its direction.  A fixed permutation scatters the members over the index range."""
    rng = np.random.default_rng(seed)
    nb = 1 if T < 8 else n_bundles
    axes = np.array([[1.0, 0.2, 0.1], [0.1, 1.0, -0.3], [0.3, -0.2, 1.0]])
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    out = np.zeros((T, 7))
    perm = rng.permutation(T)
    for m in range(T):
        b, k = m % nb, m // nb
        d = axes[b] + rng.normal(0, 1e-3, 3)
        d /= np.linalg.norm(d)
        o = 50.0 * b * np.array([0.0, 0.0, 1.0]) + 0.5 * k * axes[b] + rng.normal(0, 1e-3, 3)
        out[perm[m]] = np.concatenate([o, o + d, [1.0]])
    return out


def _crossed(edges, T, step):
    """boundaries B = step, 2 step, ... < T with an edge (a, b), a < B <= b"""
    return [B for B in range(step, T, step) if ((edges[:, 0] < B) & (edges[:, 1] >= B)).any()]


TILE_T = (1, 2, 63, 64, 65, 255, 256, 257, 321)


def tile_edges(T, mixed):
    """T around the j chunk (64) and the i block (256); all active, or every third track inactive (track 0 among them:
    T = 1 is then a workgroup without an active track)"""
    line7 = bundles(T, seed=1000 + T)
    active = np.ones(T, bool)
    if mixed:
        active[np.arange(T) % 3 == 0] = False
    c = _case(f"tile_{T}_{'mixed' if mixed else 'all'}", line7, active)
    e = expected(c)["edges"]
    full = expected_edges(line7, np.ones(T, bool), LINKER)
    assert _crossed(e, T, CHUNK) == list(range(CHUNK, T, CHUNK)), c[0]
    assert _crossed(e, T, BLOCK) == list(range(BLOCK, T, BLOCK)), c[0]
    if T >= 2:
        assert len(full) >= T - 3 and len(full) < 2 * T   # chains: neighbours only
    if mixed and T >= 63:
        # edges with an inactive end exist; connected pairs of two inactive tracks are gone
        assert (~active[e[:, 0]] | ~active[e[:, 1]]).any(), c[0]
        assert not (~active[e[:, 0]] & ~active[e[:, 1]]).any() and len(e) < len(full)
    if not mixed:
        assert np.array_equal(e, full)
    return c


# ---- orientation -------------------------------------------------------------------------------------------------------
def _orientation_lines():
    """six far-apart clusters on x-parallel axes: a long segment [0, 10], two short ones inside it, and four of length 2
    that overlap its end by a: bi-overlap a / 2 just above / below th_overlap (0.1), and -- 3 degrees off, between
    th_smartangle and th_angle -- just above / below th_smartoverlap (0.3), where the smart angle threshold flips them.
    Returns (line7, cluster id, role)."""
    L, cl, role = [], [], []
    t3 = math.radians(3.0)
    for c in range(6):
        y = 20.0 * c

        def add(x0, x1, r, tilt=0.0, dz=0.0):
            ln = x1 - x0
            L.append([x0, y, dz, x0 + ln * math.cos(tilt), y + ln * math.sin(tilt), dz, 1.0]); cl.append(c); role.append(r)
        add(0.0, 10.0, "long")
        add(2.0, 3.0, "short", dz=0.01)
        add(4.0, 4.5, "short", dz=-0.01)
        add(10.0 - 0.2 * (1 + 1e-3), 12.0 - 0.2 * (1 + 1e-3), "ov+")
        add(10.0 - 0.2 * (1 - 1e-3), 12.0 - 0.2 * (1 - 1e-3), "ov-")
        add(10.0 - 0.6 * (1 + 1e-2), 12.0 - 0.6 * (1 + 1e-2), "smart+", tilt=t3)
        add(10.0 - 0.3, 12.0 - 0.3, "smart-", tilt=t3)
    return np.asarray(L), np.asarray(cl), np.asarray(role)


def _asymmetric_pairs(line7, linker):
    T = len(line7)
    i, j = np.triu_indices(T, 1)
    ab = ora.linker3d_check_pairs(linker, line7[i], line7[j])
    ba = ora.linker3d_check_pairs(linker, line7[j], line7[i])
    m = ab != ba
    return i[m], j[m], ab[m]   # ab: the lower index is the accepting l1


@functools.lru_cache(None)
def _orientation_layout():
    """the permutation and the NaN-uncertainty choice (searched over seeds on the CPU, asserted below)"""
    base, cl, role = _orientation_lines()
    T = len(base)
    i, j = np.triu_indices(T, 1)
    assert np.array_equal(ora.linker3d_check_pairs(LINKER, base[i], base[j]), ora.linker3d_check_pairs(LINKER, base[j], base[i]))
    g = expected_edges(base, np.ones(T, bool), LINKER)
    r = {(role[a], role[b]) for a, b in g.tolist()} | {(role[b], role[a]) for a, b in g.tolist()}
    # what the geometry is for: the short ones and the accepted side of either threshold connect to the long one
    assert {("long", "short"), ("long", "ov+"), ("long", "smart+")} <= r
    assert ("long", "ov-") not in r and ("long", "smart-") not in r
    for seed in range(64):
        rng = np.random.default_rng(7000 + seed)
        perm = rng.permutation(T)
        line7 = np.zeros_like(base)
        line7[perm] = base
        nan = np.zeros(T, bool)
        nan[perm[(cl % 2 == 0) & (role == "long")]] = True          # long lines of clusters 0, 2, 4
        nan[perm[(cl % 2 == 1) & (role != "long")]] = True          # every partner in clusters 1, 3, 5
        line7[nan, 6] = np.nan
        active = np.ones(T, bool)
        active[perm[cl >= 4]] = nan[perm[cl >= 4]]                   # clusters 4, 5: only the NaN (rejecting) side active
        active[perm[(cl == 3)]] = ~nan[perm[cl == 3]]                # cluster 3: only the accepting side active
        a, b, low_accepts = _asymmetric_pairs(line7, LINKER)
        combos = {(int((x + y) & 1), bool(la)) for x, y, la in zip(a, b, low_accepts)}
        rej = np.where(low_accepts, b, a)
        acc = np.where(low_accepts, a, b)
        only_rej = active[rej] & ~active[acc]
        only_acc = ~active[rej] & active[acc]
        both = active[rej] & active[acc]
        if len(a) >= 8 and len(combos) == 4 and only_rej.any() and only_acc.any() and both.any():
            return line7, active, (a, b, low_accepts)
    raise AssertionError("orientation: no layout with every parity class and side")


def orientation(mixed):
    line7, active, (a, b, low_accepts) = _orientation_layout()
    T = len(line7)
    if not mixed:
        active = np.ones(T, bool)
    c = _case(f"orientation_{'mixed' if mixed else 'all'}", line7, active, asymmetric=int(len(a)))
    e = set(map(tuple, expected(c)["edges"].tolist()))
    assert len(a) >= 8
    if not mixed:
        # the side that tests {i < j}: i when i + j is odd, j when it is even; the edge exists iff that side accepts
        seen = set()
        for x, y, la in zip(a.tolist(), b.tolist(), low_accepts.tolist()):
            odd = (x + y) & 1
            assert ((x, y) in e) == (bool(la) if odd else not la), (x, y)
            seen.add((odd, bool(la), (x, y) in e))
        assert len({s[:2] for s in seen}) == 4 and {s[2] for s in seen} == {True, False}
    else:
        rej = np.where(low_accepts, b, a); acc = np.where(low_accepts, a, b)
        n_dropped = 0
        for x, y, r_, a_ in zip(a.tolist(), b.tolist(), rej.tolist(), acc.tolist()):
            assert ((x, y) in e) == bool(active[a_]), (x, y)     # an edge iff the accepting side is an active i
            n_dropped += bool(active[r_] and not active[a_])
        assert n_dropped >= 1                                    # only the rejecting side active: no edge
        c[5]["only_rejecting_side_active"] = n_dropped
    return c


# ---- cosine guard ------------------------------------------------------------------------------------------------------
COS_TH = (0.0, 1.0, 5.0, 89.999, 90.0, 120.0)
COS_SMART = ("off", "below", "above")


def _cos_linker(th, smart):
    """overlap and inner-segment gates out of the way (th_overlap < 0 <= every overlap here, th_innerseg huge): the angle
    gates alone decide"""
    return dict(score_th=0.5, th_angle=th, th_overlap=-1.0, th_smartoverlap=0.1, th_perp=1.0, th_innerseg=1e9,
                th_smartangle={"off": 1.0, "below": th / 2 if th > 0 else -1.0, "above": th + 5.0}[smart],
                use_smartangle=smart != "off")


def _flip(th):
    """adjacent doubles (t_in, t_out): the segment (0,0,0)-(1,t,0) is within th of the x axis for the oracle at t_in and
    not at t_out -- the nearest representable directions on either side of the threshold"""
    lk = _cos_linker(th, "off")
    base = _segs([[0, 0, 0]], [[1, 0, 0]])

    def inside(t):
        return bool(ora.linker3d_check_pairs(lk, base, _segs([[0, 0, 0]], [[1, t, 0]]))[0])
    lo, hi = 0.0, 1e6
    assert inside(lo) and not inside(hi)
    a, b = int(np.float64(lo).view(np.int64)), int(np.float64(hi).view(np.int64))   # non-negative doubles order like their bits
    while b - a > 1:
        m = (a + b) // 2
        if inside(float(np.int64(m).view(np.float64))):
            a = m
        else:
            b = m
    return float(np.int64(a).view(np.float64)), float(np.int64(b).view(np.float64))


def cos_guard(th, smart):
    """every line starts near the origin; index 0 is the x axis segment, the others make with it an angle of exactly 0
    and exactly 180, th (1 +- 1e-9 / 1e-7 / 1e-5), the adjacent doubles where the oracle's own angle test flips (+- 2
    more steps), exactly 90 and one step either side; plus a parallel copy with overlap 0.05 (smart angle territory), two
    zero-length lines, and one far-away inactive track: with it every active line is tested as i and as j."""
    S, E, tag = [[0, 0, 0]], [[1, 0, 0]], ["base"]

    def add(s, e, t):
        S.append(s); E.append(e); tag.append(t)
    add([1, 0, 0], [0, 0, 0], "180")
    add([0, 0, 0], [2, 0, 0], "0")
    add([0.95, 0, 0], [1.95, 0, 0], "0 low overlap")
    for f in (1e-9, 1e-7, 1e-5):
        for sg in (-1, 1):
            a = math.radians(th * (1 + sg * f))
            add([0, 0, 0], [math.cos(a), math.sin(a), 0], f"th(1{'+' if sg > 0 else '-'}{f:g})")
    if th < 90:
        t_in, t_out = _flip(th)
        add([0, 0, 0], [1, t_in, 0], "in0")
        add([0, 0, 0], [2, 2 * t_in, 0], "in1")                    # the same direction from other operands
        add([0, 0, 0], [1, float(np.nextafter(t_in, -np.inf)), 0], "in2")
        for k in range(3):
            t = t_out
            for _ in range(k):
                t = float(np.nextafter(t, np.inf))
            add([0, 0, 0], [1, t, 0], f"out{k}")
    tiny = float(np.nextafter(0.0, 1.0))
    add([0, 0, 0], [0, 1, 0], "90")
    add([0, 0, 0], [tiny, 1, 0], "90-")
    add([0, 0, 0], [-tiny, 1, 0], "90-'")
    add([0, 0, 0], [1e-17, 1, 0], "90--")
    add([0.5, 0, 0], [0.5, 0, 0], "zero")
    add([0.25, 0.1, 0], [0.25, 0.1, 0], "zero")
    add([1e7, 1e7, 1e7], [1e7 + 1, 1e7, 1e7], "inactive")
    line7 = _segs(S, E)
    T = len(line7)
    active = np.ones(T, bool)
    active[-1] = False
    lk = _cos_linker(th, smart)
    c = _case(f"cos_{th:g}_{smart}", line7, active, lk)
    e = set(map(tuple, expected(c)["edges"].tolist()))
    idx = {t: [k for k, x in enumerate(tag) if x == t] for t in set(tag)}
    zero = idx["zero"]
    if th < 90:
        assert not any(z in p for p in e for z in zero)           # direction (0, 0, 0): 90 degrees from everything
    # accepted pairs at the threshold: within 1e-7 relative of it (th = 0: exactly 0; th >= 90: the 90 degrees no angle
    # exceeds).  Not where the smart angle threshold sits below th_angle at th >= 89.999: there the overlap of such a pair
    # is below th_smartoverlap and the reference itself turns it down.
    if th == 0:
        near = idx["0 low overlap"] if smart != "off" else idx["0"] + idx["180"]
    elif th < 90:
        near = idx["th(1-1e-09)"] + idx["th(1-1e-07)"] + idx["in0"] + idx["in1"]
    else:
        near = idx["90"] + idx["90-"]
    hit = [k for k in near if (0, k) in e]
    if not (smart == "below" and th >= 89.999):
        assert hit, c[0]
    if smart == "off" and 0 < th < 90:
        assert all((0, k) in e for k in idx["in0"] + idx["in1"] + idx["th(1-1e-09)"])
        assert not any((0, k) in e for k in idx["out0"] + idx["th(1+1e-09)"])
    c[5].update(near_accepted=len(hit), tags=tag)
    return c


# ---- the survivor queue, full ---------------------------------------------------------------------------------------------
def queue_full():
    """192 tracks with one direction bit for bit, one of them inactive: no parity rule, and every pair passes the cosine
    test, so a wave whose 64 tracks i and 64 tracks j are different ranges queues 64 x 64 = 4096 survivors, its last
    slot included (4032 where they are the same range)."""
    T = 192
    v = np.array([0.75, 0.5, 0.25])
    perm = np.random.default_rng(42).permutation(T)
    S = np.zeros((T, 3))
    for m in range(T):
        g, k = m % 4, m // 4
        S[perm[m]] = 0.5 * k * v + np.array([0.0, 0.0, 8.0 * g])   # multiples of 1/8: s + v and (s + v) - s are exact
    line7 = _segs(S, S + v)
    d = line7[:, 3:6] - line7[:, :3]
    assert (d == v).all()                                          # one difference vector -> one unit vector, bit for bit
    u = d / np.sqrt((d * d).sum(1))[:, None]
    assert len(np.unique(u.view(np.int64), axis=0)) == 1
    c0 = abs(float(u[0] @ u[0]))
    assert c0 >= math.cos(math.radians(5.0 * (1 + 1e-6) + 1e-6))   # ... which passes cos_guard against itself
    active = np.ones(T, bool)
    active[100] = False
    c = _case("queue_full", line7, active, survivors_per_wave=QUEUE)
    i, j = directed_pairs(T, active)
    assert len(i) == (T - 1) * (T - 1)
    e = expected(c)["edges"]
    n_pairs = T * (T - 1) // 2
    assert 100 < len(e) < n_pairs // 10                            # some connect (chain neighbours), most do not
    a, b = directed_hits(line7, active, LINKER)
    for bi in range(3):                                            # in every (i wave, j chunk) combination
        for bj in range(3):
            assert ((a // 64 == bi) & (b // 64 == bj)).any(), (bi, bj)
    return c


# ---- a workgroup without an active track -------------------------------------------------------------------------------
def dead_block():
    """600 tracks, active only in [256, 512): the workgroups of the first and the third 256 leave at the
    __syncthreads_or, the second works; its partners j lie in all three ranges"""
    T = 600
    line7 = bundles(T, seed=600)
    active = np.zeros(T, bool)
    active[256:512] = True
    c = _case("dead_block", line7, active)
    e = expected(c)["edges"]
    lo, hi = e[:, 0], e[:, 1]
    assert ((lo < 256) & (hi >= 256) & (hi < 512)).any() and ((lo >= 256) & (hi < 512)).any()
    assert ((lo >= 256) & (lo < 512) & (hi >= 512)).any()
    assert (active[lo] | active[hi]).all()
    full = expected_edges(line7, np.ones(T, bool), LINKER)
    assert (~active[full[:, 0]] & ~active[full[:, 1]]).any()       # connected pairs of two inactive tracks: not edges
    return c


# ---- edge counts around the first copy, and the capacity ---------------------------------------------------------------
def _family(m, origin):
    """m mutually connected tracks: one unit segment shifted by 1e-3 per member along itself"""
    k = np.arange(m, dtype=np.float64)[:, None]
    s = np.asarray(origin, np.float64)[None, :] + k * np.array([[1e-3, 0.0, 0.0]]) + (k % 3) * np.array([[0.0, 1e-4, 0.0]])
    return _segs(s, s + np.array([[1.0, 0.0, 0.0]]))


def _family_sizes(target):
    """family sizes m1 >= m2 >= ... with sum of m (m - 1) / 2 == target, largest first (greedy; asserted)"""
    out, left = [], target
    while left:
        m = int((1 + math.isqrt(1 + 8 * left)) // 2)
        assert m >= 2
        out.append(m); left -= m * (m - 1) // 2
    assert sum(m * (m - 1) // 2 for m in out) == target
    return out


COUNT_TARGETS = dict(below=435, exact_first=FIRST, exact_first_plus_one=FIRST + 1, above=8385)


def edge_count(which):
    """all-active families of mutually connected tracks (every pair tested once: n_raw == n_unique) whose edge count is
    below / exactly / one more than / well above the 4095 edges that return with the counter"""
    target = COUNT_TARGETS[which]
    line7 = np.concatenate([_family(m, [0.0, 30.0 * f, 0.0]) for f, m in enumerate(_family_sizes(target))])
    T = len(line7)
    perm = np.random.default_rng(target).permutation(T)
    line7 = line7[perm]
    c = _case(f"count_{which}", line7, np.ones(T, bool))
    assert c[5]["n_raw"] == c[5]["n_unique"] == target, (c[0], c[5])
    assert target <= max(1 << 16, 32 * T)                          # one launch at the default capacity
    return c


def capacity(which):
    """one dense family of 40 with five inactive members (pairs of two active tracks are counted from both sides), its
    first launch with room for exactly N = n_raw edges, for N - 1, and for one"""
    line7 = _family(40, [0.0, 0.0, 0.0])
    active = np.ones(40, bool)
    active[[3, 11, 17, 29, 38]] = False
    N = expected(("capacity_probe", line7, active, LINKER))["n_raw"]
    assert N == 35 * 34 + 35 * 5
    cap = {"N": N, "N-1": N - 1, "1": 1}[which]
    c = _case(f"capacity_{which}", line7, active, capacity0=cap, attempts=1 if which == "N" else 2)
    assert c[5]["n_raw"] == N and c[5]["n_unique"] == 35 * 34 // 2 + 35 * 5
    return c


BUILDERS = ([functools.partial(tile_edges, T, mx) for T in TILE_T for mx in (False, True)]
            + [functools.partial(orientation, mx) for mx in (False, True)]
            + [functools.partial(cos_guard, th, sm) for th in COS_TH for sm in COS_SMART]
            + [queue_full, dead_block]
            + [functools.partial(edge_count, w) for w in COUNT_TARGETS]
            + [functools.partial(capacity, w) for w in ("N", "N-1", "1")])


@functools.lru_cache(None)
def all_cases():
    cases = [b() for b in BUILDERS]
    assert len({c[0] for c in cases}) == len(cases)
    return cases


def case_by_name(name):
    return next(c for c in all_cases() if c[0] == name)
