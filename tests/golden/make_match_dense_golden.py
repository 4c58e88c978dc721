"""Writes tests/golden/match_dense/*.npz: dense descinfos (lines, image shapes), a warp and a certainty map in either
direction, and what limap's own BaseDenseLineMatcher makes of them -- the match rows for one_to_many False and True and
both directions' (weighted_dists, overlap) -- plus ref_time.json (the reference's wall time on the generating machine,
CPU) and two raw copies of fixtures for the sanitizer program (asan_*.bin: inputs and upstream's rows, no code).

Run on a machine that has the limap source tree (LIMAP_SRC, default /root/reference/src): line2d/dense/matcher.py and
dense_matcher/base.py are loaded from there at generation time only, with stand-ins for their parent packages, a fake
dense matcher that returns the fixture's warps, and options with device = "cpu".  Nothing of the reference is stored:
only inputs, results and times.

The analysis half of this file is imported by tests/test_match_dense_host.py.  It evaluates the definition of DESIGN
section 17, "Dense", in float64 and says which entries (i, j) are DECIDED: every comparison that feeds the entry --
sample projection against the segment's ends, certainty against the threshold, overlap against segment_percentage_th,
distances against pixel_th, the row minimum's gap -- clears its rounding bound, so any FP32 evaluation order gives the
same row.
"""
import importlib.util
import json
import os
import struct
import sys
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "match_dense")
_spec = importlib.util.spec_from_file_location("make_match_golden", os.path.join(HERE, "make_match_golden.py"))
base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(base)
U, gamma, MAX_UNDECIDED = base.U, base.gamma, base.MAX_UNDECIDED
FAR = 10000.0

# torch's CPU grid_sample does not document its order of operations, so the bound on the warped samples is measured:
# max |upstream's FP32 chain (sample, normalise, grid_sample, unnormalise) - the same chain in float64| over all
# fixtures at generation, in pixels for the coordinates and in certainty units for the certainty.  main() measures them
# again and refuses to write fixtures that exceed what is recorded here; the analysis uses FACTOR times the record.
MEASURED_COORD_PX = 1.4e-3   # (the steepest place is the zero padding at a map's border: a texel there is hundreds of pixels)
MEASURED_CERT = 4.6e-6
FACTOR = 4.0
E_COORD, E_CERT = FACTOR * MEASURED_COORD_PX, FACTOR * MEASURED_CERT


# ---------------------------------------------------------------------------------------------------------------------
# analysis
def bilinear64(img, xn, yn):
    """grid_sample(bilinear, align_corners=False, zeros) of an (H, W) or (H, W, C) map at normalised points, float64"""
    img = np.asarray(img, np.float64)
    H, W = img.shape[:2]
    ix = ((xn + 1.0) * W - 1.0) / 2.0
    iy = ((yn + 1.0) * H - 1.0) / 2.0
    x0, y0 = np.floor(ix), np.floor(iy)
    out = 0.0
    for dy in (0, 1):
        for dx in (0, 1):
            xx, yy = x0 + dx, y0 + dy
            w = (1.0 - np.abs(ix - xx)) * (1.0 - np.abs(iy - yy))
            ok = (xx >= 0) & (xx <= W - 1) & (yy >= 0) & (yy <= H - 1)
            v = img[np.clip(yy, 0, H - 1).astype(int), np.clip(xx, 0, W - 1).astype(int)]
            wk = np.where(ok, w, 0.0)
            out = out + (v * wk[..., None] if img.ndim == 3 else v * wk)
    return out


def warped64(lines, src_shape, dst_shape, warp, cert, S):
    """the S samples of every line through one direction, float64: coordinates (N, S, 2) in target pixels, certainty
    (N, S).  Sample k is r_k start + (1 - r_k) end, r = k / (S - 1)."""
    lines = np.asarray(lines, np.float32).astype(np.float64).reshape(-1, 2, 2)
    r = (np.arange(S) / (S - 1.0))[None, :, None]
    p = r * lines[:, None, 0] + (1.0 - r) * lines[:, None, 1]
    xn, yn = 2.0 / src_shape[1] * p[..., 0] - 1.0, 2.0 / src_shape[0] * p[..., 1] - 1.0
    w = bilinear64(warp, xn, yn)
    c = bilinear64(cert, xn, yn)
    xy = np.stack([(w[..., 0] + 1.0) * dst_shape[1] / 2.0, (w[..., 1] + 1.0) * dst_shape[0] / 2.0], -1)
    return xy, c


def direction_analysis(lines_src, lines_dst, src_shape, dst_shape, warp, cert, S, thresh, seg_th):
    """one direction in float64 -> d (Ns, Nd) weighted distance (FAR below seg_th), o overlap, e the bound on
    |any FP32 evaluation - d| where d is not FAR, flags_ok: every sample flag of the entry is decided, ok: the entry's
    direction is decided (flags and the overlap's comparison)"""
    xy, c = warped64(lines_src, src_shape, dst_shape, warp, cert, S)
    L = np.asarray(lines_dst, np.float32).astype(np.float64).reshape(-1, 2, 2)
    s, e = L[:, 0], L[:, 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        d = e - s
        nrm = np.linalg.norm(d, axis=1)
        d = d / nrm[:, None]
        sp, ep = (s * d).sum(1), (e * d).sum(1)
        l = np.stack([s[:, 1] - e[:, 1], e[:, 0] - s[:, 0], s[:, 0] * e[:, 1] - s[:, 1] * e[:, 0]], 1)
        cross_mag = np.abs(s[:, 0] * e[:, 1]) + np.abs(s[:, 1] * e[:, 0])
        l = l / nrm[:, None]
        px, py = xy[..., 0][:, :, None], xy[..., 1][:, :, None]            # (Ns, S, 1)
        proj = px * d[None, None, :, 0] + py * d[None, None, :, 1]         # (Ns, S, Nd)
        # bounds: the warped sample within E_COORD per coordinate; the unit direction and the line within 8 U per
        # component (a difference, two squares, a sum, a root and a quotient: under 6 roundings); the dot products
        # gamma(4) of their terms; the end projections 16 U of their terms
        mag = np.abs(px) + np.abs(py)
        e_proj = 2.0 * E_COORD + 8 * U * mag + gamma(4) * mag
        e_end_s = 16 * U * (np.abs(s).sum(1))[None, None, :]
        e_end_e = 16 * U * (np.abs(e).sum(1))[None, None, :]
        after_start, before_end = proj > sp[None, None, :], proj < ep[None, None, :]
        dec_start = np.abs(proj - sp[None, None, :]) > e_proj + e_end_s
        dec_end = np.abs(proj - ep[None, None, :]) > e_proj + e_end_e
        cert_ok = (c > thresh)[:, :, None]
        dec_cert = (np.abs(c - thresh) > E_CERT)[:, :, None]
        degenerate = ~np.isfinite(nrm) | (nrm == 0)
        good = cert_ok & after_start & before_end & ~degenerate[None, None, :]
        # a flag is decided when all three tests are, or when one of them certainly fails
        surely_off = (dec_cert & ~cert_ok) | (dec_start & ~after_start) | (dec_end & ~before_end)
        flag_dec = (dec_cert & dec_start & dec_end) | surely_off | degenerate[None, None, :]
        flags_ok = flag_dec.all(1)                                          # (Ns, Nd)
        cnt = good.sum(1)
        o = cnt / float(S)
        dist = np.abs(px * l[None, None, :, 0] + py * l[None, None, :, 1] + l[None, None, :, 2])
        e_lz = 8 * U * (cross_mag / nrm + np.abs(l[:, 2]))
        e_dist = 2.0 * E_COORD + 8 * U * mag + gamma(4) * (mag + np.abs(l[None, None, :, 2])) + e_lz[None, None, :]
        dist = np.where(good, dist, 0.0)
        e_dist = np.where(good, e_dist, 0.0)
        wd = dist.sum(1) / np.maximum(cnt, 1)
        e_wd = e_dist.sum(1) / np.maximum(cnt, 1) + gamma(S + 2) * wd
    below = o < seg_th
    dec_ovl = np.abs(o - seg_th) > 4 * U
    return np.where(below, FAR, wd), o, np.where(below, 0.0, e_wd), flags_ok, flags_ok & dec_ovl


def pair_analysis(fx, one_to_many):
    """-> match (N1, N2) bool by the float64 definition, decided (N1, N2) bool, and the per-direction results"""
    S, th, seg, pix = fx["n_samples"], fx["sample_thresh"], fx["segment_percentage_th"], fx["pixel_th"]
    l1, l2, s1, s2 = fx["lines1"], fx["lines2"], fx["shape1"], fx["shape2"]
    seg32, pix32 = float(np.float32(seg)), float(np.float32(pix))
    d12, o12, e12, f12, k12 = direction_analysis(l1, l2, s1, s2, fx["warp12"], fx["cert12"], S, th, seg32)
    d21, o21, e21, f21, k21 = direction_analysis(l2, l1, s2, s1, fx["warp21"], fx["cert21"], S, th, seg32)
    d21, o21, e21, f21, k21 = d21.T, o21.T, e21.T, f21.T, k21.T
    first = o12 > o21
    dists = np.where(first, d12, d21)
    e = np.where(first, e12, e21)
    far = (np.minimum(o12, o21) < seg32) | (np.maximum(d12, d21) > pix32)
    dists = np.where(far, FAR, dists)
    e = np.where(far, 0.0, e)
    # decided: both directions; each finite distance away from pixel_th (a FAR one is above it whatever the rounding)
    dec = k12 & k21
    both_alive = (d12 < FAR) & (d21 < FAR)
    dec &= ~both_alive | ((np.abs(d12 - pix32) > e12) & (np.abs(d21 - pix32) > e21))
    match = dists <= pix32
    if not one_to_many and dists.shape[1] > 0:
        # the row minimum: j is the minimum iff no other value is below it.  Entries of bit-identical target lines
        # (and so bit-identical values in any evaluation that treats columns alike) count as the same value.
        same = (np.asarray(l2, np.float32).reshape(-1, 4)[:, None, :] == np.asarray(l2, np.float32).reshape(-1, 4)[None]).all(2)
        lo, hi = dists - e, dists + e
        n2 = dists.shape[1]
        is_min = np.zeros_like(match)
        min_dec = np.ones_like(match)
        for i in range(dists.shape[0]):
            row_dec = dec[i].all()
            for j in range(n2):
                others = ~same[j]
                is_min[i, j] = bool((dists[i, j] <= dists[i]).all())
                if not match[i, j]:
                    continue  # above pixel_th: not a row whatever the minimum is
                surely_min = bool((hi[i, j] < lo[i, others]).all()) if others.any() else True
                surely_not = bool((hi[i, others] < lo[i, j]).any()) if others.any() else False
                min_dec[i, j] = (surely_min or surely_not) and row_dec
        match = match & is_min
        dec = dec & min_dec
    return match, dec, dict(d12=d12, o12=o12, e12=e12, f12=f12, k12=k12, d21=d21.T, o21=o21.T, e21=e21.T, f21=f21.T,
                            k21=k21.T, dists=dists, e=e)


def load_fixture(path):
    z = np.load(path, allow_pickle=False)
    fx = {k: z[k] for k in z.files}
    for k in ("n_samples",):
        fx[k] = int(fx[k])
    for k in ("sample_thresh", "segment_percentage_th", "pixel_th"):
        fx[k] = float(fx[k])
    for k in ("shape1", "shape2"):
        fx[k] = tuple(int(v) for v in fx[k])
    return fx


def rows_to_mask(rows, n1, n2):
    m = np.zeros((n1, n2), bool)
    rows = np.asarray(rows).reshape(-1, 2)
    m[rows[:, 0], rows[:, 1]] = True
    return m


# ---------------------------------------------------------------------------------------------------------------------
# generation
def _load_reference(src):
    root = os.path.join(src, "limap")
    for pkg in ("limap", "limap.line2d", "limap.line2d.dense", "limap.line2d.dense.dense_matcher"):
        m = types.ModuleType(pkg)
        m.__path__ = [os.path.join(root, *pkg.split(".")[1:])]
        sys.modules[pkg] = m
    bm = types.ModuleType("limap.line2d.base_matcher")  # stand-in for the parent class: what its __init__ keeps

    class BaseMatcher:
        def __init__(self, extractor, options):
            self.extractor, self.topk = extractor, options.topk

    class Options:
        topk = 0

    bm.BaseMatcher, bm.DefaultMatcherOptions = BaseMatcher, Options()
    sys.modules[bm.__name__] = bm
    name = "limap.line2d.dense.dense_matcher.base"
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, "line2d", "dense", "dense_matcher", "base.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    sys.modules["limap.line2d.dense.dense_matcher"].BaseDenseMatcher = mod.BaseDenseMatcher
    name = "limap.line2d.dense.matcher"
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, "line2d", "dense", "matcher.py"))
    mm = importlib.util.module_from_spec(spec)
    sys.modules[name] = mm
    spec.loader.exec_module(mm)
    return mm, mod.BaseDenseMatcher


def make_reference(src):
    import torch
    mm, Base = _load_reference(src)

    class Fake(Base):
        def __init__(self, warps, thresh):
            self.warps, self.thresh = [torch.from_numpy(np.ascontiguousarray(a)) for a in warps], thresh

        def get_sample_thresh(self):
            return self.thresh

        def get_warping_symmetric(self, img1, img2):
            return tuple(self.warps)

    class Extractor:
        def get_module_name(self):
            return "dense_naive"

    def run(fx):
        """upstream's outputs for one fixture; an image without lines on the neighbour's side makes upstream's row
        minimum fail (a reduction over an empty axis), which is recorded as no rows"""
        out = {}
        d1 = {"image": None, "image_shape": fx["shape1"], "lines": np.asarray(fx["lines1"])}
        d2 = {"image": None, "image_shape": fx["shape2"], "lines": np.asarray(fx["lines2"])}
        warps = (fx["warp12"], fx["cert12"], fx["warp21"], fx["cert21"])
        for otm in (False, True):
            opts = mm.BaseDenseLineMatcherOptions(n_samples=fx["n_samples"],
                                                  segment_percentage_th=fx["segment_percentage_th"],
                                                  pixel_th=fx["pixel_th"], one_to_many=otm)
            opts = types.SimpleNamespace(**opts._asdict(), device="cpu")
            m = mm.BaseDenseLineMatcher(Extractor(), Fake(warps, fx["sample_thresh"]), opts)
            try:
                rows = m.match_pair(d1, d2)
            except (IndexError, RuntimeError):
                assert np.asarray(fx["lines2"]).shape[0] == 0
                rows = np.zeros((0, 2), np.int64)
            out["ref_many" if otm else "ref_one"] = np.asarray(rows, np.int32).reshape(-1, 2)
        f = m.dense_matcher
        a, b = m.compute_distance_one_direction(d1, d2, f.warps[0], f.warps[1])
        c, d = m.compute_distance_one_direction(d2, d1, f.warps[2], f.warps[3])
        out.update(ref_d12=a.numpy(), ref_o12=b.numpy(), ref_d21=c.numpy(), ref_o21=d.numpy())
        return out, m

    return run


def upstream_warp_chain(lines, src_shape, dst_shape, warp, cert, S):
    """lines 52-88 of upstream's compute_distance_one_direction, op for op in FP32 on the CPU: what the measured bound
    is measured on"""
    import torch
    import torch.nn.functional as F
    segs = torch.from_numpy(np.asarray(lines)).float().reshape(-1, 2, 2)
    ratio = torch.linspace(0, 1, S)[:, None].repeat(1, 2)
    c1 = ratio * segs[:, [0]].repeat(1, S, 1) + (1 - ratio) * segs[:, [1]].repeat(1, S, 1)
    c1 = c1.reshape(-1, 2)
    h, w = src_shape[0], src_shape[1]
    coords = torch.stack([2 / w * c1[..., 0] - 1, 2 / h * c1[..., 1] - 1], axis=-1)
    wt, ct = torch.from_numpy(np.ascontiguousarray(warp)), torch.from_numpy(np.ascontiguousarray(cert))
    to2 = F.grid_sample(wt.permute(2, 0, 1)[None], coords[None, None], align_corners=False, mode="bilinear")[0, :, 0].mT
    h2, w2 = dst_shape[0], dst_shape[1]
    to2 = torch.stack([(to2[..., 0] + 1) * w2 / 2, (to2[..., 1] + 1) * h2 / 2], axis=-1)
    cc = F.grid_sample(ct[None, None], coords[None, None], align_corners=False, mode="bilinear")[0, 0, 0]
    return to2.numpy().reshape(-1, S, 2), cc.numpy().reshape(-1, S)


def measure(fx):
    worst = [0.0, 0.0]
    for a, b, sa, sb, w, c in ((fx["lines1"], fx["lines2"], fx["shape1"], fx["shape2"], fx["warp12"], fx["cert12"]),
                               (fx["lines2"], fx["lines1"], fx["shape2"], fx["shape1"], fx["warp21"], fx["cert21"])):
        if np.asarray(a).shape[0] == 0:
            continue
        xy32, c32 = upstream_warp_chain(a, sa, sb, w, c, fx["n_samples"])
        xy64, c64 = warped64(a, sa, sb, w, c, fx["n_samples"])
        worst[0] = max(worst[0], float(np.abs(xy32 - xy64).max()))
        worst[1] = max(worst[1], float(np.abs(c32 - c64).max()))
    return worst


def fixture(d1, d2, warps, S=21, thresh=0.5, seg=0.2, pix=10.0):
    return {"lines1": np.asarray(d1["lines"], np.float64), "lines2": np.asarray(d2["lines"], np.float64),
            "shape1": tuple(d1["image_shape"][:2]), "shape2": tuple(d2["image_shape"][:2]),
            "warp12": warps[0], "cert12": warps[1], "warp21": warps[2], "cert21": warps[3],
            "n_samples": S, "sample_thresh": thresh, "segment_percentage_th": seg, "pixel_th": pix}


def write_asan_bin(path, fx, ref_one):
    """a fixture as raw little-endian arrays for tools/dense_host_asan.cpp: 16 int32 (n1, n2, h1, w1, h2, w2, hw12,
    ww12, hw21, ww21, S, rows of upstream with one_to_many off, 4 zeros), 3 float32 (segment_percentage_th, pixel_th,
    sample_thresh), then lines1, lines2, warp12, cert12, warp21, cert21 as float32 and upstream's rows as int32"""
    l1, l2 = np.asarray(fx["lines1"], np.float32).reshape(-1, 4), np.asarray(fx["lines2"], np.float32).reshape(-1, 4)
    head = [l1.shape[0], l2.shape[0], *fx["shape1"], *fx["shape2"], *fx["warp12"].shape[:2], *fx["warp21"].shape[:2],
            fx["n_samples"], len(ref_one), 0, 0, 0, 0]
    with open(path, "wb") as f:
        f.write(struct.pack("<16i", *[int(v) for v in head]))
        f.write(struct.pack("<3f", fx["segment_percentage_th"], fx["pixel_th"], fx["sample_thresh"]))
        for a in (l1, l2, fx["warp12"], fx["cert12"], fx["warp21"], fx["cert21"]):
            f.write(np.ascontiguousarray(a, "<f4").tobytes())
        f.write(np.ascontiguousarray(ref_one, "<i4").tobytes())


def main():
    sys.path.insert(0, os.path.dirname(HERE))
    import dense_cases as dc
    run = make_reference(os.environ.get("LIMAP_SRC", "/root/reference/src"))
    rng = np.random.default_rng(20241019)
    os.makedirs(OUT, exist_ok=True)
    fixtures = {}
    # a homography warp at 40 x 56 texels with noisy transformed lines
    fixtures["homography_40_30"] = fixture(*dc.homography_pair(rng, 40, 30, (480, 640), (480, 640), (40, 56), (40, 56)))
    # warps whose aspect differs from the images', images of different sizes, certainty maps with holes
    fixtures["aspect_holes_33_37"] = fixture(*dc.homography_pair(rng, 33, 37, (480, 640), (360, 600), (24, 56), (48, 20),
                                                                 holes=4))
    # n_samples = 2
    fixtures["two_samples_17_16"] = fixture(*dc.homography_pair(rng, 17, 16, (480, 640), (480, 640), (32, 32), (32, 32)),
                                            S=2)
    # samples that leave the warp's [-1, 1] range: lines that reach far outside the image
    d1, d2, w = dc.homography_pair(rng, 24, 24, (480, 640), (480, 640), (40, 56), (40, 56), holes=2)
    d1["lines"][::3, 0] += rng.uniform(300, 700, (8, 2))
    d2["lines"][1::4, 1] -= rng.uniform(300, 700, (6, 2))
    fixtures["outside_24_24"] = fixture(d1, d2, w)
    # the constructed cases must be fully decided: their random parts are drawn again until the float64 analysis
    # (which knows nothing of any FP32 evaluation) finds no entry within a rounding bound of a threshold
    def decided_draw(make):
        for _ in range(200):
            fx = make()
            if all(pair_analysis(fx, otm)[1].all() for otm in (False, True)):
                return fx
        raise AssertionError("no fully decided draw")

    # a line with a zero-length partner, and a zero-length line of its own
    def zero_length():
        d1, d2, w = dc.homography_pair(rng, 12, 12, (480, 640), (480, 640), (24, 32), (24, 32))
        d2["lines"][3, 1] = d2["lines"][3, 0]
        d1["lines"][5, 1] = d1["lines"][5, 0]
        return fixture(d1, d2, w)

    # a tie of the row minimum: two identical target lines
    def tie():
        d1, d2, w = dc.homography_pair(rng, 10, 12, (480, 640), (480, 640), (24, 32), (24, 32))
        d2["lines"][10] = d2["lines"][2]
        d2["lines"][11] = d2["lines"][7]
        return fixture(d1, d2, w)

    fixtures["zero_length_12_12"] = decided_draw(zero_length)
    fixtures["tie_10_12"] = decided_draw(tie)
    # an empty image on either side
    fixtures["empty_0_9"] = fixture(*dc.homography_pair(rng, 0, 9, (480, 640), (480, 640), (8, 8), (8, 8)))
    fixtures["empty_9_0"] = fixture(*dc.homography_pair(rng, 9, 0, (480, 640), (480, 640), (8, 8), (8, 8)))
    constructed = ("zero_length_12_12", "tie_10_12", "empty_0_9", "empty_9_0")

    times = {"machine": "generator's CPU (no GPU), limap's BaseDenseLineMatcher as it is, torch on the CPU",
             "fixtures": {}}
    worst = [0.0, 0.0]
    for name, fx in fixtures.items():
        m = measure(fx)
        worst = [max(worst[0], m[0]), max(worst[1], m[1])]
    print(f"measured: coordinates {worst[0]:.3e} px, certainty {worst[1]:.3e}")
    assert worst[0] <= MEASURED_COORD_PX and worst[1] <= MEASURED_CERT, "update MEASURED_* to the values printed above"
    for name, fx in fixtures.items():
        t0 = time.perf_counter()
        ref, _ = run(fx)
        dt = time.perf_counter() - t0
        n1, n2 = fx["lines1"].shape[0], fx["lines2"].shape[0]
        shares = {}
        for otm, key in ((False, "ref_one"), (True, "ref_many")):
            match, dec, _ = pair_analysis(fx, otm)
            share = float((~dec).mean()) if dec.size else 0.0
            shares[key] = share
            assert share <= MAX_UNDECIDED, f"{name}: {share:.1%} of the entries are undecided"
            if name in constructed:
                assert share == 0.0, f"{name}: a constructed case must be fully decided ({share:.1%})"
            got = rows_to_mask(ref[key], n1, n2)
            assert np.array_equal(got[dec], match[dec]), f"{name}: upstream contradicts the float64 definition"
        arrays = dict(fx)
        arrays.update(ref)
        arrays = {k: np.asarray(v) for k, v in arrays.items()}
        np.savez_compressed(os.path.join(OUT, name + ".npz"), **arrays)
        times["fixtures"][name] = {"lines": [n1, n2], "seconds": dt, "undecided_share": shares,
                                   "rows": [int(len(ref["ref_one"])), int(len(ref["ref_many"]))]}
        print(f"{name}: {n1} x {n2}, rows {len(ref['ref_one'])} / {len(ref['ref_many'])}, undecided {shares}, "
              f"reference {dt * 1e3:.1f} ms")
        if name in ("aspect_holes_33_37", "zero_length_12_12"):
            write_asan_bin(os.path.join(OUT, f"asan_{name}.bin"), fx, ref["ref_one"])

    # the headline shape, timed only: one pair of 500 x 500 lines, S = 21, warps 864 x 864 (RoMa's output_res)
    d1, d2, w = dc.homography_pair(rng, 500, 500, (480, 640), (480, 640), (864, 864), (864, 864))
    fx = fixture(d1, d2, w)
    reps, t0 = 3, time.perf_counter()
    for _ in range(reps):
        run(fx)
    times["pair_500_500_S21_warp864"] = {
        "seconds_per_pair": (time.perf_counter() - t0) / reps,
        "note": "CPU. Both one_to_many forms and the two directions once more: about three times the work of one "
                "match_pair; matching only, no network, no files"}
    times["measured_bound"] = {"coordinates_px": worst[0], "certainty": worst[1], "factor": FACTOR}
    with open(os.path.join(OUT, "ref_time.json"), "w") as f:
        json.dump(times, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
