"""limap.line2d matching on the GPU: the two descriptor matchers that are pure linear algebra -- ``L2D2Matcher``
(line2d/L2D2/matcher.py: top-k and mutual nearest neighbour) and the top-k form of ``NNEndpointsMatcher``
(line2d/endpoints/matcher.py:71-111) -- and SOLD2's ``WunschLineMatcher`` (line2d/SOLD2/model/line_matching.py: line
scores pooled from the point scores of the sampled descriptors, top-k, and the mutual Needleman-Wunsch form) as
``SOLD2Matcher``, and the dense-warp matcher behind ``dense_roma`` (line2d/dense/matcher.py: everything behind
``get_warping_symmetric``) as ``DenseLineMatcher`` / ``RoMaLineMatcher``, with the reference's method names, plus one
batched entry point for a scene:

    from limap_amd import matching
    matches = matching.match_scene(descinfos, neighbors, kind="l2d2", topk=10)   # img_id -> {ng_img_id: (n, 2) int32}
    matches = matching.match_scene(descinfos, neighbors, kind="sold2", topk=0)   # descinfo = [desc (dim, 5 N), valid (N, 5)]
    matches = matching.match_scene_dense(descinfos, neighbors, warps, sample_thresh=0.05)   # descinfo of DenseNaiveExtractor
    for img_id in image_ids:
        triangulator.TriangulateImage(img_id, matches[img_id])

``warps`` is a ``BaseDenseMatcher``, a callable ``(i, j) -> (warp_12, cert_12, warp_21, cert_21)`` or a dict of those:
RoMa's output, an optical flow, a depth-plus-pose warp, a homography.  The dense kind needs no descriptors: the samples
of every line go through the warp and are measured against every line of the other image (lt_kernels_dense.hip).

Scores are FP32 fmaf chains computed by the FP32-input MFMA, the top-k of every line is selected on chip
(lt_kernels_match.hip, lt_kernels_wunsch.hip); equal scores rank by ascending neighbour line.
The ``topk == 0`` form of the endpoints matcher (Sinkhorn), SuperGlue, LBD and GlueStick matchers are out of scope, and
so is everything of SOLD2 in front of the stored descinfo (network, detector, the sampling of the dense descriptor map).
Of the dense kind RoMa itself (``RoMaLineMatcher`` builds it from ``romatch`` where that is installed) and the image read
of ``DenseNaiveExtractor.extract`` beyond ``camview.read_image()`` are out of scope.
"""
import ctypes as C
import os
from typing import NamedTuple

import numpy as np

from . import _capi, _native
from . import io as limapio

__all__ = ["BaseMatcherOptions", "DefaultMatcherOptions", "BaseMatcher", "L2D2Matcher", "NNEndpointsMatcher",
           "SOLD2Matcher", "wunsch_scores_host", "wunsch_nw_host", "match_scene", "match_pair_host", "timers",
           "kernel_ms", "MAX_TOPK", "MAX_DIM", "KINDS", "BaseDenseLineMatcherOptions", "DefaultDenseLineMatcherOptions",
           "BaseDenseMatcher", "DenseNaiveExtractor", "DenseLineMatcher", "RoMaLineMatcher", "match_scene_dense",
           "match_dense_pair_host", "match_dense_dists_host", "dense_kernel_ms", "DENSE_MAX_SAMPLES",
           "DENSE_WARP_BYTES"]

MAX_TOPK = 64   # LT_MATCH_MAX_TOPK
MAX_DIM = 256   # LT_MATCH_MAX_DIM
KINDS = {"l2d2": 0, "endpoints": 1, "nn_endpoints": 1, "sold2": 2, "dense": 3, "dense_roma": 3}
SOLD2 = 2       # descinfo = [desc (dim, S N), valid (N, S)]: lt_match_wunsch_scene
DENSE = 3       # descinfo of DenseNaiveExtractor and a warp per pair: lt_match_dense_pairs (match_scene_dense)
DENSE_MAX_SAMPLES = 64          # kDenseMaxSamples: a line's good flags are one 64-bit word
DENSE_WARP_BYTES = 512 << 20    # default budget of match_scene_dense for the warps and certainties of one native call
_KEY = {0: "line_descriptors", 1: "endpoints_desc"}

_context = _capi.per_device_contexts()


def _kind(kind):
    if isinstance(kind, str):
        if kind not in KINDS:
            raise ValueError(f"matching: unknown kind {kind!r}")
        return KINDS[kind]
    if int(kind) not in (0, 1, 2, 3):
        raise ValueError(f"matching: unknown kind {kind!r}")
    return int(kind)


def _rows(d, rule, empty, transpose):
    """a descriptor array as contiguous float32 rows, NumPy or a torch GPU tensor where the input is one: 2-D (`rule`
    is the refusal's text; without elements it takes the shape `empty`), transposed where the rows are its columns.
    The device rule waits for the call's device (_gather)"""
    d = _native.operand(d, host=False, device=None, who="matching", what="a descriptor array").astype("float32")
    if d.ndim != 2:
        if all(d.shape):
            raise ValueError(f"matching: {rule}, got shape {d.shape}")
        d = d.map(lambda k: k.reshape(empty))
    return (d.map(lambda k: k.T) if transpose else d).contiguous().keep


def _rows_of(descinfo, kind):
    """the descriptor rows of one image, (rows, dim).  Endpoints: limap keeps (dim, 2 M); the native layout is one row
    per endpoint."""
    d = descinfo[_KEY[kind]] if isinstance(descinfo, dict) else descinfo
    return _rows(d, "descriptors must be 2-D", (0, 0), kind == 1)


def _width(parts):
    dims = {int(p.shape[1]) for p in parts if p.shape[0] > 0}
    if len(dims) > 1:
        raise ValueError(f"matching: descriptor widths differ across the call: {sorted(dims)}")
    return dims.pop() if dims else 8


def _sold2_parts(descinfo, num_samples):
    """the point-descriptor rows (S N, dim) float32 (NumPy, or torch where the input is) and valid (N, S) uint8 of one
    image from its descinfo [desc (dim, S N), valid (N, S)] -- list, tuple or the object array SOLD2Detector.save_descinfo
    writes (valid with a leading axis of one); an empty descinfo is an image without lines"""
    S = int(num_samples)
    if descinfo is None or len(descinfo) == 0:
        return np.zeros((0, 8), np.float32), np.zeros((0, S), np.uint8)
    if isinstance(descinfo, dict) or len(descinfo) != 2:
        raise ValueError("matching: a sold2 descinfo is the pair [desc (dim, S N), valid (N, S)]")
    d, v = descinfo[0], _native.to_host(descinfo[1])
    if v.ndim == 3 and v.shape[0] == 1:
        v = v[0]
    if v.size == 0:
        v = v.reshape(0, S)
    if v.ndim != 2 or v.shape[1] != S:
        raise ValueError(f"matching: valid must be (N, num_samples = {S}), got shape {v.shape}")
    v = np.ascontiguousarray(v != 0, np.uint8)
    rows = _rows(d, "desc must be 2-D (dim, S N)", (8, 0), True)
    if rows.shape[0] != S * v.shape[0]:
        raise ValueError(f"matching: desc has {rows.shape[0]} columns, valid {v.shape[0]} rows: not num_samples = {S} "
                         "columns per line")
    return rows, v


def _gather(parts, dim, device):
    """one array for the native call from the per-image rows: (keep-alive, pointer, on_device).  On the device where
    every image with rows brought a GPU tensor (an image without rows does not decide), else all on the host"""
    live = [_native.operand(p, host=False, device=device, who="matching", what="a descriptor array") for p in parts]
    live = [p for p in live if p.shape[0] > 0]
    if live and all(p.on_device for p in live):
        import torch
        keep = torch.cat([p.keep for p in live], 0).contiguous()
        return keep, C.c_void_p(_native.address(keep)), 1
    live = [_native.to_host(p.keep).reshape(-1, dim) for p in live]
    keep = np.ascontiguousarray(np.concatenate(live, 0), np.float32) if live else np.zeros((1, dim), np.float32)
    return keep, C.c_void_p(keep.ctypes.data), 0


def _wunsch_cfg(topk, num_samples, top_k_candidates, on_dev=0, want_scores=0):
    return _capi.LtMatchWunschConfig(int(topk), int(num_samples), int(top_k_candidates), on_dev, want_scores, 0)


def _rows_of_last_call(ctx, n_pairs, n, want_scores):
    """lt_match_get and, when asked for, lt_match_get_scores of a native call that left n rows: row_off, rows, scores"""
    row_off = np.zeros(n_pairs + 1, np.int64)
    rows = np.zeros((n, 2), np.int32)
    ctx.chk(ctx.L.lt_match_get(ctx.h, _capi.ptr(row_off, C.c_int64), _capi.ptr(rows, C.c_int32) if n else None))
    scores = None
    if want_scores:
        scores = np.zeros(n, np.float32)
        ctx.chk(ctx.L.lt_match_get_scores(ctx.h, scores.ctypes.data_as(C.POINTER(C.c_float)) if n else None))
    return row_off, rows, scores


def _match_flat(parts, pair_off, pair_nb, kind, topk, device=0, want_scores=False, valids=None, num_samples=5,
                top_k_candidates=10):
    """the native call: parts = descriptor rows per image (all NumPy or all torch); returns row_off, rows, scores.
    kind SOLD2 is lt_match_wunsch_scene: parts = point-descriptor rows per image, valids = (N, S) uint8 per image"""
    dim = _width(parts)
    desc_off = np.zeros(len(parts) + 1, np.int64)
    desc_off[1:] = np.cumsum([p.shape[0] for p in parts])
    keep, dptr, on_dev = _gather(parts, dim, device)
    ctx = _context(device)
    if on_dev:
        _native.wait_for_torch(device)
    pair_off, pair_nb = _capi.i64(pair_off), _capi.i32(pair_nb)
    pairs = (_capi.ptr(pair_off, C.c_int64), _capi.ptr(pair_nb if len(pair_nb) else _capi.i32([0]), C.c_int32))
    n_rows = C.c_int64(0)
    if kind == SOLD2:
        line_off = np.zeros(len(parts) + 1, np.int64)
        line_off[1:] = np.cumsum([v.shape[0] for v in valids])
        valid = np.ascontiguousarray(np.concatenate([v.reshape(-1) for v in valids]) if valids else np.zeros(0), np.uint8)
        if valid.size == 0:
            valid = np.zeros(1, np.uint8)
        cfg = _wunsch_cfg(topk, num_samples, top_k_candidates, on_dev, 1 if want_scores else 0)
        ctx.chk(ctx.L.lt_match_wunsch_scene(ctx.h, len(parts), _capi.ptr(line_off, C.c_int64),
                                            _capi.ptr(desc_off, C.c_int64), dptr,
                                            valid.ctypes.data_as(C.POINTER(C.c_uint8)), dim, *pairs, C.byref(cfg),
                                            C.byref(n_rows)))
    else:
        cfg = _capi.LtMatchConfig(int(kind), int(topk), on_dev, 1 if want_scores else 0)
        ctx.chk(ctx.L.lt_match_scene(ctx.h, len(parts), _capi.ptr(desc_off, C.c_int64), dptr, dim, *pairs, C.byref(cfg),
                                     C.byref(n_rows)))
    del keep
    return _rows_of_last_call(ctx, len(pair_nb), int(n_rows.value), want_scores)


def kernel_ms(device=0):
    """lt_match_wunsch_get_kernel_ms of the last sold2 call: device ms of the line-score kernel and of the NW kernel"""
    return _context(device).module_timers("lt_match_wunsch_get_kernel_ms", 2)


def _host_pair_args(descinfo1, descinfo2, num_samples):
    a, va = _sold2_parts(descinfo1, num_samples)
    b, vb = _sold2_parts(descinfo2, num_samples)
    a, b = _native.to_host(a), _native.to_host(b)
    dim = _width([a, b])
    a = np.ascontiguousarray(a.reshape(-1, dim), np.float32)
    b = np.ascontiguousarray(b.reshape(-1, dim), np.float32)
    fp, u8 = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    va = va if va.size else np.zeros((0, int(num_samples)), np.uint8)
    keep = (a, va, b, vb)
    args = (a.ctypes.data_as(fp), va.ctypes.data_as(u8), va.shape[0], b.ctypes.data_as(fp), vb.ctypes.data_as(u8),
            vb.shape[0], dim)
    return keep, args


def wunsch_scores_host(descinfo1, descinfo2, num_samples=5):
    """lt_fn_match_wunsch_scores_host: the restatement's point scores (N1, N2, S, S) and line scores (N1, N2), FP32"""
    L = _capi.load_library()
    keep, args = _host_pair_args(descinfo1, descinfo2, num_samples)
    n1, n2, S = args[2], args[5], int(num_samples)
    P, ls = np.zeros((n1, n2, S, S), np.float32), np.zeros((n1, n2), np.float32)
    fp = C.POINTER(C.c_float)
    rc = L.lt_fn_match_wunsch_scores_host(*args, S, P.ctypes.data_as(fp), ls.ctypes.data_as(fp))
    if rc != 0:
        raise ValueError(f"lt_fn_match_wunsch_scores_host: rejected (code {rc})")
    return P, ls


def wunsch_nw_host(block):
    """lt_fn_match_wunsch_nw_host: the Needleman-Wunsch values (as given, columns reversed) of one S x S FP32 block"""
    L = _capi.load_library()
    blk = np.ascontiguousarray(block, np.float32)
    if blk.ndim != 2 or blk.shape[0] != blk.shape[1]:
        raise ValueError("wunsch_nw_host: a square block expected")
    out = np.zeros(2)
    rc = L.lt_fn_match_wunsch_nw_host(blk.ctypes.data_as(C.POINTER(C.c_float)), blk.shape[0],
                                      out.ctypes.data_as(C.POINTER(C.c_double)))
    if rc != 0:
        raise ValueError(f"lt_fn_match_wunsch_nw_host: rejected (code {rc})")
    return out


def timers(device=0):
    """lt_match_get_timers of the last native call: host ms of validation + upload, kernels, download, row bookkeeping"""
    return _context(device).module_timers("lt_match_get_timers", 4)


def match_scene(descinfos, neighbors, kind="l2d2", topk=10, device=0, return_scores=False, num_samples=5,
                top_k_candidates=10):
    """Match every image of `neighbors` (img_id -> list of neighbour ids) against its neighbours in one native call.
    descinfos: img_id -> descinfo dict of the extractor (or the descriptor array itself), NumPy or torch GPU tensors.
    Returns {img_id: {ng_img_id: (n, 2) int32}} -- what ``TriangulateImage(img_id, matches)`` takes; with
    return_scores a second dict of the same shape with the FP32 score of every row.  kind "sold2": a descinfo is
    [desc (dim, num_samples N), valid (N, num_samples)]; topk == 0 is the mutual Needleman-Wunsch form over the
    top_k_candidates best lines (both keywords are used by this kind only)."""
    kind = _kind(kind)
    if kind == DENSE:
        raise ValueError("matching: the dense kind matches through a warp per pair, which match_scene does not take: "
                         "use match_scene_dense(descinfos, neighbors, warps, ...)")
    neighbors = {int(i): [int(j) for j in v] for i, v in neighbors.items()}
    ids = sorted(set(neighbors) | {j for v in neighbors.values() for j in v})
    index = {i: k for k, i in enumerate(ids)}
    valids = None
    if kind == SOLD2:
        both = [_sold2_parts(descinfos[i], num_samples) for i in ids]
        parts, valids = [b[0] for b in both], [b[1] for b in both]
    else:
        parts = [_rows_of(descinfos[i], kind) for i in ids]
    pair_off = np.zeros(len(ids) + 1, np.int64)
    pair_nb = []
    for k, i in enumerate(ids):
        pair_nb.extend(index[j] for j in neighbors.get(i, []))
        pair_off[k + 1] = len(pair_nb)
    row_off, rows, scores = _match_flat(parts, pair_off, pair_nb, kind, topk, device, return_scores, valids, num_samples,
                                        top_k_candidates)
    out, out_s = {}, {}
    for k, i in enumerate(ids):
        if i not in neighbors:
            continue
        out[i], out_s[i] = {}, {}
        for q in range(int(pair_off[k]), int(pair_off[k + 1])):
            j = ids[pair_nb[q]]
            out[i][j] = rows[row_off[q]:row_off[q + 1]]
            if return_scores:
                out_s[i][j] = scores[row_off[q]:row_off[q + 1]]
    return (out, out_s) if return_scores else out


def match_pair_host(desc1, desc2, kind="l2d2", topk=10, return_scores=False, num_samples=5, top_k_candidates=10):
    """lt_fn_match_pair_host / lt_fn_match_wunsch_pair_host: the same semantics on the host (std::fmaf in a plain loop),
    for tests; no device"""
    kind = _kind(kind)
    if kind == DENSE:
        raise ValueError("matching: the dense kind has a host entry of its own: match_dense_pair_host")
    L = _capi.load_library()
    if kind == SOLD2:
        keep, args = _host_pair_args(desc1, desc2, num_samples)
        n1, n2 = args[2], args[5]
        cap = max(1, n1 * max(1, min(max(int(topk), 1), n2)))
        rows, scores, n = np.zeros((cap, 2), np.int32), np.zeros(cap, np.float32), C.c_int64(0)
        cfg = _wunsch_cfg(topk, num_samples, top_k_candidates, 0, 1)
        rc = L.lt_fn_match_wunsch_pair_host(*args, C.byref(cfg), _capi.ptr(rows, C.c_int32),
                                            scores.ctypes.data_as(C.POINTER(C.c_float)), C.byref(n))
        if rc != 0:
            raise ValueError(f"lt_fn_match_wunsch_pair_host: rejected (code {rc})")
        rows, scores = rows[:n.value].copy(), scores[:n.value].copy()
        return (rows, scores) if return_scores else rows
    a, b = _native.to_host(_rows_of(desc1, kind)), _native.to_host(_rows_of(desc2, kind))
    dim = _width([a, b])
    a = np.ascontiguousarray(a.reshape(-1, dim), np.float32)
    b = np.ascontiguousarray(b.reshape(-1, dim), np.float32)
    per = 2 if kind == 1 else 1
    cap = max(1, (a.shape[0] // per) * max(1, min(max(int(topk), 1), b.shape[0] // per)))
    rows = np.zeros((cap, 2), np.int32)
    scores = np.zeros(cap, np.float32)
    n = C.c_int64(0)
    cfg = _capi.LtMatchConfig(kind, int(topk), 0, 1)
    fp = C.POINTER(C.c_float)
    rc = L.lt_fn_match_pair_host(a.ctypes.data_as(fp), a.shape[0], b.ctypes.data_as(fp), b.shape[0], dim, C.byref(cfg),
                                 _capi.ptr(rows, C.c_int32), scores.ctypes.data_as(fp), C.byref(n))
    if rc != 0:
        raise ValueError(f"lt_fn_match_pair_host: rejected (code {rc})")
    rows, scores = rows[:n.value].copy(), scores[:n.value].copy()
    return (rows, scores) if return_scores else rows


class BaseMatcherOptions(NamedTuple):
    """line2d/base_matcher.py:10-28 (n_jobs and weight_path are accepted and unused: one native call, no weights)"""
    topk: int = 10
    n_neighbors: int = 20
    n_jobs: int = 1
    weight_path: str = None


DefaultMatcherOptions = BaseMatcherOptions()


class BaseMatcher:
    """line2d/base_matcher.py:34-227 over the native matcher.  `extractor` only has to offer
    ``read_descinfo(descinfo_folder, idx)`` (and may be None where descinfos are passed directly)."""

    KIND = None

    def __init__(self, extractor=None, options=DefaultMatcherOptions, device=0):
        self.extractor = extractor
        self.topk = options.topk
        self.n_neighbors = options.n_neighbors
        self.n_jobs = options.n_jobs
        self.weight_path = options.weight_path
        self.device = 0 if device is None else device

    def get_module_name(self):
        raise NotImplementedError

    def match_pair(self, descinfo1, descinfo2):
        if self.topk == 0:
            return self.match_segs_with_descinfo(descinfo1, descinfo2)
        return self.match_segs_with_descinfo_topk(descinfo1, descinfo2, topk=self.topk)

    def _pair(self, descinfo1, descinfo2, topk):
        parts = [_rows_of(descinfo1, self.KIND), _rows_of(descinfo2, self.KIND)]
        _, rows, _ = _match_flat(parts, [0, 1, 1], [1], self.KIND, topk, self.device)
        return rows

    def match_segs_with_descinfo(self, descinfo1, descinfo2):
        raise NotImplementedError

    def match_segs_with_descinfo_topk(self, descinfo1, descinfo2, topk=10):
        if topk <= 0:
            raise ValueError("match_segs_with_descinfo_topk: topk must be positive")
        return self._pair(descinfo1, descinfo2, topk)

    def get_matches_folder(self, output_folder):
        return os.path.join(output_folder, f"{self.get_module_name()}_n{self.n_neighbors}_top{self.topk}")

    def read_descinfo(self, descinfo_folder, idx):
        return self.extractor.read_descinfo(descinfo_folder, idx)

    def get_match_filename(self, matches_folder, idx):
        return os.path.join(matches_folder, f"matches_{idx}.npy")

    def save_match(self, matches_folder, idx, matches):
        limapio.save_matches(matches_folder, idx, matches)

    def read_match(self, matches_folder, idx):
        return limapio.read_matches(matches_folder, idx)

    def match_scene(self, descinfos, neighbors):
        return match_scene(descinfos, neighbors, self.KIND, self.topk, self.device)

    def match_all_neighbors(self, output_folder, image_ids, neighbors, descinfo_folder, skip_exists=False):
        """one native call for all images that still need their file; returns the matches folder"""
        matches_folder = self.get_matches_folder(output_folder)
        if not skip_exists:
            _delete_folder(matches_folder)
        os.makedirs(matches_folder, exist_ok=True)
        todo = {int(i): [int(j) for j in neighbors[i]] for i in image_ids
                if not (skip_exists and os.path.exists(self.get_match_filename(matches_folder, i)))}
        if not todo:
            return matches_folder
        need = sorted(set(todo) | {j for v in todo.values() for j in v})
        descinfos = {i: self.read_descinfo(descinfo_folder, i) for i in need}
        for img_id, m in self.match_scene(descinfos, todo).items():
            self.save_match(matches_folder, img_id, m)
        return matches_folder

    def match_all_exhaustive_pairs(self, output_folder, image_ids, descinfo_folder, skip_exists=False):
        ids = [int(i) for i in image_ids]
        return self.match_all_neighbors(output_folder, ids, {i: [j for j in ids if j != i] for i in ids},
                                        descinfo_folder, skip_exists)


def _delete_folder(folder):
    import shutil
    if os.path.exists(folder):
        shutil.rmtree(folder)


class L2D2Matcher(BaseMatcher):
    """line2d/L2D2/matcher.py: descinfo["line_descriptors"] (M, 128)"""
    KIND = 0

    def get_module_name(self):
        return "l2d2"

    def check_compatibility(self, extractor):
        return extractor.get_module_name() == "l2d2"

    def match_segs_with_descinfo(self, descinfo1, descinfo2):
        return self._pair(descinfo1, descinfo2, 0)


class NNEndpointsMatcher(BaseMatcher):
    """line2d/endpoints/matcher.py:12-111, top-k form: descinfo["endpoints_desc"] (256, 2 M)"""
    KIND = 1

    def get_module_name(self):
        return "nn_endpoints"

    def match_segs_with_descinfo(self, descinfo1, descinfo2):
        raise NotImplementedError("NNEndpointsMatcher with topk == 0 (Sinkhorn through SuperGlue's weights) is out of scope")


class SOLD2Matcher(BaseMatcher):
    """line2d/SOLD2/sold2.py:101-116 over WunschLineMatcher (model/line_matching.py): descinfo = [desc (dim, S N),
    valid (N, S)].  topk > 0: the best lines by the pooled line score; topk == 0: the mutual Needleman-Wunsch form.
    What is not built raises: cross_check=False and the "d2_net" / "asl_feat" samplings (both live in front of the
    descinfo, with compute_descriptors, get_pairwise_distance, the detector and the network)."""
    KIND = SOLD2

    def __init__(self, extractor=None, options=DefaultMatcherOptions, device=0, num_samples=5, top_k_candidates=10,
                 cross_check=True, sampling="regular"):
        super().__init__(extractor, options, device)
        if not cross_check:
            raise NotImplementedError("SOLD2Matcher: cross_check=False is not built (limap's matcher always has it on)")
        if sampling != "regular":
            if sampling in ("d2_net", "asl_feat"):
                raise NotImplementedError(f"SOLD2Matcher: the {sampling!r} sampling is not built")
            raise ValueError("Wrong sampling mode: " + str(sampling))
        self.num_samples = int(num_samples)
        self.top_k_candidates = int(top_k_candidates)

    def get_module_name(self):
        return "sold2"

    def check_compatibility(self, extractor):
        return extractor.get_module_name() == "sold2"

    def _pair(self, descinfo1, descinfo2, topk):
        both = [_sold2_parts(descinfo1, self.num_samples), _sold2_parts(descinfo2, self.num_samples)]
        _, rows, _ = _match_flat([b[0] for b in both], [0, 1, 1], [1], SOLD2, topk, self.device, False,
                                 [b[1] for b in both], self.num_samples, self.top_k_candidates)
        return rows

    def match_segs_with_descinfo(self, descinfo1, descinfo2):
        return self._pair(descinfo1, descinfo2, 0)

    def match_scene(self, descinfos, neighbors):
        return match_scene(descinfos, neighbors, self.KIND, self.topk, self.device, num_samples=self.num_samples,
                           top_k_candidates=self.top_k_candidates)

    def compute_descriptors(self, *args, **kwargs):
        raise NotImplementedError("SOLD2Matcher: compute_descriptors (the grid sample of the dense map) is not built")

    def get_pairwise_distance(self, *args, **kwargs):
        raise NotImplementedError("SOLD2Matcher: get_pairwise_distance is not built")


# ---------------------------------------------------------------------------------------------------------------------
# the dense kind (line2d/dense): DESIGN.md section 17, "Dense"
class BaseDenseLineMatcherOptions(NamedTuple):
    """line2d/dense/matcher.py:11-16 (device is accepted and unused: the matcher runs on its own `device` argument)"""
    n_samples: int = 21
    segment_percentage_th: float = 0.2
    device: str = "cuda"
    pixel_th: float = 10.0
    one_to_many: bool = False


DefaultDenseLineMatcherOptions = BaseDenseLineMatcherOptions()


def _stack_xy(x, y):
    if _native.is_torch(x):
        import torch
        return torch.stack([x, y], -1)
    return np.stack([x, y], axis=-1)


class BaseDenseMatcher:
    """line2d/dense/dense_matcher/base.py: what a dense matcher offers the line matcher.  The helpers take NumPy arrays
    or torch tensors."""

    def __init__(self):
        pass

    def to_normalized_coordinates(self, coords, h, w):
        """coords: (..., 2) in the order x, y"""
        return _stack_xy(2 / w * coords[..., 0] - 1, 2 / h * coords[..., 1] - 1)

    def to_unnormalized_coordinates(self, coords, h, w):
        """inverse of to_normalized_coordinates"""
        return _stack_xy((coords[..., 0] + 1) * w / 2, (coords[..., 1] + 1) * h / 2)

    def get_sample_thresh(self):
        raise NotImplementedError

    def get_warping_symmetric(self, img1, img2):
        """-> warp_1to2 ([-1, 1], (H, W, 2)), cert_1to2 (H, W), warp_2to1, cert_2to1"""
        raise NotImplementedError


class DenseNaiveExtractor:
    """line2d/dense/extractor.py: the descinfo of the dense matchers is the image, its shape, the lines (N, 2, 2) and
    their scores.  The image comes from ``camview.read_image()``; nothing else of the reading is built here."""

    def __init__(self, options=None, device=None):
        self.options = options

    def get_module_name(self):
        return "dense_naive"

    def get_descinfo_fname(self, descinfo_folder, img_id):
        return os.path.join(descinfo_folder, f"descinfo_{img_id}.npz")

    def save_descinfo(self, descinfo_folder, img_id, descinfo):
        os.makedirs(descinfo_folder, exist_ok=True)
        np.savez(self.get_descinfo_fname(descinfo_folder, img_id), **{k: np.asarray(v) for k, v in descinfo.items()})

    def read_descinfo(self, descinfo_folder, img_id):
        with np.load(self.get_descinfo_fname(descinfo_folder, img_id), allow_pickle=False) as z:
            return {k: z[k] for k in z.files}

    def extract(self, camview, segs):
        img = camview.read_image()
        segs = np.asarray(segs)
        lines = segs[:, :4].reshape(-1, 2, 2)
        scores = segs[:, -1] * np.sqrt(np.linalg.norm(segs[:, :2] - segs[:, 2:4], axis=1))
        return {"image": img, "image_shape": img.shape, "lines": lines, "scores": scores}


def _dense_image(descinfo):
    """lines (N, 4) float32 and (h, w) of a dense descinfo"""
    lines = _native.to_host(descinfo["lines"])
    if lines.size == 0:
        lines = np.zeros((0, 4), np.float32)
    if lines.shape[1:] not in ((2, 2), (4,)):
        raise ValueError(f"matching: dense lines must be (N, 2, 2), got shape {lines.shape}")
    shape = descinfo["image_shape"]
    return np.ascontiguousarray(lines.reshape(-1, 4), np.float32), (int(shape[0]), int(shape[1]))


def _dense_maps(quad, device):
    """(warp_12, cert_12, warp_21, cert_21) -> the four arrays as float32, contiguous; all torch GPU tensors or all NumPy"""
    if len(quad) != 4:
        raise ValueError("matching: a pair's warps are (warp_12, cert_12, warp_21, cert_21)")
    out = [_native.operand(a, host=False, device=device, who="matching", what="a warp") for a in quad]
    if not all(a.on_device for a in out):
        out = [_native.operand(a, host=True, device=device, who="matching", what="a warp") for a in quad]
    out = [a.astype("float32").contiguous() for a in out]
    for w, c in ((out[0], out[1]), (out[2], out[3])):
        if w.ndim != 3 or w.shape[2] != 2 or c.ndim != 2:
            raise ValueError(f"matching: a warp must be (H, W, 2) and its certainty (H, W), got {w.shape} and {c.shape}")
    return [a.keep for a in out]


def _dense_dims(maps):
    w12, c12, w21, c21 = maps
    return [w12.shape[0], w12.shape[1], c12.shape[0], c12.shape[1], w21.shape[0], w21.shape[1], c21.shape[0], c21.shape[1]]


def _dense_cfg(opts, sample_thresh, on_dev=0, want_scores=0, want_dirs=0):
    return _capi.LtMatchDenseConfig(int(opts.n_samples), 1 if opts.one_to_many else 0, float(opts.segment_percentage_th),
                                    float(opts.pixel_th), float(sample_thresh), on_dev, want_scores, want_dirs)


def _match_dense_flat(images, pairs, maps, opts, sample_thresh, device=0, want_scores=False, want_dirs=False):
    """lt_match_dense_pairs: images = [(lines (N, 4), (h, w))], pairs = [(a, b)] into them, maps = per pair the four
    arrays of _dense_maps.  Returns row_off, rows, scores, dirs (the five matrices per pair, or None)."""
    ctx = _context(device)
    line_off = np.zeros(len(images) + 1, np.int64)
    line_off[1:] = np.cumsum([im[0].shape[0] for im in images])
    lines = np.ascontiguousarray(np.concatenate([im[0] for im in images], 0) if images else np.zeros((0, 4)), np.float32)
    if lines.shape[0] == 0:
        lines = np.zeros((1, 4), np.float32)
    shapes = _capi.i32(np.array([im[1] for im in images], np.int64).reshape(-1))
    on_dev = bool(maps) and all([_native.check_device(a, host=False, device=device, who="matching", what="a warp")
                                 for q in maps for a in q])
    if not on_dev:
        maps = [[_native.to_host(a) for a in q] for q in maps]
    n = len(pairs)
    warp_p, cert_p = (C.c_void_p * max(2 * n, 1))(), (C.c_void_p * max(2 * n, 1))()
    dims = np.zeros(max(8 * n, 1), np.int32)
    for q, m in enumerate(maps):
        warp_p[2 * q], cert_p[2 * q], warp_p[2 * q + 1], cert_p[2 * q + 1] = (_native.address(a) for a in m)
        dims[8 * q:8 * q + 8] = _dense_dims(m)
    pair_img = _capi.i32(np.array(pairs, np.int64).reshape(-1)) if n else _capi.i32([0])
    if on_dev:
        _native.wait_for_torch(device)
    cfg = _dense_cfg(opts, sample_thresh, 1 if on_dev else 0, 1 if want_scores else 0, 1 if want_dirs else 0)
    n_rows = C.c_int64(0)
    ctx.chk(ctx.L.lt_match_dense_pairs(ctx.h, len(images), _capi.ptr(line_off, C.c_int64),
                                       lines.ctypes.data_as(C.POINTER(C.c_float)),
                                       _capi.ptr(shapes if len(shapes) else _capi.i32([1, 1]), C.c_int32), n,
                                       _capi.ptr(pair_img, C.c_int32), warp_p, cert_p, _capi.ptr(dims, C.c_int32),
                                       C.byref(cfg), C.byref(n_rows)))
    del maps
    row_off, rows, scores = _rows_of_last_call(ctx, n, int(n_rows.value), want_scores)
    dirs = None
    if want_dirs:
        sizes = [images[a][0].shape[0] * images[b][0].shape[0] for a, b in pairs]
        flat = np.zeros((5, max(sum(sizes), 1)), np.float32)
        fp = C.POINTER(C.c_float)
        ctx.chk(ctx.L.lt_match_dense_get_dirs(ctx.h, *(flat[k].ctypes.data_as(fp) for k in range(5))))
        dirs, e = [], 0
        for (a, b), sz in zip(pairs, sizes):
            n1, n2 = images[a][0].shape[0], images[b][0].shape[0]
            d12, o12, d21, o21, dd = (flat[k, e:e + sz].reshape(n1, n2) for k in range(5))
            dirs.append((d12.copy(), o12.copy(), d21.T.copy(), o21.T.copy(), dd.copy()))
            e += sz
    return row_off, rows, scores, dirs


def dense_kernel_ms(device=0):
    """lt_match_dense_get_kernel_ms of the last dense call: device ms of k_dense_warp, k_dense_pairs, k_dense_select"""
    return _context(device).module_timers("lt_match_dense_get_kernel_ms", 3)


def _dense_host_args(descinfo1, descinfo2, warps, dense_options, sample_thresh):
    l1, s1 = _dense_image(descinfo1)
    l2, s2 = _dense_image(descinfo2)
    m = [np.ascontiguousarray(_native.to_host(a), np.float32) for a in warps]
    if len(m) != 4 or m[0].ndim != 3 or m[0].shape[2] != 2 or m[2].ndim != 3 or m[2].shape[2] != 2 or m[1].ndim != 2 \
            or m[3].ndim != 2:
        raise ValueError("matching: a pair's warps are (warp_12 (H, W, 2), cert_12 (H, W), warp_21, cert_21)")
    d = _dense_dims(m)
    sh1, sh2, d12, d21 = _capi.i32(s1), _capi.i32(s2), _capi.i32(d[:4]), _capi.i32(d[4:])
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    cfg = _dense_cfg(dense_options, sample_thresh)
    keep = (l1, l2, m, sh1, sh2, d12, d21, cfg)
    f = lambda a: a.ctypes.data_as(fp)
    args = (f(l1), l1.shape[0], sh1.ctypes.data_as(ip), f(l2), l2.shape[0], sh2.ctypes.data_as(ip), f(m[0]), f(m[1]),
            d12.ctypes.data_as(ip), f(m[2]), f(m[3]), d21.ctypes.data_as(ip), C.byref(cfg))
    return keep, args, l1.shape[0], l2.shape[0]


def match_dense_pair_host(descinfo1, descinfo2, warps, dense_options=DefaultDenseLineMatcherOptions, sample_thresh=0.05,
                          return_scores=False):
    """lt_fn_match_dense_pair_host: the dense kind's semantics on the host (plain loops with std::fmaf), for tests; no
    device.  warps = (warp_12, cert_12, warp_21, cert_21)"""
    L = _capi.load_library()
    keep, args, n1, n2 = _dense_host_args(descinfo1, descinfo2, warps, dense_options, sample_thresh)
    cap = max(1, n1 * n2)
    rows, scores, n = np.zeros((cap, 2), np.int32), np.zeros(cap, np.float32), C.c_int64(0)
    rc = L.lt_fn_match_dense_pair_host(*args, _capi.ptr(rows, C.c_int32), scores.ctypes.data_as(C.POINTER(C.c_float)),
                                       C.byref(n))
    if rc != 0:
        raise ValueError(f"lt_fn_match_dense_pair_host: rejected (code {rc})")
    rows, scores = rows[:n.value].copy(), scores[:n.value].copy()
    return (rows, scores) if return_scores else rows


def match_dense_dists_host(descinfo1, descinfo2, warps, dense_options=DefaultDenseLineMatcherOptions, sample_thresh=0.05):
    """lt_fn_match_dense_dists_host: d_12, overlap_12 (N1, N2), d_21, overlap_21 (N2, N1) as upstream's
    compute_distance_one_direction returns them, and the combined dists (N1, N2)"""
    L = _capi.load_library()
    keep, args, n1, n2 = _dense_host_args(descinfo1, descinfo2, warps, dense_options, sample_thresh)
    out = [np.zeros(s, np.float32) for s in ((n1, n2), (n1, n2), (n2, n1), (n2, n1), (n1, n2))]
    fp = C.POINTER(C.c_float)
    rc = L.lt_fn_match_dense_dists_host(*args, *(a.ctypes.data_as(fp) for a in out))
    if rc != 0:
        raise ValueError(f"lt_fn_match_dense_dists_host: rejected (code {rc})")
    return tuple(out)


def _warps_of(warps, descinfos, i, j):
    if isinstance(warps, BaseDenseMatcher):
        return warps.get_warping_symmetric(descinfos[i]["image"], descinfos[j]["image"])
    if isinstance(warps, dict):
        w = warps[(i, j)]
        return w() if callable(w) else w
    if callable(warps):
        return warps(i, j)
    raise ValueError("matching: warps must be a BaseDenseMatcher, a callable (i, j) -> four arrays, or a dict of those")


def match_scene_dense(descinfos, neighbors, warps, dense_options=DefaultDenseLineMatcherOptions, sample_thresh=None,
                      device=0, return_scores=False, warp_bytes=DENSE_WARP_BYTES):
    """The dense kind for a scene: every image of `neighbors` (img_id -> list of neighbour ids) against its neighbours.
    descinfos: img_id -> descinfo of DenseNaiveExtractor (needs "lines" (N, 2, 2) and "image_shape"; "image" only where
    `warps` is a BaseDenseMatcher).  warps: a BaseDenseMatcher, a callable (i, j) -> (warp_12, cert_12, warp_21,
    cert_21), or a dict (i, j) -> those four (or a callable without arguments that returns them); NumPy arrays or torch
    GPU tensors, which are read in place.  sample_thresh: the certainty a sample must exceed; None asks
    warps.get_sample_thresh().  Pairs are batched into native calls whose warps and certainties stay within warp_bytes
    (a call takes at least one pair).  Returns what match_scene returns; the score of a row is its dists."""
    if sample_thresh is None:
        if not isinstance(warps, BaseDenseMatcher):
            raise ValueError("matching: sample_thresh is needed where warps is not a BaseDenseMatcher")
        sample_thresh = warps.get_sample_thresh()
    neighbors = {int(i): [int(j) for j in v] for i, v in neighbors.items()}
    ids = sorted(set(neighbors) | {j for v in neighbors.values() for j in v})
    index = {i: k for k, i in enumerate(ids)}
    images = [_dense_image(descinfos[i]) for i in ids]
    out, out_s = {i: {} for i in neighbors}, {i: {} for i in neighbors}
    todo = [(i, j) for i in sorted(neighbors) for j in neighbors[i]]

    def flush(batch, maps):
        row_off, rows, scores, _ = _match_dense_flat(images, [(index[i], index[j]) for i, j in batch], maps, dense_options,
                                                     sample_thresh, device, return_scores)
        for q, (i, j) in enumerate(batch):
            out[i][j] = rows[row_off[q]:row_off[q + 1]]
            if return_scores:
                out_s[i][j] = scores[row_off[q]:row_off[q + 1]]

    batch, maps, used, kind = [], [], 0, None
    for i, j in todo:
        m = _dense_maps(_warps_of(warps, descinfos, i, j), device)
        nbytes = 4 * sum(int(np.prod(a.shape)) for a in m)
        if batch and (used + nbytes > warp_bytes or _native.is_torch(m[0]) != kind):
            flush(batch, maps)
            batch, maps, used = [], [], 0
        kind = _native.is_torch(m[0])
        batch.append((i, j))
        maps.append(m)
        used += nbytes
    if batch:
        flush(batch, maps)
    return (out, out_s) if return_scores else out


class DenseLineMatcher(BaseMatcher):
    """line2d/dense/matcher.py:22-238 (BaseDenseLineMatcher) over the native matcher: `dense_matcher` (a
    BaseDenseMatcher) supplies the warps and the sample threshold, everything behind it runs on the device."""
    KIND = DENSE

    def __init__(self, extractor, dense_matcher, dense_options=DefaultDenseLineMatcherOptions,
                 options=DefaultMatcherOptions, device=0):
        super().__init__(extractor, options, device)
        if extractor is not None and extractor.get_module_name() != "dense_naive":
            raise ValueError("DenseLineMatcher: the extractor must be the dense_naive one")
        if dense_options.n_samples < 2:
            raise ValueError("DenseLineMatcher: n_samples must be at least 2")
        if not isinstance(dense_matcher, BaseDenseMatcher):
            raise TypeError("DenseLineMatcher: dense_matcher must be a BaseDenseMatcher")
        self.dense_options = dense_options
        self.dense_matcher = dense_matcher

    def get_module_name(self):
        return "dense"

    def check_compatibility(self, extractor):
        return extractor.get_module_name() == "dense_naive"

    def _pair(self, descinfo1, descinfo2, opts):
        maps = _dense_maps(self.dense_matcher.get_warping_symmetric(descinfo1["image"], descinfo2["image"]), self.device)
        _, rows, _, _ = _match_dense_flat([_dense_image(descinfo1), _dense_image(descinfo2)], [(0, 1)], [maps], opts,
                                          self.dense_matcher.get_sample_thresh(), self.device)
        return rows

    def match_segs_with_descinfo(self, descinfo1, descinfo2):
        return self._pair(descinfo1, descinfo2, self.dense_options)

    def match_segs_with_descinfo_topk(self, descinfo1, descinfo2, topk=10):
        """every pair under the threshold, whatever `topk` (dense/matcher.py:200-238 never reads it)"""
        return self._pair(descinfo1, descinfo2, self.dense_options._replace(one_to_many=True))

    def compute_distance_one_direction(self, descinfo1, descinfo2, warp_1to2, cert_1to2):
        """(weighted_dists, overlap), both (N1, N2) float32, of the restated definition, from the device"""
        back_w, back_c = np.zeros((1, 1, 2), np.float32), np.zeros((1, 1), np.float32)
        if _native.check_device(warp_1to2, host=False, device=self.device, who="matching", what="a warp"):
            import torch
            back_w, back_c = (torch.from_numpy(a).to(warp_1to2.device) for a in (back_w, back_c))
        maps = _dense_maps((warp_1to2, cert_1to2, back_w, back_c), self.device)
        dirs = _match_dense_flat([_dense_image(descinfo1), _dense_image(descinfo2)], [(0, 1)], [maps], self.dense_options,
                                 self.dense_matcher.get_sample_thresh(), self.device, want_dirs=True)[3]
        return dirs[0][0], dirs[0][1]

    def match_scene(self, descinfos, neighbors):
        opts = self.dense_options if self.topk == 0 else self.dense_options._replace(one_to_many=True)
        return match_scene_dense(descinfos, neighbors, self.dense_matcher, opts, None, self.device)


class RoMaLineMatcher(DenseLineMatcher):
    """line2d/dense/matcher.py:241-260.  The network is not part of this package: RoMa is built from `romatch` where
    that is installed."""

    def __init__(self, extractor, mode="outdoor", dense_options=DefaultDenseLineMatcherOptions,
                 options=DefaultMatcherOptions, device=0):
        super().__init__(extractor, self._roma(mode, dense_options.device), dense_options, options, device)

    @staticmethod
    def _roma(mode, device):
        try:
            import romatch
        except ImportError as e:
            raise ImportError("RoMaLineMatcher needs the `romatch` package (RoMa), which is not installed; pass warps "
                              "from any other source to DenseLineMatcher or match_scene_dense") from e
        return _RoMa(romatch, mode, device)

    def get_module_name(self):
        return "dense_roma"


class _RoMa(BaseDenseMatcher):
    """line2d/dense/dense_matcher/roma.py over an installed `romatch`"""

    def __init__(self, romatch, mode="outdoor", device="cuda"):
        super().__init__()
        self.output_res = 864
        self.mode = mode
        if mode == "outdoor":
            self.model = romatch.roma_outdoor(device=device, coarse_res=560, upsample_res=self.output_res)
        elif mode == "indoor":
            self.model = romatch.roma_indoor(device=device, coarse_res=560, upsample_res=self.output_res)
        elif mode == "tiny_outdoor":
            self.model = romatch.tiny_roma_v1_outdoor(device=device)
        else:
            raise ValueError(f"Unknown mode for RoMa: {mode}")

    def get_sample_thresh(self):
        return self.model.sample_thresh

    def get_warping_symmetric(self, img1, img2):
        from PIL import Image
        im1, im2 = Image.fromarray(img1), Image.fromarray(img2)
        warp, cert = self.model.match(im1, im2, batched=False)
        if self.mode.startswith("tiny"):
            back, back_cert = self.model.match(im2, im1, batched=False)
            return warp[:, :, 2:], cert, back[:, :, 2:], back_cert
        n = self.output_res
        return warp[:, :n, 2:], cert[:, :n], warp[:, n:, :2], cert[:, n:]
