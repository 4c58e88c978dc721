"""limap.line2d matching on the GPU: the two descriptor matchers that are pure linear algebra -- ``L2D2Matcher``
(line2d/L2D2/matcher.py: top-k and mutual nearest neighbour) and the top-k form of ``NNEndpointsMatcher``
(line2d/endpoints/matcher.py:71-111) -- and SOLD2's ``WunschLineMatcher`` (line2d/SOLD2/model/line_matching.py: line
scores pooled from the point scores of the sampled descriptors, top-k, and the mutual Needleman-Wunsch form) as
``SOLD2Matcher``, with the reference's method names, plus one batched entry point for a scene:

    from limap_amd import matching
    matches = matching.match_scene(descinfos, neighbors, kind="l2d2", topk=10)   # img_id -> {ng_img_id: (n, 2) int32}
    matches = matching.match_scene(descinfos, neighbors, kind="sold2", topk=0)   # descinfo = [desc (dim, 5 N), valid (N, 5)]
    for img_id in image_ids:
        triangulator.TriangulateImage(img_id, matches[img_id])

Scores are FP32 fmaf chains computed by the FP32-input MFMA, the top-k of every line is selected on chip
(lt_kernels_match.hip, lt_kernels_wunsch.hip); equal scores rank by ascending neighbour line.
The ``topk == 0`` form of the endpoints matcher (Sinkhorn), SuperGlue, LBD and GlueStick matchers are out of scope, and
so is everything of SOLD2 in front of the stored descinfo (network, detector, the sampling of the dense descriptor map).
"""
import ctypes as C
import os
from typing import NamedTuple

import numpy as np

from . import _capi
from . import io as limapio

__all__ = ["BaseMatcherOptions", "DefaultMatcherOptions", "BaseMatcher", "L2D2Matcher", "NNEndpointsMatcher",
           "SOLD2Matcher", "wunsch_scores_host", "wunsch_nw_host", "match_scene", "match_pair_host", "timers",
           "kernel_ms", "MAX_TOPK", "MAX_DIM", "KINDS"]

MAX_TOPK = 64   # LT_MATCH_MAX_TOPK
MAX_DIM = 256   # LT_MATCH_MAX_DIM
KINDS = {"l2d2": 0, "endpoints": 1, "nn_endpoints": 1, "sold2": 2}
SOLD2 = 2       # descinfo = [desc (dim, S N), valid (N, S)]: lt_match_wunsch_scene
_KEY = {0: "line_descriptors", 1: "endpoints_desc"}

_context = _capi.per_device_contexts()


def _kind(kind):
    if isinstance(kind, str):
        if kind not in KINDS:
            raise ValueError(f"matching: unknown kind {kind!r}")
        return KINDS[kind]
    if int(kind) not in (0, 1, 2):
        raise ValueError(f"matching: unknown kind {kind!r}")
    return int(kind)


def _is_torch(a):
    return type(a).__module__.split(".")[0] == "torch"


def _rows_of(descinfo, kind):
    """the descriptor rows of one image, (rows, dim) float32: NumPy array, or torch tensor where the input is one.
    Endpoints: limap keeps (dim, 2 M); the native layout is one row per endpoint."""
    d = descinfo[_KEY[kind]] if isinstance(descinfo, dict) else descinfo
    if _is_torch(d):
        import torch
        d = d.to(torch.float32)
        if d.dim() != 2:
            d = d.reshape(0, 0) if d.numel() == 0 else d
        if d.dim() != 2:
            raise ValueError(f"matching: descriptors must be 2-D, got shape {tuple(d.shape)}")
        return (d.t() if kind == 1 else d).contiguous()
    a = np.asarray(d, np.float32)
    if a.ndim != 2:
        if a.size:
            raise ValueError(f"matching: descriptors must be 2-D, got shape {a.shape}")
        a = a.reshape(0, 0)
    return np.ascontiguousarray(a.T if kind == 1 else a)


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
    d, v = descinfo[0], descinfo[1]
    if _is_torch(v):
        v = v.cpu().numpy()
    v = np.asarray(v)
    if v.ndim == 3 and v.shape[0] == 1:
        v = v[0]
    if v.size == 0:
        v = v.reshape(0, S)
    if v.ndim != 2 or v.shape[1] != S:
        raise ValueError(f"matching: valid must be (N, num_samples = {S}), got shape {v.shape}")
    v = np.ascontiguousarray(v != 0, np.uint8)
    if _is_torch(d):
        import torch
        d = d.to(torch.float32)
        if d.dim() != 2:
            raise ValueError(f"matching: desc must be 2-D (dim, S N), got shape {tuple(d.shape)}")
        rows = d.t().contiguous()
    else:
        d = np.asarray(d, np.float32)
        if d.ndim != 2:
            if d.size:
                raise ValueError(f"matching: desc must be 2-D (dim, S N), got shape {d.shape}")
            d = d.reshape(8, 0)
        rows = np.ascontiguousarray(d.T)
    if rows.shape[0] != S * v.shape[0]:
        raise ValueError(f"matching: desc has {rows.shape[0]} columns, valid {v.shape[0]} rows: not num_samples = {S} "
                         "columns per line")
    return rows, v


def _gather(parts, dim, device):
    """one array for the native call from the per-image rows: (keep-alive, pointer, on_device)"""
    if parts and all(_is_torch(p) for p in parts):
        import torch
        live = [p for p in parts if p.shape[0] > 0]
        if live and all(p.is_cuda for p in live):
            if any(p.device.index != device for p in live):
                raise ValueError(f"matching: descriptors on another device than cuda:{device}")
            keep = torch.cat(live, 0).contiguous()
            torch.cuda.synchronize(device)  # the context's stream does not wait for torch's streams
            return keep, C.c_void_p(keep.data_ptr()), 1
    parts = [p.cpu().numpy() if _is_torch(p) else p for p in parts]
    live = [p.reshape(-1, dim) for p in parts if p.shape[0] > 0]
    keep = np.ascontiguousarray(np.concatenate(live, 0), np.float32) if live else np.zeros((1, dim), np.float32)
    return keep, C.c_void_p(keep.ctypes.data), 0


def _wunsch_cfg(topk, num_samples, top_k_candidates, on_dev=0, want_scores=0):
    return _capi.LtMatchWunschConfig(int(topk), int(num_samples), int(top_k_candidates), on_dev, want_scores, 0)


def _match_flat_sold2(parts, valids, pair_off, pair_nb, topk, num_samples, top_k_candidates, device=0,
                      want_scores=False):
    """lt_match_wunsch_scene: parts = point-descriptor rows per image, valids = (N, S) uint8 per image"""
    ctx = _context(device)
    dim = _width(parts)
    line_off = np.zeros(len(parts) + 1, np.int64)
    line_off[1:] = np.cumsum([v.shape[0] for v in valids])
    desc_off = np.zeros(len(parts) + 1, np.int64)
    desc_off[1:] = np.cumsum([p.shape[0] for p in parts])
    keep, dptr, on_dev = _gather(parts, dim, device)
    valid = np.ascontiguousarray(np.concatenate([v.reshape(-1) for v in valids]) if valids else np.zeros(0), np.uint8)
    if valid.size == 0:
        valid = np.zeros(1, np.uint8)
    pair_off, pair_nb = _capi.i64(pair_off), _capi.i32(pair_nb)
    cfg = _wunsch_cfg(topk, num_samples, top_k_candidates, on_dev, 1 if want_scores else 0)
    n_rows = C.c_int64(0)
    ctx.chk(ctx.L.lt_match_wunsch_scene(ctx.h, len(parts), _capi.ptr(line_off, C.c_int64), _capi.ptr(desc_off, C.c_int64),
                                        dptr, valid.ctypes.data_as(C.POINTER(C.c_uint8)), dim,
                                        _capi.ptr(pair_off, C.c_int64),
                                        _capi.ptr(pair_nb if len(pair_nb) else _capi.i32([0]), C.c_int32),
                                        C.byref(cfg), C.byref(n_rows)))
    del keep
    n = int(n_rows.value)
    row_off = np.zeros(len(pair_nb) + 1, np.int64)
    rows = np.zeros((n, 2), np.int32)
    ctx.chk(ctx.L.lt_match_get(ctx.h, _capi.ptr(row_off, C.c_int64), _capi.ptr(rows, C.c_int32) if n else None))
    scores = None
    if want_scores:
        scores = np.zeros(n, np.float32)
        ctx.chk(ctx.L.lt_match_get_scores(ctx.h, scores.ctypes.data_as(C.POINTER(C.c_float)) if n else None))
    return row_off, rows, scores


def kernel_ms(device=0):
    """lt_match_wunsch_get_kernel_ms of the last sold2 call: device ms of the line-score kernel and of the NW kernel"""
    out = np.zeros(2)
    ctx = _context(device)
    ctx.chk(ctx.L.lt_match_wunsch_get_kernel_ms(ctx.h, out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def _host_pair_args(descinfo1, descinfo2, num_samples):
    a, va = _sold2_parts(descinfo1, num_samples)
    b, vb = _sold2_parts(descinfo2, num_samples)
    a = a.cpu().numpy() if _is_torch(a) else a
    b = b.cpu().numpy() if _is_torch(b) else b
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
    out = np.zeros(4)
    ctx = _context(device)
    ctx.chk(ctx.L.lt_match_get_timers(ctx.h, out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def _match_flat(parts, pair_off, pair_nb, kind, topk, device=0, want_scores=False):
    """the native call: parts = descriptor rows per image (all NumPy or all torch); returns row_off, rows, scores"""
    ctx = _context(device)
    dim = _width(parts)
    desc_off = np.zeros(len(parts) + 1, np.int64)
    desc_off[1:] = np.cumsum([p.shape[0] for p in parts])
    keep, dptr, on_dev = _gather(parts, dim, device)
    pair_off, pair_nb = _capi.i64(pair_off), _capi.i32(pair_nb)
    cfg = _capi.LtMatchConfig(int(kind), int(topk), on_dev, 1 if want_scores else 0)
    n_rows = C.c_int64(0)
    ctx.chk(ctx.L.lt_match_scene(ctx.h, len(parts), _capi.ptr(desc_off, C.c_int64), dptr, dim,
                                 _capi.ptr(pair_off, C.c_int64), _capi.ptr(pair_nb if len(pair_nb) else _capi.i32([0]), C.c_int32),
                                 C.byref(cfg), C.byref(n_rows)))
    n = int(n_rows.value)
    row_off = np.zeros(len(pair_nb) + 1, np.int64)
    rows = np.zeros((n, 2), np.int32)
    ctx.chk(ctx.L.lt_match_get(ctx.h, _capi.ptr(row_off, C.c_int64), _capi.ptr(rows, C.c_int32) if n else None))
    scores = None
    if want_scores:
        scores = np.zeros(n, np.float32)
        ctx.chk(ctx.L.lt_match_get_scores(ctx.h, scores.ctypes.data_as(C.POINTER(C.c_float)) if n else None))
    return row_off, rows, scores


def match_scene(descinfos, neighbors, kind="l2d2", topk=10, device=0, return_scores=False, num_samples=5,
                top_k_candidates=10):
    """Match every image of `neighbors` (img_id -> list of neighbour ids) against its neighbours in one native call.
    descinfos: img_id -> descinfo dict of the extractor (or the descriptor array itself), NumPy or torch GPU tensors.
    Returns {img_id: {ng_img_id: (n, 2) int32}} -- what ``TriangulateImage(img_id, matches)`` takes; with
    return_scores a second dict of the same shape with the FP32 score of every row.  kind "sold2": a descinfo is
    [desc (dim, num_samples N), valid (N, num_samples)]; topk == 0 is the mutual Needleman-Wunsch form over the
    top_k_candidates best lines (both keywords are used by this kind only)."""
    kind = _kind(kind)
    neighbors = {int(i): [int(j) for j in v] for i, v in neighbors.items()}
    ids = sorted(set(neighbors) | {j for v in neighbors.values() for j in v})
    index = {i: k for k, i in enumerate(ids)}
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
    if kind == SOLD2:
        row_off, rows, scores = _match_flat_sold2(parts, valids, pair_off, pair_nb, topk, num_samples, top_k_candidates,
                                                  device, return_scores)
    else:
        row_off, rows, scores = _match_flat(parts, pair_off, pair_nb, kind, topk, device, return_scores)
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
    a, b = _rows_of(desc1, kind), _rows_of(desc2, kind)
    if _is_torch(a):
        a = a.cpu().numpy()
    if _is_torch(b):
        b = b.cpu().numpy()
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
        _, rows, _ = _match_flat_sold2([b[0] for b in both], [b[1] for b in both], [0, 1, 1], [1], topk,
                                       self.num_samples, self.top_k_candidates, self.device)
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
