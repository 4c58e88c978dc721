"""limap.vplib on the GPU: the JLinkage vanishing-point detector with ``VPResult``, its config and
``get_vp_detector`` (vplib/bindings.cc, vpbase.h, base_vp_detector.{h,cc,py}, JLinkage/JLinkage.{h,cc,py},
register_vp_detector.py of limap; names and defaults follow them), plus a whole-scene call -- one set of launches for all
images instead of one serial pass per image spread over joblib processes:

    from limap_amd import vplib
    vpdetector = vplib.get_vp_detector(cfg["vpdet_config"], n_jobs=cfg["n_jobs"])
    vpresults = vpdetector.detect_vp_all_images(all_2d_lines, camviews)        # img_id -> VPResult
    triangulator.InitVPResults(vpresults)                                      # use_vp without limap

limap's own code around its J-Linkage third party (length filter, FP32 endpoints, the guard, the cluster filters,
``count_valid_supports_2d``, ``fitVP``, ``AssociateVPs``) is reproduced bit for bit.  The third party itself samples
its hypotheses at random, so no fixed output exists to equal: hypotheses, consistency test and clustering order are
this project's deterministic definition, computed by the HIP kernels of lt_kernels_vp.hip and,
identically, by a host path (``detect_vps_host``).  Two configuration keys are new: ``num_hypotheses`` (5000) and
``seed`` (0); upstream ignores both, as it ignores every unknown key.  ``GlobalVPTrackConstructor``, the VP-line
bipartites and Progressive-X are out of scope.
"""
import ctypes as C

import numpy as np

from . import _capi, _native
from .structures import lines2d_array

__all__ = ["VPTrack", "MergeVPTracksByDirection", "GlobalVPTrackConstructorConfig", "GlobalVPTrackConstructor", "VPResult", "BaseVPDetectorConfig", "BaseVPDetectorOptions", "DefaultVPDetectorOptions", "JLinkageConfig",
           "JLinkage", "get_vp_detector", "detect_vps", "detect_vps_host", "timers"]

_context = _capi.per_device_contexts()
_p = _capi.ptr


class VPResult:
    """vplib/vpbase.h:18-47: ``labels`` (one per line, -1: no vanishing point) and ``vps`` (homogeneous, unit norm)"""

    def __init__(self, labels=None, vps=None):
        if isinstance(labels, VPResult):
            labels, vps = labels.labels, labels.vps
        elif isinstance(labels, dict):  # ASSIGN_PYDICT_ITEM: a missing key keeps the empty default
            labels, vps = labels.get("labels"), labels.get("vps")
        self.labels = [] if labels is None else [int(x) for x in labels]
        self.vps = [] if vps is None else [np.array(v, np.float64).reshape(3) for v in vps]

    def as_dict(self):
        return {"labels": list(self.labels), "vps": [v.copy() for v in self.vps]}

    def count_lines(self):
        return len(self.labels)

    def count_vps(self):
        return len(self.vps)

    def GetVPLabel(self, line_id):
        return self.labels[line_id]

    def GetVPbyCluster(self, vp_id):
        return self.vps[vp_id]

    def HasVP(self, line_id):
        return self.GetVPLabel(line_id) >= 0

    def GetVP(self, line_id):
        if not self.HasVP(line_id):
            raise ValueError("Check failed: HasVP(line_id) == true")
        return self.GetVPbyCluster(self.GetVPLabel(line_id))


class BaseVPDetectorConfig:
    """vplib/base_vp_detector.h:20-35: keys that are present overwrite the defaults, unknown keys are ignored.
    ``num_hypotheses`` and ``seed`` are this backend's own keys; ``as_dict`` lists upstream's four."""

    KEYS = (("min_length", float), ("inlier_threshold", float), ("min_num_supports", int), ("th_perp_supports", float))
    OWN_KEYS = (("num_hypotheses", int), ("seed", int))

    def __init__(self, d=None):
        self.min_length = 40.0
        self.inlier_threshold = 1.0
        self.min_num_supports = 5
        self.th_perp_supports = 3.0
        self.num_hypotheses = 5000
        self.seed = 0
        if isinstance(d, BaseVPDetectorConfig):
            d = dict(d.as_dict(), num_hypotheses=d.num_hypotheses, seed=d.seed)
        for k, t in self.KEYS + self.OWN_KEYS:
            if d and k in d:
                setattr(self, k, t(d[k]))

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self.KEYS}

    def _struct(self):
        return _capi.LtVpConfig(self.min_length, self.inlier_threshold, self.th_perp_supports, self.min_num_supports,
                                self.num_hypotheses, self.seed & 0xFFFFFFFFFFFFFFFF)


class JLinkageConfig(BaseVPDetectorConfig):
    """vplib/JLinkage/JLinkage.h:18-23"""


class BaseVPDetectorOptions:
    """vplib/base_vp_detector.py:7-15 (a NamedTuple there): ``n_jobs`` is kept for the signature; the whole scene is one
    native call here"""

    def __init__(self, n_jobs=1):
        self.n_jobs = n_jobs

    def _replace(self, **kw):
        return BaseVPDetectorOptions(**{"n_jobs": self.n_jobs, **kw})


DefaultVPDetectorOptions = BaseVPDetectorOptions()


def _cfg(cfg):
    return cfg if isinstance(cfg, BaseVPDetectorConfig) else BaseVPDetectorConfig(cfg)


def _split(off, labels, vp_off, vps, clusters, want_clusters):
    out = []
    for m in range(len(off) - 1):
        r = VPResult(labels[off[m]:off[m + 1]].tolist(), vps[vp_off[m]:vp_off[m + 1]])
        out.append((r, clusters[off[m]:off[m + 1]].copy()) if want_clusters else r)
    return out


def _detect(lines_list, cfg, device=0, clusters=False):
    """one native call for the batch -> list of VPResult (with clusters: of (VPResult, cluster of every line))"""
    if not lines_list:
        return []
    ctx = _context(device)
    off, flat = _native.csr(lines_list, 4)
    st = cfg._struct()
    n_vps = C.c_int64(0)
    ctx.chk(ctx.L.lt_vp_detect(ctx.h, len(lines_list), _p(off, C.c_int64), _p(flat), C.byref(st), C.byref(n_vps)))
    labels = np.zeros(max(int(off[-1]), 1), np.int32)
    clu = np.zeros(max(int(off[-1]), 1), np.int32)
    vp_off = np.zeros(len(lines_list) + 1, np.int64)
    vps = np.zeros((max(n_vps.value, 1), 3))
    ctx.chk(ctx.L.lt_vp_get(ctx.h, _p(labels, C.c_int32), _p(vp_off, C.c_int64), _p(vps), _p(clu, C.c_int32)))
    return _split(off, labels, vp_off, vps, clu, clusters)


def _detect_host(lines_list, cfg, n_threads=0, clusters=False):
    if not lines_list:
        return []
    L = _capi.load_library()
    off, flat = _native.csr(lines_list, 4)
    st = cfg._struct()
    cap = int(sum(a.shape[0] // 3 for a in lines_list)) + 1
    labels = np.zeros(max(int(off[-1]), 1), np.int32)
    clu = np.zeros(max(int(off[-1]), 1), np.int32)
    vp_off = np.zeros(len(lines_list) + 1, np.int64)
    vps = np.zeros((cap, 3))
    rc = L.lt_fn_vp_detect_host(len(lines_list), _p(off, C.c_int64), _p(flat), C.byref(st), int(n_threads),
                                _p(labels, C.c_int32), _p(vp_off, C.c_int64), _p(vps), cap, _p(clu, C.c_int32))
    if rc != 0:
        raise ValueError("lt_fn_vp_detect_host: bad configuration or lines (see lt_vp_config in include/limap_amd.h), "
                         "or a check of InfiniteLine2d fails on a support line")
    return _split(off, labels, vp_off, vps, clu, clusters)


def _cluster_sets(words_list, device=0):
    """lt_vp_cluster_sets: the clustering kernel alone on caller-supplied preference sets, one (rows, words) uint64 array
    per image (the same width in all) -> list of the int32 roots of every image.  For tests."""
    if not words_list:
        return []
    ctx = _context(device)
    off = np.zeros(len(words_list) + 1, np.int64)
    off[1:] = np.cumsum([a.shape[0] for a in words_list])
    n_words = words_list[0].shape[1]
    assert all(a.ndim == 2 and a.shape[1] == n_words for a in words_list)
    flat = np.ascontiguousarray(np.concatenate(words_list, 0), np.uint64) if off[-1] else np.zeros((1, n_words), np.uint64)
    roots = np.zeros(max(int(off[-1]), 1), np.int32)
    ctx.chk(ctx.L.lt_vp_cluster_sets(ctx.h, len(words_list), _p(off, C.c_int64), n_words, _p(flat, C.c_uint64),
                                     _p(roots, C.c_int32)))
    return [roots[off[m]:off[m + 1]].copy() for m in range(len(words_list))]


def detect_vps(all_2d_lines, cfg=None, device=0):
    """AssociateVPs for every image of ``all_2d_lines`` (dict img_id -> lines in any form structures.lines2d_array
    accepts) in one native call.  Returns dict img_id -> VPResult in the key order of ``all_2d_lines``.  The result of an
    image does not depend on the other images of the call."""
    cfg = _cfg(cfg)
    keys = list(all_2d_lines.keys())
    res = _detect([lines2d_array(all_2d_lines[k]) for k in keys], cfg, device)
    return dict(zip(keys, res))


def detect_vps_host(all_2d_lines, cfg=None, n_threads=0):
    """``detect_vps`` by the host path of the library (no device): the same results bit for bit, for tests and timing"""
    cfg = _cfg(cfg)
    keys = list(all_2d_lines.keys())
    res = _detect_host([lines2d_array(all_2d_lines[k]) for k in keys], cfg, n_threads)
    return dict(zip(keys, res))


def timers(device=0):
    """lt_vp_get_timers of the last device call: host ms of upload + length filter, kernels, download, host tail; device
    ms of the preference kernel and of the clustering kernel"""
    return _context(device).module_timers("lt_vp_get_timers", 6)


class BaseVPDetector:
    """vplib/base_vp_detector.py:21-78"""

    def __init__(self, options=DefaultVPDetectorOptions):
        self.n_jobs = options.n_jobs

    def get_module_name(self):
        raise NotImplementedError

    def detect_vp(self, lines, camview=None):
        raise NotImplementedError

    def detect_vp_all_images(self, all_lines, camviews=None):
        return {img_id: self.detect_vp(lines, None if camviews is None else camviews[img_id])
                for img_id, lines in all_lines.items()}


class JLinkage(BaseVPDetector):
    """vplib/JLinkage/JLinkage.py: ``cfg_jlinkage`` is the ``vpdet_config`` dict (or a config object)"""

    def __init__(self, cfg_jlinkage=None, options=DefaultVPDetectorOptions, device=0):
        super().__init__(options)
        self.config_ = JLinkageConfig(cfg_jlinkage)
        self.device = int(device)

    def as_dict(self):
        return self.config_.as_dict()

    def get_module_name(self):
        return "JLinkage"

    def detect_vp(self, lines, camview=None):
        return _detect([lines2d_array(lines)], self.config_, self.device)[0]

    def detect_vp_all_images(self, all_lines, camviews=None):
        return detect_vps(all_lines, self.config_, self.device)


def get_vp_detector(cfg_vp_detector, n_jobs=1):
    """vplib/register_vp_detector.py: the detector named by cfg_vp_detector["method"]"""
    options = BaseVPDetectorOptions()._replace(n_jobs=n_jobs)
    method = cfg_vp_detector["method"]
    if method == "jlinkage":
        return JLinkage(cfg_vp_detector, options)
    raise NotImplementedError  # "progressivex" (a learned third party) and anything else


# ---- 3D vanishing-point tracks (vplib/vptrack.h, global_vptrack_constructor.h): host containers and set-up of
# limap.runners.pointline_association ----
class VPTrack:
    """vplib/vptrack.h:21-35: a 3D direction and its supports (image id, 2D VP id)"""

    def __init__(self, direction=None, supports=None):
        if isinstance(direction, VPTrack):
            direction, supports = direction.direction, direction.supports
        elif isinstance(direction, dict):
            direction, supports = direction.get("direction"), direction.get("supports")
        self.direction = np.zeros(3) if direction is None else np.array(direction, np.float64).reshape(3)
        self.supports = [] if supports is None else [(int(a), int(b)) for a, b in supports]

    def as_dict(self):
        return {"direction": self.direction.copy(), "supports": list(self.supports)}

    def length(self):
        return len(self.supports)


def _angle_deg(a, b):
    c = min(abs(float(np.dot(a, b))), 1.0)
    return float(np.degrees(np.arccos(c)))


def MergeVPTracksByDirection(tracks, th_angle_merge=1.0):
    """vptrack.cc:21-104: union-find over the pairs within th_angle_merge that share no image; the merged direction is
    the length-weighted mean in input order, normalised; sorted by length (stable)"""
    tracks = [VPTrack(t) for t in tracks]
    n = len(tracks)
    parent = [-1] * n
    images = [set(i for i, _ in t.supports) for t in tracks]

    def root(i):
        while parent[i] != -1:
            i = parent[i]
        return i
    for i in range(n - 1):
        ri = root(i)  # read once per i, as upstream does
        for j in range(i + 1, n):
            rj = root(j)
            if ri == rj:
                continue
            if _angle_deg(tracks[i].direction, tracks[j].direction) > th_angle_merge:
                continue
            if images[ri] & images[rj]:
                continue
            if len(images[ri]) < len(images[rj]):
                parent[ri] = rj
                images[rj] |= images[ri]
                images[ri] = set()
            else:
                parent[rj] = ri
                images[ri] |= images[rj]
                images[rj] = set()
    labels, k = [-1] * n, 0
    for i in range(n):
        if parent[i] == -1:
            labels[i] = k
            k += 1
    for i in range(n):
        if labels[i] == -1:
            labels[i] = labels[root(i)]
    out = [VPTrack() for _ in range(k)]
    for i, t in enumerate(tracks):
        o = out[labels[i]]
        if not o.supports:
            o.direction = t.direction.copy()
        else:
            o.direction = (o.direction * o.length() + t.direction * t.length()) / (o.length() + t.length())
        o.supports += t.supports
    for o in out:
        o.direction = o.direction / np.linalg.norm(o.direction)
    return sorted(out, key=lambda t: -t.length())


class GlobalVPTrackConstructorConfig:
    """global_vptrack_constructor.h:20-31"""

    def __init__(self, d=None):
        self.min_common_lines, self.th_angle_verify, self.min_track_length = 3, 10.0, 5
        for k, typ in (("min_common_lines", int), ("th_angle_verify", float), ("min_track_length", int)):
            if d and k in d and d[k] is not None:
                setattr(self, k, typ(d[k]))


def _direction_from_vp(view, vp):
    """CameraView::get_direction_from_vp: R^T K^-1 vp, normalised"""
    d = view.R().T @ np.linalg.solve(view.K(), np.asarray(vp, float))
    return d / np.linalg.norm(d)


def _track_labels(nodes, edges):
    """ComputeTrackLabels (base/graph.cc:168-244): the edges (a, b, similarity) by descending (similarity, a, b); two
    components join unless they share an image, the one with fewer images under the other; the roots are numbered in
    node order"""
    n = len(nodes)
    parent = [-1] * n
    imgs = [{nd[0]} for nd in nodes]

    def root(i):
        while parent[i] != -1:
            i = parent[i]
        return i
    for a, b, _ in sorted(edges, key=lambda e: (e[2], e[0], e[1]), reverse=True):
        ra, rb = root(a), root(b)
        if ra == rb or imgs[ra] & imgs[rb]:
            continue
        if len(imgs[ra]) < len(imgs[rb]):
            ra, rb = rb, ra
        parent[rb] = ra
        imgs[ra] |= imgs[rb]
        imgs[rb] = set()
    labels, k = [-1] * n, 0
    for i in range(n):
        if parent[i] == -1:
            labels[i] = k
            k += 1
    return [labels[root(i)] for i in range(n)]


class GlobalVPTrackConstructor:
    """global_vptrack_constructor.h:33-51"""

    def __init__(self, cfg=None):
        self.config_ = cfg if isinstance(cfg, GlobalVPTrackConstructorConfig) else GlobalVPTrackConstructorConfig(cfg)
        self.vpresults_ = {}

    def Init(self, vpresults):
        self.vpresults_ = {int(k): VPResult(v) for k, v in vpresults.items()}

    def ClusterLineTracks(self, linetracks, imagecols):
        """global_vptrack_constructor.cc:8-120"""
        cfg, res = self.config_, self.vpresults_
        counters = {}
        for track in linetracks:
            edges = set()
            n = track.count_lines()
            for i in range(n - 1):
                i1, l1 = int(track.image_id_list[i]), int(track.line_id_list[i])
                if not res[i1].HasVP(l1):
                    continue
                node1 = (i1, res[i1].GetVPLabel(l1))
                d1 = _direction_from_vp(imagecols.camview(i1), res[i1].GetVP(l1))
                for j in range(i + 1, n):
                    i2, l2 = int(track.image_id_list[j]), int(track.line_id_list[j])
                    if i1 == i2 or not res[i2].HasVP(l2):
                        continue
                    node2 = (i2, res[i2].GetVPLabel(l2))
                    edge = (node1, node2) if i1 < i2 else (node2, node1)
                    if edge in edges:
                        continue
                    d2 = _direction_from_vp(imagecols.camview(i2), res[i2].GetVP(l2))
                    if _angle_deg(d1, d2) > cfg.th_angle_verify:
                        continue
                    edges.add(edge)
            for e in edges:
                counters[e] = counters.get(e, 0) + 1
        nodes, index, gedges = [], {}, []
        for e in sorted(counters):
            if counters[e] < cfg.min_common_lines:
                continue
            ids = []
            for nd in e:
                if nd not in index:
                    index[nd] = len(nodes)
                    nodes.append(nd)
                ids.append(index[nd])
            gedges.append((ids[0], ids[1], counters[e]))
        labels = _track_labels(nodes, gedges)
        by_label = {}
        for i, lb in enumerate(labels):
            by_label.setdefault(lb, VPTrack()).supports.append(nodes[i])
        out = []
        for lb in sorted(by_label):
            t = by_label[lb]
            if t.length() < cfg.min_track_length:
                continue
            avg = np.zeros(3)
            for img_id, vp_id in t.supports:
                avg = avg + _direction_from_vp(imagecols.camview(img_id), res[img_id].GetVPbyCluster(vp_id))
            avg = avg / float(t.length())
            t.direction = avg / np.linalg.norm(avg)
            out.append(t)
        return sorted(out, key=lambda t: -t.length())
