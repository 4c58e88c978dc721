#!/usr/bin/env python
"""bench.py -- line-triangulation hot path on N MI355X GPUs (one process per GPU).

    python bench.py --gpus 1 --steps 20 --warmup 3
    python bench.py --gpus 1 --steps 20 --warmup 3 --dump-outputs DIR   # + the last timed step's results as DIR/*.npy
    python bench.py --gpus 1 --full                                      # + every extra figure and check (below)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

Workload (BASELINE.json configs[1]): synthetic 100 views x 500 segments/view PER GPU, 20 neighbours, matched
mode topk = 10 (10^7 connections per GPU), cfgs/triangulation/default.yaml parameters, var2d = 2.0 (LSD).
At N > 1 the default is WEAK scaling: N connected rooms with 100 views each; every rank owns the 2D segments +
poses of its 100 images, and one RCCL all-gather over xGMI gives every rank the whole scene before it
triangulates its own images.  `--scaling strong` fixes the TOTAL job instead (`--config3` = BASELINE.json
configs[2]: 1000 views x 1000 segs over 4 rooms, sharded by image with connection-count weights).

One step = [all-gather of the per-image payload (N > 1)] + rebuild of the per-camera / per-segment invariants +
the whole device pipeline (pair invariants, candidate generation, placement, multi-view scoring, per-node
arg-max + valid edges) with the match lists already resident in HBM.  metric value = 3D line candidates scored
per second, whole job.

A plain run sets up, warms up, times the K steps, writes --dump-outputs and prints the line, which carries the
roofline of the scoring stage (HIP-event timed on the kernels' stream inside the timed region) with the FP64-VALU /
LDS view next to the HBM one.  `--full` adds everything that takes runs of its own: the generation kernels priced by
their own events, the merge of the shards and ComputeLineTracks with and without a step, the sustained loop, the
strong-scaling and streamed legs, batches in flight, the same measurements for exhaustive matching (CI config 1's
mode), the end-to-end wall-clock of the reference's API sequence (ctor + Init + TriangulateImage x views +
ComputeLineTracks, incl. PCIe and the host tail), and the CPU oracle timed on the host cores with a stage-by-stage
comparison of its results with the product's (rank 0, N = 1 only; a mismatch fails the run).
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0      # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
FP64_VALU_PEAK_TF = 78.6   # MI355X FP64 vector peak: AMD's product specification (78.6 TFLOP/s; = 256 CUs x 2.4 GHz x 128
                           # flop/clk/CU -- the guide has no FP64 figure); nothing here is an MFMA contraction
# cfgs/triangulation/default.yaml:102-110 (remerging.linker3d)
REMERGE_LINKER = dict(score_th=0.5, th_angle=5.0, th_overlap=0.001, th_smartoverlap=0.1, th_smartangle=1.0,
                      th_perp=1.0, th_innerseg=1.0)
DEVICE_SOURCES = ("lt_kernels.hip", "lt_kernels_v2.hip", "lt_kernels_score.hip", "lt_kernels_tail.hip", "lt_devfn.h", "lt_geom.h", "lt_device.h")


def device_source_hash():
    """Hash of the device code: counter-derived numbers under profiles/ are only quoted for the build they
    were measured on."""
    h = hashlib.sha256()
    for f in DEVICE_SOURCES:
        with open(os.path.join(ROOT, "limap_amd", "csrc", f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def algorithmic_bytes(stats, n_img_active, nn, survivors, mode, line_slots=False):
    """bytes_score = 136 C + 104 nodes + 4 E ;
    bytes_gen = 8 P + 32 (nodes + N nn M) + 88 N (1 + nn) + 96 C, with NO 8 P term in exhaustive mode (the
    connections are implicit there).  The rows reach the device packed to one 32-bit word each since round 3, so the
    row term priced here is 4 P (the smaller, i.e. stricter, figure: `achieved` = algorithmic bytes / time).
    Matched mode runs HOT LOOP 1 as two kernels; its bytes are split where the data is touched:
      k_gates    : every match row (4 P), the segment and camera records (the 32 / 88 terms), and the list of
                   rows that pass the gates (8 S, S = stage-A survivors; an entry carries the row)
      k_tri_rows : the survivor list (8 S) and the candidate records it emits (96 C)."""
    C, E, P, G = stats["candidates"], stats["valid_edges"], stats["connections"], stats["active_nodes"]
    # one packed word per match row (line | neighbour line << 16) in the row-slot form; 16 bits (the neighbour line: the
    # line is the lane) + 4 bytes of run length per (block, line) in the line-slot form of round 5
    rows = ((2 * P + 4 * nn * G) if line_slots else 4 * P) if mode == "matched" else 0
    score = 136 * C + 104 * G + 4 * E
    gen = rows + 32 * (G + nn * G) + 88 * n_img_active * (1 + nn) + 96 * C
    gates = rows + 32 * (G + nn * G) + 88 * n_img_active * (1 + nn) + 8 * survivors
    tri = 8 * survivors + 96 * C
    return {"score": score, "gen": gen, "gates": gates, "tri": tri}


def cpu_parity(T, O):
    """Product (after ComputeLineTracks) against the oracle on the same job: the bars of north_star --
    best candidate per node (global_line_triangulator.cc:145-153), valid-edge sets (:118-142), track
    membership and order (merging/merging.cc:84-101) identical, track endpoints <= 1e-5 relative IN THE SAME
    ORIENTATION (start to start, end to end: `n_swapped` counts tracks that would only match with start and end
    exchanged -- the SVD sign of merging/aggregator.cc:76-78 -- and must be 0)."""
    gb, ob = T.context().get_best(), O.get_best()
    best_ok = bool(np.array_equal(gb["has_best"], ob["has_best"]) and np.array_equal(gb["src"], ob["src"]))
    best_geom_ok = bool(np.array_equal(gb["line"], ob["line"]))
    sc_den = np.maximum(np.abs(ob["score"]), 1e-300)
    best_score_err = float(np.max(np.abs(gb["score"] - ob["score"]) / sc_den)) if len(sc_den) else 0.0
    (goff, ge), (ooff, oe) = T.context().get_valid_edges(), O.get_valid_edges()
    edges_ok = bool(np.array_equal(goff, ooff))
    if edges_ok and len(ge):  # order inside a node is unobservable (std::set): compare sorted per node
        node = np.repeat(np.arange(len(goff) - 1), np.diff(goff))
        kg = np.lexsort((ge[:, 1], ge[:, 0], node))
        ko = np.lexsort((oe[:, 1], oe[:, 0], node))
        edges_ok = bool(np.array_equal(ge[kg], oe[ko]))
    gt, ot = T.context().get_tracks(), O.get_tracks()
    members_ok = bool(all(np.array_equal(gt[k], ot[k]) for k in ("off", "image_ids", "line_ids", "node_ids")))
    err, n_swapped = None, None
    if members_ok and len(gt["line"]):
        gl, ol = gt["line"], ot["line"]
        scale = np.maximum(np.abs(ol[:, :6]).max(axis=1, keepdims=True), 1e-9)
        d_same = (np.abs(gl[:, :6] - ol[:, :6]) / scale).max(axis=1)
        d_swap = (np.abs(gl[:, :6] - np.concatenate([ol[:, 3:6], ol[:, 0:3]], 1)) / scale).max(axis=1)
        err = float(d_same.max())
        n_swapped = int(np.count_nonzero((d_swap < d_same) & (d_same > 1e-5)))
    st, so = T.stats(), O.stats()
    rep = {"best_src_identical": best_ok, "best_geometry_bit_exact": best_geom_ok, "best_score_max_rel_err": best_score_err,
           "edges_identical": edges_ok, "track_members_identical": members_ok, "max_endpoint_rel_err": err,
           "n_swapped": n_swapped,
           "tracks_cpu": so["tracks"], "tracks_gpu": st["tracks"], "candidates_cpu": so["candidates"],
           "candidates_gpu": st["candidates"], "valid_edges_cpu": so["valid_edges"], "valid_edges_gpu": st["valid_edges"]}
    from limap_amd.base import track_report  # limap's track report as a secondary signal
    rep["track_report_cpu"] = track_report(ot["off"], ot["image_ids"])
    rep["track_report_gpu"] = track_report(gt["off"], gt["image_ids"])
    ok = (best_ok and best_geom_ok and edges_ok and members_ok and best_score_err <= 1e-12
          and (err is None or (err <= 1e-5 and n_swapped == 0)) and so["tracks"] == st["tracks"] and so["candidates"] == st["candidates"]
          and rep["track_report_cpu"] == rep["track_report_gpu"])
    rep["ok"] = bool(ok)
    return ok, rep


def load_pmc(world, default_wl):
    """Counter-derived per-launch numbers (HBM bytes, FP64 VALU flops, LDS bytes) from the rocprofv3 --pmc passes
    committed under profiles/ -- valid for the default 1-GPU workload and ONLY for the device code they were
    collected on (source hash recorded in the file); anything else reports null."""
    path = os.path.join(ROOT, "profiles", "r06_pmc.json")
    if not (default_wl and world == 1 and os.path.exists(path)):
        return {}, None
    d = json.load(open(path))
    if d.get("device_source_hash") != device_source_hash():
        return {}, "profiles/r06_pmc.json was collected on different device code: counter-derived fields are null"
    return d.get("kernels", {}), None


def exhaustive_stage_pmc(pmc):
    """Counters of the exhaustive mode's scoring stage: since round 6 it runs in the split form -- k_depth_order (two size
    classes, summed by tools/prof_pmc_json.sh), the sweep kernel k_score3<sorted, split> and k_dense8 -- and one pair of events
    times the three (the dense kernel there is k_dense_rows since the last part of the round); LT_SCORE_FUSED=1: k_depth_order + the
    fused k_score3."""
    parts = [n for n in ("k_depth_order", "k_score3", "k_dense8", "k_dense_rows") if n in pmc]
    if os.environ.get("LT_SCORE_FUSED") or not ("k_dense8" in pmc or "k_dense_rows" in pmc) or "k_score3" not in pmc:
        return pmc
    out = dict(pmc)
    keys = set.intersection(*[set(k for k, v in pmc[n].items() if isinstance(v, (int, float))) for n in parts])
    out["k_score3"] = {k: sum(pmc[n][k] for n in parts) for k in keys if k not in ("valu_busy_frac", "lds_active_frac")}
    out["k_score3"]["per_kernel"] = {n: {k: v for k, v in pmc[n].items() if k != "raw"} for n in parts}
    return out


def roofline_entry(name, nbytes, ms, pmc):
    gbs = nbytes / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
    e = {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS,
         "traffic": None, "kernel_ms": ms, "algorithmic_bytes": nbytes}
    k = pmc.get(name)
    if k and ms > 0:
        e["traffic"] = k.get("hbm_bytes")
        if k.get("per_kernel"):
            e["per_kernel_counters"] = k["per_kernel"]
        if k.get("valu_flops_f64") is not None:
            tf = k["valu_flops_f64"] / (ms * 1e-3) / 1e12
            e["valu_f64"] = {"flops_per_launch": k["valu_flops_f64"], "achieved_tflops": tf, "peak_tflops": FP64_VALU_PEAK_TF,
                             "frac": tf / FP64_VALU_PEAK_TF, "valu_insts_per_launch": k.get("valu_insts")}
            if k.get("valu_insts"):
                # share of the VALU issue slots the kernel used: a wave64 VALU instruction occupies its SIMD for 4 cycles
                # (16 lanes per cycle); 256 CUs x 4 SIMDs at 2.4 GHz
                e["valu_f64"]["issue_frac"] = k["valu_insts"] * 4.0 / (1024.0 * 2.4e9 * ms * 1e-3)
        if k.get("lds_active_frac") is not None:
            e["lds"] = {"active_frac": k["lds_active_frac"], "what": "SQ_ACTIVE_INST_LDS / SQ_BUSY_CU_CYCLES"}
        fr = {"hbm": e["frac"], "valu_issue": e.get("valu_f64", {}).get("issue_frac", e.get("valu_f64", {}).get("frac", 0.0))}
        e["nearest_roof"] = max(fr, key=fr.get)
    return e


def feed(ctx, scene, imgs, mode, topk):
    for i in imgs:
        if mode == "matched":
            m = scene.matches_of(int(i), topk)
            nb = list(m.keys())
            off = np.zeros(len(nb) + 1, np.int64)
            off[1:] = np.cumsum([len(m[k]) for k in nb])
            pairs = np.concatenate([m[k] for k in nb], 0) if nb else np.zeros((0, 2), np.int32)
            ctx.triangulate_image(int(i), nb, off, pairs)
        else:
            ctx.triangulate_image_exhaustive(int(i), scene.neighbors[int(i)])
    ctx.upload()


def shard_node_ranges(scene, world, weights):
    """every rank's node range [g_lo, g_hi) under ltdist.shard_images (deterministic: each rank computes all of them) and a
    key capacity for the one-collective form of merge_shards_device: 8 valid edges per node of the largest shard (the
    bench scenes have 0.3-2; a rank that exceeds it fails loudly)"""
    from limap_amd import dist as ltdist
    ranges = []
    for r in range(world):
        imgs = ltdist.shard_images(scene.img_ids, r, world, weights)
        idx = np.searchsorted(scene.img_ids, imgs)
        ranges.append((int(scene.seg_off[idx[0]]), int(scene.seg_off[idx[-1] + 1])) if len(idx) else (0, 0))
    return ranges, 8 * max(max(b - a for a, b in ranges), 1)


def strong_config3_leg(cfg, rank, world, local_rank, dev, use_dist, steps=5, warmup=2, n_full=3):
    """BASELINE.json configs[2] (1000 views x 1000 segs, 4 rooms, 3000 GT segments, seed 1) as a STRONG-scaling leg of the
    same run: the fixed job is sharded by image over the `world` ranks, one all-gather per step brings the scene to every
    rank, each rank runs generation + scoring for its own images; `ms_per_step` = max over ranks, and
    `step_with_merge_and_tail_ms` adds the shards' way to rank 0 and rank 0's ComputeLineTracks.  One driver run of
    `bench.py --gpus N` thus yields north_star's config-3 curve beside the weak one."""
    import torch
    import torch.distributed as dist
    from limap_amd import _capi
    from limap_amd import dist as ltdist
    from limap_amd import synthetic as syn
    shape = dict(n_views=1000, n_segs=1000, n_neighbors=20, n_rooms=4, n_gt=3000, seed=1, topk=10)
    small = os.environ.get("LT_BENCH_STRONG_SCENE")  # tests: "views,segs,neighbors" of a scene that takes a second
    if small:
        v, sg, nbn = (int(x) for x in small.split(","))
        shape = dict(n_views=v, n_segs=sg, n_neighbors=nbn, seed=1, topk=10)
    scene = syn.make_scene(**shape)
    n_segs_img = np.diff(scene.seg_off)
    weights = np.array([len(scene.neighbors[int(i)]) * n_segs_img[n] * 10 for n, i in enumerate(scene.img_ids)], float)
    my_imgs = ltdist.shard_images(scene.img_ids, rank, world, weights)
    ctx = _capi.Context(cfg_dict=cfg, device=local_rank)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    ctx.set_ranges(*scene.ranges)
    gather = ltdist.SceneGather(scene.img_ids, scene.seg_off, rank, world, _comm_dev(dev), weights=weights, force_collective=use_dist)
    gather.load_local(scene.kvec, scene.qvec, scene.tvec, scene.segs)
    d_k, d_q, d_t, d_s = gather.all_gather()
    if ONE_GPU:
        d_k, d_q, d_t, d_s = d_k.to(dev), d_q.to(dev), d_t.to(dev), d_s.to(dev)
    ctx.init_device(scene.img_ids, d_k.data_ptr(), d_q.data_ptr(), d_t.data_ptr(), scene.seg_off, d_s.data_ptr())
    feed(ctx, scene, my_imgs, "matched", 10)
    if not ONE_GPU:
        ctx.set_scene_chunks(*gather.chunk_pointers())
    pending = [gather.gather_async()]
    merge_dev = None if ONE_GPU else dev

    def step():
        if pending[0] is not None:
            pending[0].wait()
        if gather.collective and not ONE_GPU:
            ctx.refresh_scene_chunks()
        pending[0] = gather.gather_async()
        ctx.run_device(wait=False)

    def sync():
        ctx.sync()
        torch.cuda.synchronize(dev)
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize(dev)

    def rmax(x):
        if not use_dist:
            return x
        t = torch.tensor([x], dtype=torch.float64, device=_comm_dev(dev))
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    for _ in range(warmup):
        step()
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    ctx.sync()
    torch.cuda.synchronize(dev)
    local = time.perf_counter() - t0
    sync()
    elapsed = rmax(time.perf_counter() - t0)
    my_idx = np.searchsorted(scene.img_ids, my_imgs)
    node_range = (int(scene.seg_off[my_idx[0]]), int(scene.seg_off[my_idx[-1] + 1])) if len(my_idx) else (0, 0)
    all_ranges, key_cap = shard_node_ranges(scene, world, weights)  # -> ONE collective per merge
    note = None
    tf0 = time.perf_counter()
    try:
        for it in range(n_full + 1):
            if it == 1:  # (the first pass sizes the tail's buffers: not timed)
                sync()
                tf0 = time.perf_counter()
            step()
            ctx.sync()
            if world > 1:
                ltdist.merge_shards_device(ctx, node_range, rank, world, merge_dev, all_ranges=all_ranges, key_cap=key_cap)
            if rank == 0:
                ctx.compute_tracks()
        sync()
    except Exception as e:
        note = f"{type(e).__name__}: {e}"
    full = rmax(time.perf_counter() - tf0)
    tail_ms = None
    if rank == 0 and note is None:  # rank 0's last ComputeLineTracks by stage (lt_get_timers slots 10, 22, 23)
        tmt = ctx.timers()
        tail_ms = {"total": tmt["tail"], "device_half_and_graph": tmt["tail_device"], "edge_order_and_union_find": tmt["tail_unionfind"],
                   "members_and_aggregation": tmt["tail"] - tmt["tail_device"] - tmt["tail_unionfind"]}
    # ... and PIPELINED: rank 0 enqueues the device half of step k's tail, then step k + 1, and does the host half of
    # step k's tail (graph, union-find, aggregation) while the device works on step k + 1 (lt_compute_tracks_begin / _end)
    over, over_note = None, None
    if note is None:
        try:
            def merge_and_begin():
                ctx.sync()
                if world > 1:
                    ltdist.merge_shards_device(ctx, node_range, rank, world, merge_dev, all_ranges=all_ranges, key_cap=key_cap)
                if rank == 0:
                    ctx.compute_tracks_begin()
            sync()
            step()
            merge_and_begin()
            to0 = time.perf_counter()
            for _ in range(n_full):
                step()
                if rank == 0:
                    ctx.compute_tracks_end()
                merge_and_begin()
            if rank == 0:
                ctx.compute_tracks_end()
            sync()
            over = rmax(time.perf_counter() - to0)
        except Exception as e:
            over_note = f"{type(e).__name__}: {e}"
    if pending[0] is not None:
        pending[0].wait()
        torch.cuda.synchronize(dev)
    st = ctx.stats()
    cand = float(st["candidates"])
    per_rank = [1e3 * local / steps]
    if use_dist:
        tot = torch.tensor([cand], dtype=torch.float64, device=_comm_dev(dev))
        dist.all_reduce(tot, op=dist.ReduceOp.SUM)
        cand = float(tot.item())
        allr = torch.zeros(world, dtype=torch.float64, device=_comm_dev(dev))
        dist.all_gather_into_tensor(allr, torch.tensor([per_rank[0]], dtype=torch.float64, device=_comm_dev(dev)))
        per_rank = allr.cpu().tolist()
    res = {"workload": (f"synthetic {shape['n_views']} views x {shape['n_segs']} segs/view in total, {shape['n_neighbors']} neighbours, "
                        "matched topk=10" + ("" if small else ", 4 rooms (BASELINE configs[2])")),
           "scaling": "strong", "n_gpus": world, "steps": steps, "ms_per_step": 1e3 * elapsed / steps,
           "value": cand * steps / elapsed, "unit": "candidates/s",
           "step_with_merge_and_tail_ms": None if note else 1e3 * full / n_full, "note": note, "tail_ms": tail_ms,
           "step_with_merge_and_tail_overlapped_ms": None if over is None else 1e3 * over / n_full,
           "overlapped_note": over_note or "the host half of step k's tail (rank 0) runs while the device works on step k + 1",
           "ms_per_step_per_rank": per_rank, "load_imbalance_max_over_mean": max(per_rank) / (sum(per_rank) / len(per_rank)),
           "n_ranks_rccl": dist.get_world_size() if (use_dist and dist.get_backend() == "nccl") else 0,
           "tracks_rank0": st["tracks"] if rank == 0 else None, "candidates": cand}
    del ctx
    return res


def streamed_config5_leg(cfg, rank, world, local_rank, dev, use_dist, pmc_path=None):
    """BASELINE.json configs[4] ("Rome16K / large COLMAP model (>= 5k images) streamed triangulation, 8 GPUs, HBM GB/s
    roofline report"; reference caller runners/rome16k/triangulation.py:15-45, cfgs/triangulation/rome16k.yaml) on its
    synthetic stand-in: 5000 views x 600 segs over 50 rooms, 20 neighbours, matched top-10, add_halfpix --
    STREAMED through limap_amd.stream: chunks of 250 consecutive images, each on a worker context that holds only the chunk's
    neighbour closure, chunk k on rank k % world, no collective while the chunks run, every rank's per-image results to rank 0
    through one gather, ONE ComputeLineTracks there.  A chunk's working set (30 M match rows, ~1.7 M candidate records,
    pair store) is ~0.45 GB: past the 256 MB Infinity Cache, so the per-kernel bytes / time here are HBM numbers."""
    import torch
    import torch.distributed as dist
    from limap_amd import stream as ltstream
    from limap_amd import synthetic as syn
    shape = dict(n_views=5000, n_segs=600, n_neighbors=20, n_rooms=50, seed=2)
    chunk = 250
    small = os.environ.get("LT_BENCH_STREAM_SCENE")  # tests: "views,segs,neighbors,chunk" of a scene that takes a second
    if small:
        v, sg, nbn, chunk = (int(x) for x in small.split(","))
        shape = dict(n_views=v, n_segs=sg, n_neighbors=nbn, seed=2)
    t0 = time.perf_counter()
    scene = syn.make_scene(**shape)
    t_scene = time.perf_counter() - t0
    cfg5 = dict(cfg)
    cfg5["add_halfpix"] = True  # cfgs/triangulation/rome16k.yaml
    st = ltstream.StreamedTriangulation(cfg5, scene.img_ids, scene.kvec, scene.qvec, scene.tvec, scene.seg_off, scene.segs,
                                        scene.neighbors, scene.ranges, chunk_images=chunk, rank=rank, world=world,
                                        device=local_rank, comm_device=_comm_dev(dev))

    def rmax(x):
        if not use_dist:
            return x
        t = torch.tensor([x], dtype=torch.float64, device=_comm_dev(dev))
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    def rsum(xs):
        if not use_dist:
            return list(xs)
        t = torch.tensor(list(xs), dtype=torch.float64, device=_comm_dev(dev))
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        return t.cpu().tolist()

    if use_dist:
        dist.barrier()
    tw0 = time.perf_counter()
    for ch in st.my_chunks():
        st.run_chunk(ch, scene.matches_of, fine_timers=True)
    torch.cuda.synchronize(dev)
    t_matches = 1e-3 * sum(r["matches_ms"] for r in st.per_chunk)  # the synthetic generator is not part of the pipeline
    wall_chunks = rmax(time.perf_counter() - tw0 - t_matches)
    tf0 = time.perf_counter()
    note = None
    A = None
    try:
        A = st.finish()
    except Exception as e:
        note = f"{type(e).__name__}: {e}"
    t_finish = rmax(time.perf_counter() - tf0)
    nn = shape["n_neighbors"]
    # per kernel: algorithmic bytes (the same formulas as the main line) and event time summed over this rank's
    # chunks, then over the ranks -- bytes / time = the rate one GPU sustains on a chunk
    keys = ("gates", "tri", "score")
    tkey = {"gates": "k_gates", "tri": "k_tri_rows", "score": "k_score3"}
    by, ms = {k: 0.0 for k in keys}, {k: 0.0 for k in keys}
    ws = []
    for r in st.per_chunk:
        G_act = int(r["images"]) * shape["n_segs"]
        ab = algorithmic_bytes(dict(candidates=r["candidates"], valid_edges=r["valid_edges"], connections=r["connections"],
                                    active_nodes=G_act), r["images"], nn, r.get("survivors", 0.0), "matched",
                               line_slots=bool(r.get("line_slots", 0.0)))
        for k in keys:
            by[k] += ab[k]
            ms[k] += r.get(tkey[k], 0.0)
        # what a chunk keeps resident in HBM while it runs: 16-bit transposed rows + run lengths, the derived per-segment
        # tables of the closure (128 + 80 B), candidate records (128 B) + meta / score / perm (32 B), the pair store of the
        # split scoring form (256 entries of 16 B per 64 candidates)
        ws.append(2 * r["connections"] + 4 * nn * G_act + 208 * r["closure_segments"] + 160 * r["candidates"] + 64 * r["candidates"])
    tot = rsum([by[k] for k in keys] + [ms[k] for k in keys] +
               [sum(r["device_ms"] for r in st.per_chunk), sum(r["candidates"] for r in st.per_chunk),
                sum(r["connections"] for r in st.per_chunk), float(len(st.per_chunk)),
                sum(r["init_ms"] for r in st.per_chunk), sum(r["buffer_ms"] for r in st.per_chunk),
                sum(r["upload_ms"] for r in st.per_chunk), sum(r["export_ms"] for r in st.per_chunk), float(sum(ws))])
    B = dict(zip(keys, tot[0:3]))
    T = dict(zip(keys, tot[3:6]))
    dev_ms, cands, conns, n_chunks, init_ms, buf_ms, up_ms, exp_ms, ws_sum = tot[6:15]
    pmc = {}
    if pmc_path and os.path.exists(pmc_path) and not small:
        d = json.load(open(pmc_path))
        if d.get("device_source_hash") == device_source_hash():
            pmc = d.get("kernels", {})
    names = {"gates": "k_gates_ln (stage A)", "tri": "k_tri_rounds (stage B)", "score": "scoring stage (k_score_q)"}
    roof = {}
    for k in keys:
        gbs = B[k] / (T[k] * 1e-3) / 1e9 if T[k] > 0 else 0.0
        roof[tkey[k]] = {"kernel": names[k], "bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": gbs / HBM_PEAK_GBS, "algorithmic_bytes_per_chunk": B[k] / max(n_chunks, 1),
                         "kernel_ms_per_chunk": T[k] / max(n_chunks, 1),
                         "traffic": (pmc.get(tkey[k], {}).get("hbm_bytes_per_chunk") if pmc else None)}
    res = {"workload": (f"synthetic {shape['n_views']} views x {shape['n_segs']} segs, {nn} neighbours, matched topk=10, add_halfpix"
                        + ("" if small else " (stand-in for BASELINE configs[4], rome16k.yaml)")
                        + f", streamed in chunks of {chunk} images with their neighbour closure, chunk k on rank k % {world}"),
           "n_gpus": world, "chunks": int(n_chunks), "chunk_images": chunk,
           "closure_images_max": int(rmax(float(max((r["closure_images"] for r in st.per_chunk), default=0)))),
           "connections": int(conns), "candidates": int(cands),
           "device_ms_per_chunk": dev_ms / max(n_chunks, 1),
           "host_ms_per_chunk": {"init_closure": init_ms / max(n_chunks, 1), "buffer_rows": buf_ms / max(n_chunks, 1),
                                 "upload": up_ms / max(n_chunks, 1), "download_export_import": exp_ms / max(n_chunks, 1)},
           "hbm_working_set_bytes_per_chunk": ws_sum / max(n_chunks, 1),
           "chunks_wall_s": wall_chunks, "images_per_s": shape["n_views"] / wall_chunks if wall_chunks > 0 else None,
           "candidates_per_s": cands / wall_chunks if wall_chunks > 0 else None,
           "candidates_per_s_device": cands / (dev_ms * 1e-3) * world if dev_ms > 0 else None,
           "gather_import_tail_s": t_finish, "tracks": (A.stats()["tracks"] if A is not None else None), "note": note,
           "roofline": roof, "scene_generation_s": t_scene,
           "timing_note": "chunks_wall_s = max over ranks of (wall of its chunks - time inside the synthetic match generator); "
                          "per-kernel times are HIP events of every chunk run (LT_FINE_TIMERS=2), bytes the SURVEY 8(d) formulas"}
    del st
    return res


_REAL_STDOUT = None
# LT_BENCH_ONE_GPU=1 (tests): an N-rank job whose ranks all use cuda:0 -- backend gloo (RCCL wants a device per rank), the
# scene gathered through host tensors and copied to the device, no per-step refresh from the receive buffer.  It exists to run
# the N > 1 control flow of this file (sharding, merges, reductions, the strong leg) on a one-GPU box.
ONE_GPU = os.environ.get("LT_BENCH_ONE_GPU") == "1"


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(ctx, out_dir, suffix=""):
    """`--dump-outputs DIR`: what the timed step hands its caller -- the per-node results of the last device run (best
    candidate per node, its support score and source, candidate counts, the valid edges) -- as DIR/<name>.npy in float64,
    so that two builds can be compared output for output.  Valid edges are sorted inside every node (their order there has
    no observable effect: it feeds a std::set).  Above 64 MB in all, a fixed seeded sample of the nodes is written (the
    sampled node indices are in `node_index`).  Returns {name: shape}."""
    best = ctx.get_best()
    n_tris = ctx.get_num_tris()
    off, edges = ctx.get_valid_edges()
    G = len(n_tris)
    node = np.repeat(np.arange(G, dtype=np.int64), np.diff(off))
    order = np.lexsort((edges[:, 1], edges[:, 0], node)) if len(edges) else np.zeros(0, np.int64)
    edges = edges[order]
    per_node = 10 + 1 + 2 + 1 + 1 + 1 + 1   # best_line, best_score, best_src, has_best, num_tris, node_index, edge count
    take = G
    while take > 0 and 8 * (per_node * take + 2 * len(edges) * take / max(G, 1)) > 0.9 * DUMP_LIMIT_BYTES:
        take //= 2
    idx = np.arange(G, dtype=np.int64) if take == G else np.sort(np.random.default_rng(0).choice(G, take, replace=False))
    cnt = np.diff(off)[idx]
    keep = np.zeros(G, bool)
    keep[idx] = True
    sel = np.nonzero(keep[node])[0]   # (node is ascending: the sampled nodes' edges stay in node order)
    arrays = {"node_index": idx, "best_line": best["line"][idx], "best_score": best["score"][idx],
              "best_src": best["src"][idx], "has_best": best["has_best"][idx], "num_tris": n_tris[idx],
              "valid_edge_count": cnt, "valid_edges": edges[sel].reshape(-1, 2)}
    arrays = {k: np.ascontiguousarray(v, np.float64) for k, v in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        raise RuntimeError(f"--dump-outputs: {total} bytes exceed the {DUMP_LIMIT_BYTES} byte limit")
    os.makedirs(out_dir, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(out_dir, k + suffix + ".npy"), a)
    return {k: list(a.shape) for k, a in arrays.items()}


def _comm_dev(dev):
    """device of the small tensors that go through collectives"""
    import torch
    return torch.device("cpu") if ONE_GPU else dev


def _quiet_stdout():
    """The driver reads ONE JSON line from stdout.  Libraries loaded along the way write there too (RCCL's version
    banner at init, the progress lines of the reference build timed as a CPU baseline): from here on file descriptor
    1 is stderr, and the JSON line alone goes to the saved descriptor."""
    global _REAL_STDOUT
    if _REAL_STDOUT is None:
        sys.stdout.flush()
        _REAL_STDOUT = os.dup(1)
        os.dup2(2, 1)


def _emit(line):
    sys.stdout.flush()
    try:
        import ctypes
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass
    data = (line + "\n").encode()
    fd = _REAL_STDOUT if _REAL_STDOUT is not None else 1
    while data:
        data = data[os.write(fd, data):]


def e2e_child(views, segs, neighbors, seed, topk):
    """`bench.py --e2e-child ...`: the reference's call sequence in a process WITHOUT torch -- what a caller of the library
    that does not import torch sees.  In a process that has imported torch the same repetitions measured 0.4-0.6 ms more
    (tools/profile_e2e_variants.py: 2.9-3.2 -> 3.4-3.8 ms; constructor + Init 0.43 -> 0.7-0.8).  Found at the end of round 6:
    the harness's own gc.collect() in front of every repetition walks the ~1e6 objects `import torch` leaves behind and the
    repetition starts with cold caches (gc.freeze() once, or no collection: constructor + Init back at 0.3-0.4); loading
    torch's libraries without the Python import, which HIP runtime serves the calls, OpenMP / MKL settings, NUMA confinement
    and malloc tunables change nothing.  The legs below freeze the collector's generations before their repetitions; this
    child stays as the figure of a torch-free caller.  Prints one E2E_CHILD json line."""
    import gc
    from limap_amd import merging, synthetic as syn, triangulation as tri
    sc = syn.make_scene(n_views=views, n_segs=segs, n_neighbors=neighbors, seed=seed)
    cfg = syn.default_triangulation_cfg()
    matches = {int(i): sc.matches_of(int(i), topk) for i in sc.img_ids}
    segs_list = [sc.segs_of(j) for j in range(sc.n_images)]
    n_rep = 6
    per_image, batched, with_post, parts = [], [], [], []
    n_tracks = n_post = 0
    gc.collect(); gc.freeze()
    for form in ("per_image", "batched"):
        for rep in range(n_rep):
            gc.collect()
            gc.disable()
            t0 = time.perf_counter()
            T = tri.GlobalLineTriangulator(cfg)
            T.SetRanges(sc.ranges)
            T.InitArrays(sc.img_ids, sc.kvec, sc.qvec, sc.tvec, segs_list)
            t1 = time.perf_counter()
            if form == "per_image":
                for i in sc.img_ids:
                    T.TriangulateImage(int(i), matches[int(i)])
            else:
                T.TriangulateAll(matches)
            t2 = time.perf_counter()
            tracks = T.ComputeLineTracks()
            t3 = time.perf_counter()
            n_tracks = len(tracks)
            if form == "per_image":
                per_image.append(1e3 * (t3 - t0))
                parts.append({"ctor_init": round(1e3 * (t1 - t0), 2), "buffer": round(1e3 * (t2 - t1), 2),
                              "compute_tracks": round(1e3 * (t3 - t2), 2)})
                ts = merging.TrackSet.from_triangulator(T)
                ts.filter_by_reprojection(8.0, 5.0).remerge(REMERGE_LINKER).filter_by_reprojection(8.0, 5.0)
                ts.filter_by_sensitivity(75.0, 3).filter_by_overlap(0.5, 3)
                with_post.append(1e3 * (time.perf_counter() - t0))
                n_post = len(ts)
                del ts
            else:
                batched.append(1e3 * (t3 - t0))
            gc.enable()
            del T, tracks
    med = lambda v: float(np.median(v[1:]))  # repetition 0 is the cold one
    _emit("E2E_CHILD " + json.dumps({
        "e2e_wall_ms": med(per_image), "e2e_with_postprocess_ms": med(with_post), "e2e_batched_ms": med(batched),
        "e2e_reps_ms": [round(x, 3) for x in per_image], "e2e_with_postprocess_reps_ms": [round(x, 3) for x in with_post],
        "e2e_batched_reps_ms": [round(x, 3) for x in batched], "e2e_reps_parts": parts, "tracks": n_tracks,
        "tracks_after_postprocess": n_post, "torch_in_process": "torch" in sys.modules}))


def main():
    _quiet_stdout()
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # defaults: a timed region of ~50 ms (200 steps of 0.25 ms) -- with 20 steps the 5 ms region carried ~4 % of fixed cost
    # (the first step's enqueue latency, the final synchronisation's wake-up) and was too short for an outside observer
    # of the GPU to see
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--views", type=int, default=100, help="views per GPU (weak scaling) / in total (strong scaling)")
    ap.add_argument("--segs", type=int, default=500)
    ap.add_argument("--neighbors", type=int, default=20)
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--rooms", type=int, default=0, help="rooms of the synthetic scene (default: one per 100 views)")
    ap.add_argument("--gt", type=int, default=0, help="ground-truth 3D segments (default: 600 per room)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--mode", default="matched", choices=["matched", "exhaustive"])
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"])
    ap.add_argument("--config3", action="store_true",
                    help="BASELINE.json configs[2]: strong scaling, 1000 views x 1000 segs over 4 rooms, 3000 GT segments, seed 1")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps: every extra figure and check -- per-kernel events, merge and tail, the "
                         "sustained loop, the legs, e2e wall-clock, CPU baselines and parity (the options below shape it)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baselines and parity")
    ap.add_argument("--cpu-threads", type=int, default=0)
    ap.add_argument("--no-extras", action="store_true",
                    help="--full without the extras (batches in flight, exhaustive leg): profiling runs want the main kernels only")
    ap.add_argument("--strong-leg", default="auto", choices=["auto", "on", "off"],
                    help="BASELINE config 3 as a strong-scaling leg of a --full run (`strong_config3` in the line); auto = "
                         "with the default workload")
    ap.add_argument("--stream-leg", default="auto", choices=["auto", "on", "off"],
                    help="BASELINE config 5's stand-in (5000 x 600, streamed in chunks with neighbour closure, chunks round-robin "
                         "over the ranks) as a leg of a --full run (`streamed_config5` in the line); auto = with the default workload")
    ap.add_argument("--stream", action="store_true",
                    help="the streamed leg only: the line's value is the streamed job's candidates/s (5000 x 600)")
    ap.add_argument("--sustain-s", type=float, default=2.0,
                    help="--full, after the timed region: the same step looped for about this long (sustained_ms_per_step; "
                         "an outside observer of the device sees it busy); 0 = off")
    ap.add_argument("--e2e-child", nargs=5, type=int, metavar=("VIEWS", "SEGS", "NEIGHBORS", "SEED", "TOPK"),
                    help="internal: the end-to-end call sequence in this (torch-free) process, see e2e_child")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps: write the per-node results of the last timed step as DIR/<name>.npy "
                         "(float64, at most 64 MB; see dump_outputs)")
    args = ap.parse_args()
    if args.dump_outputs and args.stream:
        ap.error("--dump-outputs is not available with --stream")
    if args.dump_outputs and args.steps < 1:
        ap.error("--dump-outputs needs --steps >= 1")
    for leg in ("strong_leg", "stream_leg"):
        if getattr(args, leg) == "on" and not args.full:
            ap.error(f"--{leg.replace('_', '-')} on needs --full")
    if args.e2e_child:
        return e2e_child(*args.e2e_child)
    if args.config3:
        args.scaling, args.views, args.segs, args.rooms, args.gt, args.seed = "strong", 1000, 1000, 4, 3000, 1

    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (no CPU fallback)")
    if ONE_GPU:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # LT_BENCH_FORCE_DIST=1: take the multi-rank code path (process group, all-gather, barrier, reductions)
    # in a one-rank job -- a smoke test of the RCCL plumbing on a single GPU
    use_dist = world > 1 or os.environ.get("LT_BENCH_FORCE_DIST") == "1"
    if use_dist:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        if ONE_GPU:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    from limap_amd import _capi
    from limap_amd import synthetic as syn
    from limap_amd import dist as ltdist

    stream_pmc = os.path.join(ROOT, "profiles", "r06_stream_pmc.json")
    if args.stream:
        # the streamed job as its own line: one "step" = the whole model once through the chunks
        cfg = syn.default_triangulation_cfg()
        leg = streamed_config5_leg(cfg, rank, world, local_rank, dev, use_dist, pmc_path=stream_pmc)
        if rank == 0:
            sc = leg["roofline"]["k_score3"]
            _emit(json.dumps({
                "metric": "3D line candidates scored/sec, large model streamed in chunks (BASELINE configs[4] stand-in)",
                "value": leg["candidates_per_s"], "unit": "candidates/s", "n_gpus": world, "steps": 1, "warmup": 0,
                "ms_per_step": 1e3 * leg["chunks_wall_s"], "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
                "dtype": "f64", "data": "synthetic", "config": {"workload": leg["workload"]},
                "roofline": {"bound": "hbm", "achieved": sc["achieved"], "peak": sc["peak"], "unit": "GB/s", "frac": sc["frac"],
                             "traffic": sc["traffic"], "kernel": sc["kernel"]},
                "cpu_baseline": None, "streamed_config5": leg, "device_source_hash": device_source_hash()}))
        if use_dist:
            dist.barrier()
            dist.destroy_process_group()
        return

    strong = args.scaling == "strong"
    n_total = args.views if strong else args.views * world
    n_rooms = args.rooms or (max(1, n_total // 250) if strong else world)
    scene = syn.make_scene(n_views=n_total, n_segs=args.segs, n_neighbors=args.neighbors, n_rooms=n_rooms,
                           n_gt=(args.gt or None), seed=args.seed, topk=args.topk)
    cfg = syn.default_triangulation_cfg()
    # shard by image, balanced by the connections each image brings: matched = rows of its blocks,
    # exhaustive = its segments x its neighbours' segments
    n_segs_img = np.diff(scene.seg_off)
    idx_of = {int(i): n for n, i in enumerate(scene.img_ids)}
    if args.mode == "matched":
        weights = np.array([len(scene.neighbors[int(i)]) * n_segs_img[n] * args.topk for n, i in enumerate(scene.img_ids)], float)
    else:
        weights = np.array([n_segs_img[n] * sum(n_segs_img[idx_of[j]] for j in scene.neighbors[int(i)])
                            for n, i in enumerate(scene.img_ids)], float)
    my_imgs = ltdist.shard_images(scene.img_ids, rank, world, weights)

    ctx = _capi.Context(cfg_dict=cfg, device=local_rank)
    stream = torch.cuda.current_stream(dev)
    ctx.set_stream(stream.cuda_stream)
    ctx.set_ranges(*scene.ranges)

    # ---- scene payload: this rank uploads only its own images, the rest arrives by all-gather ----
    gather = ltdist.SceneGather(scene.img_ids, scene.seg_off, rank, world, _comm_dev(dev), weights=weights, force_collective=use_dist)
    gather.load_local(scene.kvec, scene.qvec, scene.tvec, scene.segs)
    d_k, d_q, d_t, d_s = gather.all_gather()
    if ONE_GPU:
        d_k, d_q, d_t, d_s = d_k.to(dev), d_q.to(dev), d_t.to(dev), d_s.to(dev)
    ctx.init_device(scene.img_ids, d_k.data_ptr(), d_q.data_ptr(), d_t.data_ptr(), scene.seg_off, d_s.data_ptr())

    # ---- this rank's images: buffer + upload the match lists (resident before the timed region) ----
    t_up0 = time.perf_counter()
    feed(ctx, scene, my_imgs, args.mode, args.topk)
    t_upload = time.perf_counter() - t_up0

    # per-step path: the invariants are rebuilt straight from the all-gather's receive buffer
    if not ONE_GPU:
        ctx.set_scene_chunks(*gather.chunk_pointers())
    merge_dev = None if ONE_GPU else dev

    # One step = the scene of one batch arrives by all-gather, the invariants are rebuilt from the receive
    # buffer, the hot path runs.  The collective for the NEXT step is launched as soon as this step's
    # invariants have been rebuilt (the receive buffer is free again), so it overlaps with the kernels:
    # K steps contain K all-gathers, the first one is waited for at the top of the first step.
    pending = [gather.gather_async()]

    def step():
        if pending[0] is not None:
            pending[0].wait()
        # the invariants (camera / segment records) are rebuilt from the receive buffer when an all-gather has refilled it;
        # a one-rank job without the collective has nothing new to rebuild them from (they were built by init_device)
        if gather.collective and not ONE_GPU:
            ctx.refresh_scene_chunks()
        pending[0] = gather.gather_async()
        # enqueue only: the host's end-of-run bookkeeping of step k (result slots, event timings) happens
        # after step k+1 has been enqueued; the sync below completes the last one inside the timed region
        ctx.run_device(wait=False)

    def sync():
        ctx.sync()
        torch.cuda.synchronize(dev)
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize(dev)

    # The library SAMPLES the events around the stages of pipelined runs (each one is a ~5 us bubble in the stream): every
    # LT_TIMER_SAMPLE-th run carries them (default 8).  The roofline's kernel duration is the mean over the sampled steps of
    # the timed region -- at least four of them.
    if "LT_TIMER_SAMPLE" not in os.environ:
        os.environ["LT_TIMER_SAMPLE"] = str(max(1, min(8, args.steps // 4)))
    event_sampling = int(os.environ["LT_TIMER_SAMPLE"])
    # Pre-roll (untimed, reported as `preroll` in the line): the W warm-up steps of a short command (--steps 20 --warmup 3 is
    # 0.75 ms of device work after seconds of set-up) end before the GPU has left its idle clocks -- measured: 0.242-0.247 ms per
    # step against 0.231 with 20 warm-up steps and 200 timed ones, the scoring stage 85 against 80 us.  ~40 ms of the same step
    # first, so that the K timed steps measure the device in the state a job that runs for longer than a millisecond sees.
    step()
    sync()
    tp0 = time.perf_counter()
    step()
    sync()
    est = max(time.perf_counter() - tp0, 1e-5)
    n_pre = int(max(0, min(200, 0.04 / est)))
    if use_dist:  # every rank the same count (rank 0's estimate)
        tpre = torch.tensor([n_pre], dtype=torch.int64, device=_comm_dev(dev))
        dist.broadcast(tpre, 0)
        n_pre = int(tpre.item())
    tp0 = time.perf_counter()
    for _ in range(n_pre):
        step()
    sync()
    preroll = {"steps": n_pre + 2, "ms": 1e3 * (time.perf_counter() - tp0),
               "why": "untimed steps before the W warm-up steps: the GPU leaves its idle clocks only after milliseconds of work"}
    for _ in range(args.warmup):
        step()
    sync()
    ctx.timer_sums(reset=True)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    ctx.sync()
    torch.cuda.synchronize(dev)
    elapsed_local = time.perf_counter() - t0   # this rank alone (load imbalance shows here)
    sync()
    elapsed = time.perf_counter() - t0
    acc, n_runs = ctx.timer_sums()  # the library sums its HIP-event timings over the runs (no per-step readout)
    assert n_runs == args.steps, (n_runs, args.steps)
    last = ctx.timers()
    for k in ("upload", "buffer"):
        acc[k] = last[k] * max(args.steps, 1)
    if acc.get("survivors", 0.0) == 0.0:  # counted on demand when the run did not have it on the host
        acc["survivors"] = last["survivors"] * max(args.steps, 1)
    kt = {k: v / max(args.steps, 1) for k, v in acc.items()}  # average HIP-event ms per launch
    dumped = None
    if args.dump_outputs:  # the results of the last timed step, read back after the clock has stopped
        dumped = dump_outputs(ctx, args.dump_outputs, suffix=f"_rank{rank}" if world > 1 else "")
    # The timed region carries the events around the dominant stage only (scoring = k_score_q: roofline).  The generation
    # kernels are priced in a few extra steps with their own events on (LT_FINE_TIMERS=2 costs ~5 us per step), --full only.
    if args.mode == "matched" and args.full:
        prev_fine = os.environ.get("LT_FINE_TIMERS")
        os.environ["LT_FINE_TIMERS"] = "2"
        os.environ["LT_TIMER_SAMPLE"] = "1"
        ctx.timer_sums(reset=True)
        for _ in range(5):
            step()
        sync()
        acc2, n2 = ctx.timer_sums(reset=True)
        if prev_fine is None:
            os.environ.pop("LT_FINE_TIMERS", None)
        else:
            os.environ["LT_FINE_TIMERS"] = prev_fine
        os.environ["LT_TIMER_SAMPLE"] = str(event_sampling)
        # (generation and placement stages too: the timed region records no event between them)
        for k in ("k_gates", "k_tri_rows", "gen", "compact"):
            kt[k] = acc2[k] / max(n2, 1)
    elif args.mode == "matched":  # (not measured: a plain run leaves them out of kernel_ms)
        for k in ("k_gates", "k_tri_rows", "gen", "compact"):
            kt.pop(k, None)
    if pending[0] is not None:  # the collective launched by the last step
        pending[0].wait()
        torch.cuda.synchronize(dev)

    # the collective alone (what the overlap hides): 10 all-gathers back to back
    allgather_us = None
    if use_dist and args.full:
        torch.cuda.synchronize(dev)
        dist.barrier()
        ta = time.perf_counter()
        for _ in range(10):
            gather.gather_only()
        torch.cuda.synchronize(dev)
        allgather_us = 1e6 * (time.perf_counter() - ta) / 10

    # the tail (not part of the timed step), --full only.  N > 1: the other shards' per-node results and valid-edge keys
    # travel to rank 0 device to device (ltdist.merge_shards_device: one gather of two flat buffers, no host copy, no
    # per-image export), and rank 0's tail runs on its device over the whole scene.  This rank's nodes are one range of
    # the global node index (images are sharded in id order).
    my_idx = np.searchsorted(scene.img_ids, my_imgs)
    node_range = (int(scene.seg_off[my_idx[0]]), int(scene.seg_off[my_idx[-1] + 1])) if len(my_idx) else (0, 0)
    merge_note, t_merge, t_tail = None, None, None
    if args.full:
        all_ranges, key_cap = shard_node_ranges(scene, world, weights)  # -> ONE collective per merge
        if world > 1:
            try:
                tm0 = time.perf_counter()
                ltdist.merge_shards_device(ctx, node_range, rank, world, merge_dev, all_ranges=all_ranges, key_cap=key_cap)
                t_merge = time.perf_counter() - tm0
            except Exception as e:  # never lose the throughput line over the (untimed) merge
                merge_note = f"merge failed: {type(e).__name__}: {e}"
        t_tail0 = time.perf_counter()
        ctx.compute_tracks()
        t_tail = time.perf_counter() - t_tail0
    st = ctx.stats()   # (reads this rank's per-node results back: the pair statistic is summed on the host)
    st["active_nodes"] = int(sum(scene.seg_off[j + 1] - scene.seg_off[j] for j in my_idx))
    step_full_ms, full_note, track_report_gpu = None, None, None
    if args.full:
        st_after = ctx.stats()
        # ---- second figure (not `value`): the step INCLUDING what `value` leaves out -- the per-node results' way to the
        # host, rank 0's import of the other shards (one tensor gather) and the serial tail ComputeLineTracks on rank 0
        # (global_line_triangulator.cc:234-351: the Amdahl part of an N-GPU run).  Strictly sequential per step; max
        # over ranks; reported beside ms_per_step so that a scaling curve shows both.
        n_full = max(1, min(args.steps, 5))
        sync()
        tf0 = time.perf_counter()
        try:
            for _ in range(n_full):
                step()
                ctx.sync()
                if world > 1:  # (nothing is downloaded: the tail works from device-resident results, merged on the device)
                    ltdist.merge_shards_device(ctx, node_range, rank, world, merge_dev, all_ranges=all_ranges, key_cap=key_cap)
                if rank == 0 or world == 1:
                    ctx.compute_tracks()
            sync()
        except Exception as e:
            full_note = f"{type(e).__name__}: {e}"
        full_elapsed = time.perf_counter() - tf0
        if pending[0] is not None:
            pending[0].wait()
            torch.cuda.synchronize(dev)
        if use_dist:
            t_f = torch.tensor([full_elapsed], dtype=torch.float64, device=_comm_dev(dev))
            dist.all_reduce(t_f, op=dist.ReduceOp.MAX)
            full_elapsed = float(t_f.item())
        step_full_ms = None if full_note else 1e3 * full_elapsed / n_full
        if rank == 0:  # limap's track report (visualize/trackvis/base.py:25-50): a secondary parity signal
            from limap_amd.base import track_report
            trk = ctx.get_tracks()
            track_report_gpu = track_report(trk["off"], trk["image_ids"])

    per_rank_ms = [1e3 * elapsed_local / max(args.steps, 1)]
    if use_dist:
        t_el = torch.tensor([elapsed], dtype=torch.float64, device=_comm_dev(dev))
        dist.all_reduce(t_el, op=dist.ReduceOp.MAX)
        elapsed = float(t_el.item())
        tot = torch.tensor([st["candidates"], st["connections"], st["pairs"]], dtype=torch.float64, device=_comm_dev(dev))
        dist.all_reduce(tot, op=dist.ReduceOp.SUM)
        cand_total, conn_total, pairs_total = [float(x) for x in tot.tolist()]
        loc = torch.tensor([per_rank_ms[0], float(st["candidates"]), float(len(my_imgs))], dtype=torch.float64, device=_comm_dev(dev))
        allr = torch.zeros(3 * world, dtype=torch.float64, device=_comm_dev(dev))
        dist.all_gather_into_tensor(allr, loc)
        allr = allr.cpu().numpy().reshape(world, 3)
        per_rank_ms = allr[:, 0].tolist()
        per_rank_cand, per_rank_imgs = allr[:, 1].tolist(), allr[:, 2].tolist()
    else:
        cand_total, conn_total, pairs_total = float(st["candidates"]), float(st["connections"]), float(st["pairs"])
        per_rank_cand, per_rank_imgs = [float(st["candidates"])], [float(len(my_imgs))]

    ms_per_step = 1e3 * elapsed / max(args.steps, 1)
    value = cand_total * args.steps / elapsed

    out = None
    parity_ok = True
    default_wl = (args.views, args.segs, args.neighbors, args.topk, args.scaling, args.seed, args.rooms, args.gt) == \
                 (100, 500, 20, 10, "weak", 0, 0, 0)
    pmc_all, pmc_note = load_pmc(world, default_wl)
    if rank == 0:
        ab = algorithmic_bytes(st, len(my_imgs), args.neighbors, kt.get("survivors", 0.0), args.mode,
                               line_slots=bool(last.get("line_slots", 0.0)))
        pmc = pmc_all.get(args.mode, {})
        # per-KERNEL durations: HIP events recorded on the launch stream right around each kernel
        # (lt_get_timers [13]-[15]); "gen" is the two-kernel stage HOT LOOP 1 for continuity with round-1 lines
        if args.mode == "matched":
            # scoring = scoreOneNode as TWO kernels since round 4 (k_score3: the sweep, writes the pairs that pass; k_dense8:
            # pair_score over them, maxima, sums), timed as one stage by the events around them; its counters are the sums
            # of the two kernels' (LT_SCORE_FUSED=1: one kernel, k_score3)
            # Round 6: ONE kernel again, k_score_q (sweep role, then dense role, per workgroup) -- its counters are the stage's
            two_kernels = bool(last.get("score_two_kernels", 0.0)) or bool(os.environ.get("LT_SCORE_TWO_KERNELS"))
            if "k_score_q" in pmc and not two_kernels and not os.environ.get("LT_SCORE_FUSED"):
                pmc = dict(pmc)
                pmc["k_score3"] = dict(pmc["k_score_q"])
            elif "k_dense8" in pmc and "k_score3" in pmc and not os.environ.get("LT_SCORE_FUSED"):
                a_, b_ = pmc["k_score3"], pmc["k_dense8"]
                pmc = dict(pmc)
                pmc["k_score3"] = {k: (a_[k] + b_[k]) for k in a_ if k in b_ and isinstance(a_[k], (int, float))
                                   and isinstance(b_[k], (int, float)) and k not in ("valu_busy_frac", "lds_active_frac")}
                pmc["k_score3"]["per_kernel"] = {n_: {k: v for k, v in e_.items() if k != "raw"}
                                                 for n_, e_ in (("k_score3(sweep)", a_), ("k_dense8", b_))}
            kernels = {"k_score3": (ab["score"], kt.get("k_score3", 0.0))}
            if args.full:  # (priced in the extra steps with their own events)
                kernels.update(k_gates=(ab["gates"], kt.get("k_gates", 0.0)), k_tri_rows=(ab["tri"], kt.get("k_tri_rows", 0.0)))
        else:
            pmc = exhaustive_stage_pmc(pmc)
            kernels = {"k_score3": (ab["score"], kt.get("k_score3", 0.0)), "k_gen_exhaustive": (ab["gen"], kt.get("gen", 0.0))}
        dom = max(kernels, key=lambda k: kernels[k][1])
        roof = {name: roofline_entry(name, nbytes, ms, pmc) for name, (nbytes, ms) in kernels.items()}
        kt["line_slots"] = last.get("line_slots", 0.0)
        if args.mode == "matched" and args.full and last.get("line_slots", 0.0):  # the stage names stay, the kernels are round 5's
            roof["k_gates"]["kernel"] = "k_gates_ln (stage A, line-slot form: one lane per line)"
            roof["k_tri_rows"]["kernel"] = "k_tri_rounds (stage B in rounds of 64 survivors)"
        if args.mode == "matched" and kt.get("gen", 0.0) > 0:
            roof["stage_gen(k_gates+k_tri_rows)"] = roofline_entry("stage_gen", ab["gen"], kt["gen"], {})
        wl = (f"synthetic {args.views} views x {args.segs} segs/view " + ("in total" if strong else "per GPU")
              + f", {n_rooms} room(s), {args.neighbors} neighbours, {args.mode}"
              + (f" topk={args.topk}" if args.mode == "matched" else "")
              + ", cfgs/triangulation/default.yaml params, var2d=2.0")
        out = {
            "metric": ("3D line candidates scored/sec (" + ("100 views x 500 segs per GPU" if default_wl else wl.split(",")[0])
                       + (", matched topk=%d)" % args.topk if args.mode == "matched" else ", exhaustive)")),
            "value": value, "unit": "candidates/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "config": {"workload": wl, "views_total": n_total, "segs_per_view": args.segs, "n_neighbors": args.neighbors,
                       "mode": args.mode, "topk": args.topk, "parallelism": f"shard-by-image x{world}",
                       "scene_seed": args.seed, "rooms": n_rooms},
            "counts": {"connections": conn_total, "candidates": cand_total, "scoring_pairs": pairs_total,
                       "valid_edges_rank0": st["valid_edges"]},
            "kernel_ms": kt, "preroll": preroll,
            "connections_per_s": conn_total * args.steps / elapsed,
            "roofline": dict(roof[dom], kernel=(dom if not (dom == "k_score3" and args.mode == "matched" and not os.environ.get("LT_SCORE_FUSED"))
                                                else ("k_score3 + k_dense8 (the scoring stage in its two-kernel form: sweep kernel + dense kernel, one pair of events)"
                                                      if (kt.get("score_two_kernels") or os.environ.get("LT_SCORE_TWO_KERNELS"))
                                                      else "k_score_q (the scoring stage, scoreOneNode, as one kernel: every workgroup sweeps its share "
                                                           "of the tiles, then evaluates units of finished tiles)")),
                             event_sampling=f"HIP events around the stage on every {event_sampling}. step of the timed region "
                                            "(LT_TIMER_SAMPLE; each event is a ~5 us bubble in the stream)"),
            "roofline_all": roof,
            "roofline_note": pmc_note or ("traffic / valu_f64 / lds: rocprofv3 --pmc passes over this exact device code "
                                          "(profiles/r06_pmc.json, tools/prof_pmc_json.sh); FP64 VALU peak 78.6 TF"),
            "host_ms": {"upload_matches": 1e3 * t_upload},
            "ranks": {"world_size": dist.get_world_size() if use_dist else 1,
                      "n_ranks_rccl": dist.get_world_size() if (use_dist and dist.get_backend() == "nccl") else 0,
                      "backend": (dist.get_backend() + (" (RCCL)" if dist.get_backend() == "nccl" else "")) if use_dist else None,
                      "ms_per_step_per_rank": per_rank_ms, "candidates_per_rank": per_rank_cand,
                      "load_imbalance_max_over_mean": (max(per_rank_ms) / (sum(per_rank_ms) / len(per_rank_ms))) if per_rank_ms else None,
                      "images_per_rank": per_rank_imgs},
            "device_source_hash": device_source_hash(),
        }
        if args.full:
            out["step_with_merge_and_tail_ms"] = step_full_ms
            out["step_with_merge_and_tail_note"] = full_note or (
                f"{n_full} steps of: all-gather + kernels + per-node results to the host + rank 0's import of the other "
                "shards + ComputeLineTracks on rank 0, sequential, max over ranks (not part of `value`)")
            out["counts"]["tracks_rank0"] = st_after["tracks"]
            out["host_ms"].update(tail_compute_tracks=1e3 * t_tail,
                                  merge_shards_device=None if t_merge is None else 1e3 * t_merge)
            out.update(tracks_whole_scene=st_after["tracks"], merge_note=merge_note, track_report=track_report_gpu)
            out["ranks"]["allgather_alone_us"] = allgather_us
        if dumped is not None:
            out["dumped_outputs"] = {"dir": args.dump_outputs, "arrays": dumped}

    # ---- the same step, sustained: the timed region above is a few milliseconds of a process that runs for tens of
    # seconds; this loop keeps the device on the step for --sustain-s so that an observer outside the process (the driver's
    # SMI sampler) sees it busy, and reports what the step costs when it is not a burst ----
    sustained = None
    if args.full and args.sustain_s > 0 and not args.no_extras:
        # (steps for about sustain_s seconds: from the faster of the two per-step figures at hand -- the timed region's and the
        # pre-roll's -- so that a short timed region's burst figure does not cut the loop short)
        per_step_ms = ms_per_step
        if preroll["steps"] >= 20:
            per_step_ms = min(per_step_ms, preroll["ms"] / (preroll["steps"] - 2))
        n_s = max(args.steps, int(args.sustain_s * 1e3 / max(per_step_ms, 1e-3)))
        if use_dist:
            t_n = torch.tensor([n_s], dtype=torch.int64, device=_comm_dev(dev))
            dist.broadcast(t_n, 0)
            n_s = int(t_n.item())
        sync()
        ts0 = time.perf_counter()
        for _ in range(n_s):
            step()
        sync()
        el_s = time.perf_counter() - ts0
        if use_dist:
            t_s = torch.tensor([el_s], dtype=torch.float64, device=_comm_dev(dev))
            dist.all_reduce(t_s, op=dist.ReduceOp.MAX)
            el_s = float(t_s.item())
        sustained = {"steps": n_s, "seconds": el_s, "sustained_ms_per_step": 1e3 * el_s / n_s}
        if pending[0] is not None:
            pending[0].wait()
            torch.cuda.synchronize(dev)
    if out is not None and sustained is not None:
        out["sustained_ms_per_step"] = sustained["sustained_ms_per_step"]
        out["sustained"] = sustained

    # ---- the strong-scaling leg: BASELINE config 3 over the same ranks (every rank takes part) ----
    if args.full and args.mode == "matched" and (args.strong_leg == "on" or (args.strong_leg == "auto" and default_wl and not args.no_extras)):
        try:
            sc3 = strong_config3_leg(cfg, rank, world, local_rank, dev, use_dist)
        except Exception as e:  # an extra: never lose the main line over it
            sc3 = {"error": f"{type(e).__name__}: {e}"}
        if out is not None:
            out["strong_config3"] = sc3

    # ---- the streamed leg: BASELINE config 5's stand-in over the same ranks (every rank takes part) ----
    if args.full and args.mode == "matched" and (args.stream_leg == "on" or (args.stream_leg == "auto" and default_wl and not args.no_extras)):
        try:
            s5 = streamed_config5_leg(cfg, rank, world, local_rank, dev, use_dist, pmc_path=stream_pmc)
        except Exception as e:  # an extra: never lose the main line over it
            s5 = {"error": f"{type(e).__name__}: {e}"}
        if out is not None:
            out["streamed_config5"] = s5

    # ---- extra (not `value`): independent batches in flight, N = 1 ----
    # A service that triangulates independent scenes keeps more than one batch in flight; two contexts (each
    # with its own stream and buffers, the same workload) overlap one batch's kernel tails and launch gaps
    # with the other's kernels.  `value` above stays the one-batch-at-a-time figure the per-kernel roofline
    # numbers belong to (HIP-event kernel durations are not meaningful while two streams interleave).
    if args.full and rank == 0 and world == 1 and args.mode == "matched" and not args.no_extras:
        def make_ctx():
            c = _capi.Context(cfg_dict=cfg, device=local_rank)
            c.set_ranges(*scene.ranges)
            c.init(scene.img_ids, scene.kvec, scene.qvec, scene.tvec, scene.seg_off, scene.segs)
            feed(c, scene, my_imgs, "matched", args.topk)
            return c
        try:
            pool = [make_ctx(), make_ctx()]
            res = {}
            for n_in_flight in (1, 2):
                use = pool[:n_in_flight]
                for s in range(2 * n_in_flight):
                    use[s % n_in_flight].run_device(wait=False)
                for c in use:
                    c.sync()
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for s in range(args.steps):
                    use[s % n_in_flight].run_device(wait=False)
                for c in use:
                    c.sync()
                torch.cuda.synchronize(dev)
                el = time.perf_counter() - t0
                res[str(n_in_flight)] = {"ms_per_batch": 1e3 * el / max(args.steps, 1),
                                         "candidates_per_s": cand_total * args.steps / el}
            out["batches_in_flight"] = dict(res, note="run only (no scene refresh); separate contexts and streams, "
                                                     "same workload per batch; not the headline value")
            del pool
        except Exception as e:  # an extra: never lose the main line over it
            out["batches_in_flight"] = {"error": f"{type(e).__name__}: {e}"}

    # ---- extra: the same scene with exhaustive matching (CI config 1's mode), N = 1 ----
    if args.full and rank == 0 and world == 1 and args.mode == "matched" and default_wl and not args.no_extras:
        try:
            cx = _capi.Context(cfg_dict=cfg, device=local_rank)
            cx.set_ranges(*scene.ranges)
            cx.init(scene.img_ids, scene.kvec, scene.qvec, scene.tvec, scene.seg_off, scene.segs)
            feed(cx, scene, my_imgs, "exhaustive", args.topk)
            n_x = max(3, min(args.steps, 8))
            cx.run_device(wait=True)
            cx.timer_sums(reset=True)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(n_x):
                cx.run_device(wait=False)
            cx.sync()
            torch.cuda.synchronize(dev)
            el = time.perf_counter() - t0
            accx, _ = cx.timer_sums()
            ktx = {k: v / n_x for k, v in accx.items()}
            cx.download()
            sx = cx.stats()
            sx["active_nodes"] = st["active_nodes"]
            abx = algorithmic_bytes(sx, len(my_imgs), args.neighbors, 0.0, "exhaustive")
            pmx = exhaustive_stage_pmc(pmc_all.get("exhaustive", {}))
            rx = {"k_score3": roofline_entry("k_score3", abx["score"], ktx.get("k_score3", 0.0), pmx),
                  "k_gen_exhaustive": roofline_entry("k_gen_exhaustive", abx["gen"], ktx.get("gen", 0.0), pmx)}
            out["exhaustive"] = {"ms_per_step": 1e3 * el / n_x, "value": sx["candidates"] * n_x / el, "unit": "candidates/s",
                                 "steps": n_x, "counts": {k: sx[k] for k in ("connections", "candidates", "pairs", "valid_edges")},
                                 "kernel_ms": {k: ktx[k] for k in ("run", "gen", "compact", "score", "select", "k_score3")},
                                 "roofline": rx, "note": "same scene, TriangulateImageExhaustiveMatch; run only (no scene refresh)"}
            del cx
        except Exception as e:
            out["exhaustive"] = {"error": f"{type(e).__name__}: {e}"}

    # ---- end-to-end wall-clock through the reference's API sequence, rank 0 / N = 1 ----
    if args.full and rank == 0 and world == 1:
        from limap_amd import triangulation as tri
        matches = {int(i): scene.matches_of(int(i), args.topk) for i in scene.img_ids} if args.mode == "matched" else None
        segs_list = [scene.segs_of(j) for j in range(scene.n_images)]
        e2e = []
        e2e_all_parts = []
        e2e_post, post_all = [], []   # the whole of line_triangulation(): ... + filters + remerge; the chain alone
        from limap_amd import merging
        import gc
        n_rep = 5
        # Everything alive now (torch's ~1e6 objects, the scene) leaves the collector's generations: the collection in front of
        # each repetition then walks only what the previous repetition left, instead of evicting the library's and the HIP
        # runtime's working set from the caches right before the clock starts (that was the "0.4-0.6 ms that come with
        # `import torch`" of the round's first lines: constructor + Init 0.6-0.7 ms against 0.3-0.4)
        gc.collect()
        gc.freeze()
        for rep in range(n_rep):
            torch.cuda.synchronize(dev)
            gc.collect()   # a generation-2 pass over the previous repetition's objects must not
            gc.disable()   # land inside one of the timed repetitions
            t0 = time.perf_counter()
            T = tri.GlobalLineTriangulator(cfg, device=local_rank)
            T.SetRanges(scene.ranges)
            T.InitArrays(scene.img_ids, scene.kvec, scene.qvec, scene.tvec, segs_list)
            t1 = time.perf_counter()
            for i in scene.img_ids:
                if args.mode == "matched":
                    T.TriangulateImage(int(i), matches[int(i)])
                else:
                    T.TriangulateImageExhaustiveMatch(int(i), scene.neighbors[int(i)])
            t2 = time.perf_counter()
            tracks_py = T.ComputeLineTracks()  # the call the runner makes (line_triangulation.py:168): returns the tracks
            e2e.append(time.perf_counter() - t0)
            # the steps that follow inside line_triangulation() (runners/line_triangulation.py:171-200, cfg defaults):
            # filter_by_reprojection, remerge to its fixed point, filter_by_reprojection, _by_sensitivity, _by_overlap
            tp0 = time.perf_counter()
            ts = merging.TrackSet.from_triangulator(T)
            ts.filter_by_reprojection(8.0, 5.0).remerge(REMERGE_LINKER).filter_by_reprojection(8.0, 5.0)
            ts.filter_by_sensitivity(75.0, 3).filter_by_overlap(0.5, 3)
            tp1 = time.perf_counter()
            post_all.append(1e3 * (tp1 - tp0))
            e2e_post.append(tp1 - t0)
            post_tracks = len(ts)
            del ts
            gc.enable()
            e2e_parts = {"ctor_init": 1e3 * (t1 - t0), "buffer": 1e3 * (t2 - t1), "compute_tracks": 1e3 * (e2e[-1] - (t2 - t0)),
                         "buffer_native": T.timers().get("buffer", 0.0)}
            e2e_all_parts.append({k: round(v, 2) for k, v in e2e_parts.items()})
            tm = T.timers()
            if rep == n_rep - 1:
                assert len(tracks_py) == st_after["tracks"] or world != 1
                T_last = T  # kept for the cpu_parity comparison below
            del T
        # repetition 0 is the cold one (device buffers, pinned staging and the host thread team are created): reported
        # on its own; the warm figure is the median of the others
        out["e2e_wall_ms"] = 1e3 * float(np.median(e2e[1:]))
        # ... and the same repetitions through the post-triangulation chain: the wall-clock of the reference's
        # line_triangulation() (north_star), median of the warm repetitions
        out["e2e_with_postprocess_ms"] = 1e3 * float(np.median(e2e_post[1:]))
        post_ms = float(np.median(post_all[1:]))
        out["e2e_cold_ms"] = 1e3 * e2e[0]
        out["e2e_breakdown_ms"] = dict(e2e_parts, **{k: tm[k] for k in ("upload", "run", "download", "tail")})
        out["e2e_reps_ms"] = [1e3 * x for x in e2e]
        # the same job with the TriangulateImage loop as ONE call (TriangulateAll: the rows of all images validated and
        # buffered in one pass) -- an extension of the reference's surface, reported beside the per-image form
        if args.mode == "matched":
            e2e_b, parts_b = [], None
            for rep in range(n_rep):
                torch.cuda.synchronize(dev)
                gc.collect()
                gc.disable()
                t0 = time.perf_counter()
                T = tri.GlobalLineTriangulator(cfg, device=local_rank)
                T.SetRanges(scene.ranges)
                T.InitArrays(scene.img_ids, scene.kvec, scene.qvec, scene.tvec, segs_list)
                t1 = time.perf_counter()
                T.TriangulateAll(matches)
                t2 = time.perf_counter()
                tracks_b = T.ComputeLineTracks()
                e2e_b.append(time.perf_counter() - t0)
                gc.enable()
                parts_b = {"ctor_init": 1e3 * (t1 - t0), "buffer": 1e3 * (t2 - t1), "compute_tracks": 1e3 * (e2e_b[-1] - (t2 - t0)),
                           "buffer_native": T.timers().get("buffer", 0.0)}
                assert len(tracks_b) == len(tracks_py)
                del T
            out["e2e_batched_ms"] = 1e3 * float(np.median(e2e_b[1:]))  # repetition 0 sizes its staging anew
            out["e2e_batched_cold_ms"] = 1e3 * e2e_b[0]
            out["e2e_batched_breakdown_ms"] = parts_b
            out["e2e_batched_reps_ms"] = [1e3 * x for x in e2e_b]
        out["e2e_reps_parts"] = e2e_all_parts
        # a FRESH process that calls limap_amd.warmup() (a synthetic scene of this shape, another seed, once through the
        # whole sequence) and then runs this scene once: what the first real scene of a pre-warmed service costs
        if args.mode == "matched" and default_wl and not args.no_extras:
            try:
                import subprocess
                code = ("import sys, time, gc; sys.path.insert(0, %r)\n"
                        "import limap_amd\nfrom limap_amd import synthetic as syn, triangulation as tri\n"
                        "sc = syn.make_scene(n_views=%d, n_segs=%d, n_neighbors=%d, seed=%d)\n"
                        "m = {int(i): sc.matches_of(int(i), %d) for i in sc.img_ids}\n"
                        "sl = [sc.segs_of(j) for j in range(sc.n_images)]\n"
                        "w = limap_amd.warmup(%d, %d, %d, %d)\ngc.collect(); gc.disable()\n"
                        "t0 = time.perf_counter()\nT = tri.GlobalLineTriangulator(syn.default_triangulation_cfg())\n"
                        "T.SetRanges(sc.ranges); T.InitArrays(sc.img_ids, sc.kvec, sc.qvec, sc.tvec, sl)\n"
                        "[T.TriangulateImage(int(i), m[int(i)]) for i in sc.img_ids]\nn = len(T.ComputeLineTracks())\n"
                        "print('AFTER_WARMUP', 1e3 * (time.perf_counter() - t0), 1e3 * w, n)\n"
                        % (os.path.dirname(os.path.abspath(__file__)), args.views, args.segs, args.neighbors, args.seed,
                           args.topk, args.views, args.segs, args.neighbors, args.topk))
                pr = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
                line = [l for l in pr.stdout.splitlines() if l.startswith("AFTER_WARMUP")]
                if line:
                    _, ms, wms, ntr = line[-1].split()
                    out["e2e_after_warmup_ms"] = float(ms)
                    out["warmup_ms"] = float(wms)
                    assert int(ntr) == len(tracks_py)
                else:
                    out["e2e_after_warmup_ms"] = {"error": pr.stderr[-300:]}
            except Exception as e:  # an extra: never lose the main line over it
                out["e2e_after_warmup_ms"] = {"error": f"{type(e).__name__}: {e}"}
        # the same call sequences in a process that has NOT imported torch (see e2e_child); the in-process figures above stay
        # the headline e2e_* fields
        if args.mode == "matched" and default_wl and not args.no_extras:
            try:
                import subprocess
                pr = subprocess.run([sys.executable, os.path.abspath(__file__), "--e2e-child", str(args.views), str(args.segs),
                                     str(args.neighbors), str(args.seed), str(args.topk)], capture_output=True, text=True,
                                    timeout=180)
                line = [l for l in pr.stdout.splitlines() if l.startswith("E2E_CHILD ")]
                if line:
                    ch = json.loads(line[-1][10:])
                    assert ch["tracks"] == len(tracks_py) and not ch["torch_in_process"]
                    ch["note"] = ("the same call sequences in a fresh child process that does not import torch (e2e_wall_ms above is "
                                  "measured in this process, which needs torch for the driver's contract; until the end of round 6 it "
                                  "read 0.4-0.6 ms more than this child: the harness's gc.collect() before each repetition walked "
                                  "torch's objects and the repetition started with cold caches -- gc.freeze() now, DESIGN.md section 4)")
                    out["e2e_clean_process"] = ch
                else:
                    out["e2e_clean_process"] = {"error": pr.stderr[-300:]}
            except Exception as e:  # an extra: never lose the main line over it
                out["e2e_clean_process"] = {"error": f"{type(e).__name__}: {e}"}
        out["postprocess"] = {"ms": post_ms, "reps_ms": [round(x, 3) for x in post_all], "tracks_after": post_tracks,
                              "steps": "filter_by_reprojection, remerge (to fixed point), filter_by_reprojection, "
                                       "filter_by_sensitivity, filter_by_overlap (cfgs/triangulation/default.yaml:102-115)"}

        if not args.no_cpu_baseline:
            from oracle import oracle as ora
            ora.build()
            n_cores = os.cpu_count() or 1
            cpu_model = None
            try:
                cpu_model = [l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")][0]
            except Exception:
                pass
            nthreads = args.cpu_threads or min(n_cores, 16)

            def run_cpu(mod, images, faithful, threads, exhaustive=False, tracks=True):
                mod.set_num_threads(threads)
                O = mod.OracleTriangulator(cfg, faithful=faithful)
                t0 = time.perf_counter()
                O.SetRanges(scene.ranges)
                O.Init(scene.img_ids, scene.kvec, scene.qvec, scene.tvec, scene.seg_off, scene.segs)
                for i in images:
                    if exhaustive:
                        O.TriangulateImageExhaustiveMatch(int(i), scene.neighbors[int(i)])
                    else:
                        O.TriangulateImage(int(i), matches[int(i)])
                if tracks:
                    O.ComputeLineTracks()
                return O, time.perf_counter() - t0

            # bounded sample: the same scene, first `n_s` images triangulated (all images as neighbours)
            n_s = min(len(scene.img_ids), 100 if args.mode == "matched" else 4)
            # The stated baseline is the BEST thread count, not a fixed one: the reference's OpenMP regions are per node
            # (<= 10 iterations each), so its fork/join cost grows with the team -- 16 threads are ~2x slower than 1 here.
            # Matched mode: the whole job (all images + ComputeLineTracks) at 1, 4 and 16 threads (64 threads were measured
            # once on the 256-CPU host of the GPU box: 73 s against 4.2 s at one thread -- not repeated in every run).
            by_threads = {}
            if args.mode == "matched" and n_s == len(scene.img_ids) and not args.cpu_threads:
                cand_threads = sorted({1, min(4, n_cores), min(16, n_cores)})
            else:
                cand_threads = [nthreads]
            O, cpu_s = None, None
            for th in cand_threads:
                O_t, s_t = run_cpu(ora, scene.img_ids[:n_s], True, th, exhaustive=args.mode != "matched")
                by_threads[str(th)] = {"wall_s": s_t, "candidates_per_s": O_t.stats()["candidates"] / s_t}
                if cpu_s is None or s_t < cpu_s:
                    O, cpu_s, nthreads = O_t, s_t, th
                del O_t
            so = O.stats()
            tp0 = time.perf_counter()
            ots = ora.OracleTrackSet(O)
            ots.filter_by_reprojection(8.0, 5.0); ots.remerge(REMERGE_LINKER); ots.filter_by_reprojection(8.0, 5.0)
            ots.filter_by_sensitivity(75.0, 3); ots.filter_by_overlap(0.5, 3)
            cpu_post_s, cpu_post_tracks = time.perf_counter() - tp0, ots.num_tracks()
            flags = "g++ -O2 -fopenmp -ffp-contract=off"
            out["cpu_baseline"] = {
                "value": so["candidates"] / cpu_s, "unit": "candidates/s", "cores": nthreads, "kind": "port",
                "sample": f"oracle (reference-faithful mode: by-value camview copies, per-call R()/K_inv(); {flags}), best of "
                          f"{cand_threads} OpenMP threads = {nthreads}: Init + TriangulateImage on {n_s} of {len(scene.img_ids)} "
                          f"images + ComputeLineTracks, {so['connections']} connections, {so['candidates']} candidates",
                "wall_s": cpu_s, "timers_s": O.timers(), "by_threads": by_threads,
                "postprocess_s": cpu_post_s, "postprocess_tracks_after": cpu_post_tracks,
                "host": {"logical_cpus": n_cores, "cpu_model": cpu_model},
            }
            if n_s == len(scene.img_ids):
                out["e2e_speedup_vs_cpu"] = cpu_s / (out["e2e_wall_ms"] * 1e-3)
                # whole line_triangulation() on both sides: ... + the post-triangulation chain
                out["e2e_with_postprocess_speedup_vs_cpu"] = (cpu_s + cpu_post_s) / (out["e2e_with_postprocess_ms"] * 1e-3)
            # stage-by-stage comparison of the product's results with the oracle's on the SAME job (the oracle
            # just ran it): arg-max per node, valid-edge sets, track memberships, endpoints (north_star bars)
            if n_s != len(scene.img_ids):  # bounded sample: run the product on the same image subset
                T_last = tri.GlobalLineTriangulator(cfg, device=local_rank)
                T_last.SetRanges(scene.ranges)
                T_last.InitArrays(scene.img_ids, scene.kvec, scene.qvec, scene.tvec, segs_list)
                for i in scene.img_ids[:n_s]:
                    if args.mode == "matched":
                        T_last.TriangulateImage(int(i), matches[int(i)])
                    else:
                        T_last.TriangulateImageExhaustiveMatch(int(i), scene.neighbors[int(i)])
                T_last.ComputeLineTracks()
            parity_ok, out["cpu_parity"] = cpu_parity(T_last, O)
            out["cpu_parity"]["images"] = n_s
            del O
            if args.mode == "matched" and default_wl and not args.no_extras:
                # the other CPU figures SURVEY 8(d) asks for, so that the GPU/CPU ratio is not read off one number:
                # one thread (per-core cost, no fork/join), hoisted invariants ("optimised CPU"), and the REFERENCE'S
                # OWN SOURCES (oracle/_ref, Eigen replaced by the stand-in headers) where that library travelled
                O2, s2 = run_cpu(ora, scene.img_ids, False, nthreads)
                out["cpu_baseline_optimised"] = {"value": O2.stats()["candidates"] / s2, "unit": "candidates/s", "cores": nthreads,
                                                 "kind": "port", "wall_s": s2, "timers_s": O2.timers(),
                                                 "sample": "oracle with the per-camera invariants hoisted (no by-value camview copies), "
                                                           f"{nthreads} threads, all images + ComputeLineTracks"}
                del O2
                try:
                    from oracle import ref as oref
                    if os.path.exists(oref.LIB_PATH):
                        R = oref.module()
                        O3, s3 = run_cpu(R, scene.img_ids, True, nthreads)
                        out["cpu_baseline_reference_build"] = {
                            "value": O3.stats()["candidates"] / s3, "unit": "candidates/s", "cores": nthreads, "kind": "reference",
                            "wall_s": s3, "tracks": O3.stats()["tracks"],
                            "sample": "oracle/_ref: limap::triangulation::GlobalLineTriangulator compiled from the reference's own "
                                      "sources (Eigen / COLMAP / PoseLib = stand-in headers, so slower than a real Eigen build), "
                                      f"{nthreads} threads, all images + ComputeLineTracks"}
                        del O3
                except Exception as e:
                    out["cpu_baseline_reference_build"] = {"error": f"{type(e).__name__}: {e}"}
                ora.set_num_threads(nthreads)
            # exhaustive leg: parity of the product with the oracle on an image subset
            if "exhaustive" in out and "error" not in out["exhaustive"]:
                try:
                    sub = [int(i) for i in scene.img_ids[:4]]
                    Tx = tri.GlobalLineTriangulator(cfg, device=local_rank)
                    Tx.SetRanges(scene.ranges)
                    Tx.InitArrays(scene.img_ids, scene.kvec, scene.qvec, scene.tvec, segs_list)
                    for i in sub:
                        Tx.TriangulateImageExhaustiveMatch(i, scene.neighbors[i])
                    Tx.ComputeLineTracks()
                    nthreads_x = args.cpu_threads or min(n_cores, 16)  # wide nodes (~450 candidates): the team pays here
                    Ox, sx_s = run_cpu(ora, sub, True, nthreads_x, exhaustive=True)
                    okx, repx = cpu_parity(Tx, Ox)
                    repx["images"] = len(sub)
                    out["exhaustive"]["cpu_parity"] = repx
                    out["exhaustive"]["cpu_baseline"] = {"value": Ox.stats()["candidates"] / sx_s, "unit": "candidates/s",
                                                         "cores": nthreads_x, "kind": "port", "wall_s": sx_s,
                                                         "sample": f"reference-faithful oracle, {len(sub)} images exhaustive + tail"}
                    parity_ok = parity_ok and okx
                    del Tx, Ox
                except Exception as e:
                    out["exhaustive"]["cpu_parity"] = {"error": f"{type(e).__name__}: {e}"}
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        # RCCL writes a version banner to the C stdout buffer; flush it first so that the JSON line is the
        # LAST line of stdout
        _emit(json.dumps(out))
        if not parity_ok:
            sys.stderr.write("bench.py: product and CPU oracle DISAGREE: %s\n" % json.dumps(out.get("cpu_parity")))
            sys.exit(3)


if __name__ == "__main__":
    main()
