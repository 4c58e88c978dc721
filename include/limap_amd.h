/*
 * limap_amd.h -- C ABI of the MI355X-native line-triangulation backend (liblimap_amd.so).
 *
 * Drop-in boundary for the hot path of cvg/limap's `limap.triangulation.GlobalLineTriangulator`
 * (reference pybind surface: src/limap/triangulation/bindings.cc:19-32,78-119; only production
 * caller: src/limap/runners/line_triangulation.py:102-168).  Plain pointers and sizes, no
 * exceptions across the boundary: every call returns 0 on success or a negative code, and
 * lt_last_error(ctx) holds the message the reference would have thrown.  One context per thread.
 *
 * All arithmetic is FP64 like the reference.  Image ids are arbitrary int32 values; internally
 * images are ordered by ascending id (the reference iterates std::map<int, ...>).  A "node" is an
 * (image, line) pair; global node index = seg_off[image index] + line id.
 */
#ifndef LIMAP_AMD_H
#define LIMAP_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LT_OK 0
#define LT_ERR_RUNTIME (-1)  /* std::runtime_error in the reference (bad matches, bad strategy) */
#define LT_ERR_ARGUMENT (-2) /* THROW_CHECK / std::out_of_range in the reference */
#define LT_ERR_HIP (-3)      /* HIP runtime failure */
#define LT_ERR_STATE (-4)    /* call-order violation (e.g. triangulate before init) */

/* Replaces GlobalLineTriangulatorConfig(py::dict) = BaseLineTriangulatorConfig
 * (triangulation/base_line_triangulator.h:20-43, .cc:16-31) + GlobalLineTriangulatorConfig
 * (triangulation/global_line_triangulator.h:11-24, .cc:18-29) + LineLinker2dConfig /
 * LineLinker3dConfig (base/line_linker.h:18-52,88-151, .cc:21-34,164-179), field for field.
 * lt_config_default() fills the reference's C++ defaults. */
typedef struct lt_config {
  int32_t debug_mode;
  int32_t add_halfpix;
  int32_t use_vp;                            /* VP-guided proposals (needs lt_init_vp) */
  int32_t use_endpoints_triangulation;
  int32_t disable_many_points_triangulation; /* many-points proposal (needs lt_set_bipartites) */
  int32_t disable_one_point_triangulation;
  int32_t disable_algebraic_triangulation;
  int32_t disable_vp_triangulation;
  double min_length_2d;
  double line_tri_angle_threshold;
  double IoU_threshold;
  double sensitivity_threshold;
  double var2d;
  double fullscore_th;
  int32_t max_valid_conns;
  int32_t min_num_outer_edges;
  int32_t merging_strategy; /* 0 "greedy", 1 "exhaustive", 2 "avg" (merging/merging.cc:18-368); any other
                               value -> LT_ERR_RUNTIME from lt_compute_tracks, where the reference throws
                               (global_line_triangulator.cc:314-316) */
  int32_t num_outliers_aggregator;
  double l2_score_th, l2_th_angle, l2_th_overlap, l2_th_smartoverlap, l2_th_smartangle,
      l2_th_perp, l2_th_innerseg;
  int32_t l2_use_angle, l2_use_overlap, l2_use_smartangle, l2_use_perp, l2_use_innerseg;
  int32_t _pad0;
  double l3_score_th, l3_th_angle, l3_th_overlap, l3_th_smartoverlap, l3_th_smartangle,
      l3_th_perp, l3_th_innerseg, l3_th_scaleinv;
  int32_t l3_use_angle, l3_use_overlap, l3_use_smartangle, l3_use_perp, l3_use_innerseg,
      l3_use_scaleinv;
} lt_config;

typedef struct lt_ctx lt_ctx;

void lt_config_default(lt_config *cfg);
int lt_abi_version(void);          /* bumped on any incompatible change of this header */
uint64_t lt_sizeof_config(void);   /* sizeof(lt_config) the library was built with */

/* GlobalLineTriangulator(cfg) -- bindings.cc:79-80,99.  device = HIP device ordinal.
 * Returns NULL (and writes a message to stderr) if no usable GPU / HIP runtime is present:
 * there is NO CPU fallback. */
lt_ctx *lt_create(const lt_config *cfg, int device);
void lt_destroy(lt_ctx *ctx);
const char *lt_last_error(lt_ctx *ctx);
/* run the kernels on a caller-owned hipStream_t (e.g. torch's current stream); NULL = own stream */
int lt_set_stream(lt_ctx *ctx, void *hip_stream);

/* SetRanges / UnsetRanges -- base_line_triangulator.h:61-65, bindings.cc:94-95 */
int lt_set_ranges(lt_ctx *ctx, const double lo[3], const double hi[3]);
int lt_unset_ranges(lt_ctx *ctx);

/* Init(all_2d_segs, imagecols) -- base_line_triangulator.cc:45-63, global_line_triangulator.cc:31-57.
 * kvec = (fx,fy,cx,cy) of the undistorted pinhole camera, qvec = (w,x,y,z), tvec; seg_off[n_img+1]
 * offsets into segs[.][4] = (x1,y1,x2,y2).  Host pointers; data is snapshotted (the reference
 * keeps a raw pointer to the caller's ImageCollection -- base_line_triangulator.cc:50). */
int lt_init(lt_ctx *ctx, int n_img, const int32_t *img_ids, const double *kvec, const double *qvec,
            const double *tvec, const int64_t *seg_off, const double *segs);
/* InitVPResults(vpresults) -- base_line_triangulator.h:47-49, bindings.cc:89.  Per image (any subset and
 * order of the ids given to lt_init) the VP label of every line (-1 = none; vplib/vpbase.h:35,42) and its
 * vanishing points (homogeneous image coordinates, vps[.][3]); CSR: label_off / vp_off [n_img + 1].
 * Used by the VP-guided proposals of triangulateOneNode (base_line_triangulator.cc:250-281) when
 * cfg.use_vp && !cfg.disable_vp_triangulation (both triangulation modes).  Call after lt_init. */
int lt_init_vp(lt_ctx *ctx, int n_img, const int32_t *img_ids, const int64_t *label_off, const int32_t *labels,
               const int64_t *vp_off, const double *vps);
/* SetBipartites2d(all_bpt2ds) / SetSfMPoints(points) -- base_line_triangulator.h:71-77, bindings.cc:90-91.
 * Per image (CSR pt_off) its 2D points: id, xy, point3D_id; per line (CSR line_off over the images, lp_off
 * over the lines -- every line of the image must be listed) the ids of its neighbouring points
 * (structures::PL_Bipartite2d::neighbor_points).  SfM points: point3D_id -> xyz; with none given the shared
 * points are triangulated from the two views.  Enables the many-points proposal of triangulateOneNode
 * (base_line_triangulator.cc:183-236: line fit through the shared 3D points + Pluecker projection) in
 * matched and exhaustive mode, and the one-point proposal (:238-248, one candidate per shared point, any number of
 * shared points per connection, as in the reference; see lt_fn_triangulate_line_with_one_point for the solver).
 * Call after lt_init. */
int lt_set_bipartites(lt_ctx *ctx, int n_img, const int32_t *img_ids, const int64_t *pt_off, const int32_t *pt_ids,
                      const double *pt_xy, const int32_t *pt_p3d, const int64_t *line_off, const int64_t *lp_off,
                      const int32_t *lp_ptids);
int lt_set_sfm_points(lt_ctx *ctx, int64_t n, const int32_t *ids, const double *xyz);
/* Same with kvec/qvec/tvec/segs already resident in HBM (e.g. the output of the RCCL all-gather),
 * images given in ascending id order. */
int lt_init_device(lt_ctx *ctx, int n_img, const int32_t *img_ids, const void *d_kvec,
                   const void *d_qvec, const void *d_tvec, const int64_t *seg_off,
                   const void *d_segs);

/* Re-read the scene arrays from HBM (same image set and segment counts as the last init) and
 * rebuild the per-camera / per-segment invariants on the context's stream, keeping the buffered
 * or uploaded images: the per-step entry of the multi-GPU path, called after the all-gather. */
int lt_refresh_scene_device(lt_ctx *ctx, const void *d_kvec, const void *d_qvec, const void *d_tvec,
                            const void *d_segs);

/* Multi-GPU per-step path without unpack copies: describe the scene as n_chunks chunks (one per
 * rank of the all-gather), chunk c holding images [img_begin[c], img_begin[c+1]) (indices in
 * ascending-id order) as four device arrays kvec | qvec | tvec | segs.  lt_set_scene_chunks records
 * the (persistent) buffer addresses once; lt_refresh_scene_chunks rebuilds the invariants from them
 * on the context's stream after every all-gather.  While a job is uploaded (lt_upload) only the images
 * that job references -- triangulated here, or a neighbour -- get their segment records rebuilt (a rank
 * of an N-GPU job needs ~1/N of the gathered scene); cameras are always rebuilt for all images. */
int lt_set_scene_chunks(lt_ctx *ctx, int n_chunks, const int32_t *img_begin, const void *const *d_kvec,
                        const void *const *d_qvec, const void *const *d_tvec, const void *const *d_segs);
int lt_refresh_scene_chunks(lt_ctx *ctx);

/* TriangulateImage(img_id, matches) -- base_line_triangulator.cc:71-109, bindings.cc:83.
 * Rows m_off[k]..m_off[k+1] of m_pairs[.][2] = (line_id, ng_line_id) belong to neighbour
 * nb_ids[k].  Calls are buffered; the GPU runs at the next lt_flush / lt_compute_tracks / getter
 * (observable behaviour is unchanged: results are only readable through those). */
int lt_triangulate_image(lt_ctx *ctx, int img_id, int n_nb, const int32_t *nb_ids,
                         const int64_t *m_off, const int32_t *m_pairs);
/* Same, with the (K,2) int32 row array of every neighbour given by its own pointer -- the natural
 * form of the std::map<int, Eigen::MatrixXi> argument; saves the caller a concatenation. */
int lt_triangulate_image_rows(lt_ctx *ctx, int img_id, int n_nb, const int32_t *nb_ids,
                              const int32_t *const *rows, const int64_t *n_rows);
/* The TriangulateImage loop of the caller (runners/line_triangulation.py:160-167: `for img_id in imagecols.get_img_ids():
 * Triangulator.TriangulateImage(img_id, matches)`) as ONE call: image k has the neighbours nb_ids[nb_off[k] .. nb_off[k+1])
 * and, for neighbour entry e in that range, the (n_rows[e], 2) int32 row array rows[e].  Same buffering, same validation
 * and the same errors as n calls of lt_triangulate_image_rows in the given order -- but one pass over all rows (one
 * parallel region over the (image, neighbour) blocks instead of one per call: the per-call form spends 2.1 ms of a
 * 5 ms end-to-end run on 100 calls of 0.8 MB each).  Atomic: on an error nothing of the call is kept.  No reference
 * counterpart (the reference's per-image call does the work itself). */
int lt_triangulate_all_rows(lt_ctx *ctx, int n_images, const int32_t *img_ids, const int64_t *nb_off, const int32_t *nb_ids,
                            const int32_t *const *rows, const int64_t *n_rows);
/* TriangulateImageExhaustiveMatch(img_id, neighbors) -- base_line_triangulator.cc:111-136 */
int lt_triangulate_image_exhaustive(lt_ctx *ctx, int img_id, int n_nb, const int32_t *nb_ids);

/* Staged execution of the buffered images (lt_flush = upload + run + download). */
int lt_upload(lt_ctx *ctx);     /* host staging -> HBM (matches, neighbour tables) */
int lt_run_device(lt_ctx *ctx); /* kernels only, inputs resident in HBM; repeatable */
/* The same run enqueued without waiting for it.  If the previous lt_run_device_async is still in flight it is
 * completed AFTER the new run has been enqueued, and ITS status is the return value (a streaming caller keeps
 * the device busy across the host's end-of-run bookkeeping); lt_sync completes the run in flight and returns
 * its status.  Every other entry point that touches results or inputs completes it first.  No reference
 * counterpart (the reference's TriangulateImage is synchronous host code).
 * Two configurations make the call SYNCHRONOUS in part: with extra proposals (VP, points) stage B runs twice and the host
 * waits for the candidate count between the two runs (it sizes the staging exactly; this also drains a run that was still
 * in flight); and when the bound-sized arrays of a batch would exceed 48 GB the exact count is fetched before placement. */
int lt_run_device_async(lt_ctx *ctx);
int lt_sync(lt_ctx *ctx);
int lt_download(lt_ctx *ctx);   /* per-node results -> host */
int lt_flush(lt_ctx *ctx);

/* ComputeLineTracks() -- global_line_triangulator.cc:353-359 */
int lt_compute_tracks(lt_ctx *ctx);
/* The same in two halves, for a caller that streams steps (rank 0 of a multi-GPU job; no reference counterpart):
 * _begin enqueues the device half of the tail behind the resident run -- valid-edge keys, sort, similarities, the graph
 * nodes' records into page-locked memory -- and returns; the caller may then enqueue the NEXT run (lt_run_device_async);
 * _end waits for the tail's own event, not for that run, and does the host half (graph, union-find, aggregation:
 * global_line_triangulator.cc:234-351) while the device works on the next step.  Needs the device form of the tail
 * (results of the run resident on the device; the node filter of min_num_outer_edges > 0 runs on the device too, over a
 * single context's run as over imported shards); lt_compute_tracks() == _begin + _end. */
int lt_compute_tracks_begin(lt_ctx *ctx);
int lt_compute_tracks_end(lt_ctx *ctx);

/* CountImages / CountLines -- base_line_triangulator.h:84-87 */
int64_t lt_count_images(lt_ctx *ctx);
int64_t lt_count_lines(lt_ctx *ctx, int img_id);
int64_t lt_num_nodes(lt_ctx *ctx);

/* Per-node results, node order = images ascending id x lines.
 * line10 = start3,end3,depths2,uncertainty,line.score ; score = multi-view support score;
 * src2 = (ng_img_id, ng_line_id) ; has_best = 0 for nodes without any candidate
 * (GetBestScoredTriNode / GetAllBestTris -- global_line_triangulator.cc:496-541). */
int lt_get_best(lt_ctx *ctx, double *out_line10, double *out_score, int32_t *out_src2,
                uint8_t *out_has_best);
int lt_get_num_tris(lt_ctx *ctx, int32_t *out_n_tris);
/* valid_edges_ (global_line_triangulator.cc:138-142) as CSR: (neighbour index, ng_line_id) */
int64_t lt_num_valid_edges(lt_ctx *ctx);
int lt_get_valid_edges(lt_ctx *ctx, int64_t *out_off, int32_t *out_edges2);
/* valid_flags_ (filterNodeByNumOuterEdges, global_line_triangulator.cc:168-232): 1 for nodes that keep at
 * least min_num_outer_edges valid edges to surviving nodes.  The reference fills it inside run_clustering
 * (:236), so this needs lt_compute_tracks first (LT_ERR_STATE otherwise); GetAllValidBestTris (:502-514). */
int lt_get_valid_flags(lt_ctx *ctx, uint8_t *out_flags);
/* All scored candidates of the last device run (GetScoredTrisNode; kept regardless of
 * debug_mode until the next run): CSR off[n_nodes+1], line10, score, src2. */
int64_t lt_num_all_tris(lt_ctx *ctx);
int lt_get_all_tris(lt_ctx *ctx, int64_t *out_off, double *out_line10, double *out_score,
                    int32_t *out_src2);
/* GetTracks() -- tracks as CSR over members (LineTrack fields, base/linetrack.h:33-42):
 * line7 = start3,end3,uncertainty; line3d10 = per support the Line3d of line3d_list in full: start3, end3, depths2,
 * uncertainty, score -- the post-triangulation steps read the uncertainties (merging/merging.cc:513-644 re-aggregates
 * from them), a (start, end) pair alone changes their outcome */
int64_t lt_num_tracks(lt_ctx *ctx);
int64_t lt_num_track_members(lt_ctx *ctx);
int lt_get_tracks(lt_ctx *ctx, double *out_line7, int64_t *out_off, int32_t *out_img_ids,
                  int32_t *out_line_ids, int32_t *out_node_ids, double *out_scores,
                  double *out_line3d10);

/* Multi-GPU tail: the rank that triangulated an image exports its per-node results (neighbour list,
 * best candidate per line, valid edges); the rank that runs ComputeLineTracks imports them for the
 * images it did not triangulate itself.  lt_image_results_size returns the image's line count and
 * its number of valid edges (array sizes for the export). */
int64_t lt_image_results_size(lt_ctx *ctx, int img_id, int64_t *n_edges);
int lt_export_image_results(lt_ctx *ctx, int img_id, int32_t *out_nb_ids /*[255]*/, int32_t *out_n_nb,
                            double *out_line10, double *out_score, int32_t *out_src2, int32_t *out_n_tris,
                            int64_t *out_edge_off, int32_t *out_edges2);
int lt_import_image_results(lt_ctx *ctx, int img_id, int n_nb, const int32_t *nb_ids, const double *line10,
                            const double *score, const int32_t *src2, const int32_t *n_tris,
                            const int64_t *edge_off, const int32_t *edges2);
/* The same for n images in ONE call and two flat blobs -- what a streamed job moves per chunk (limap_amd/stream.py:
 * BASELINE configs[4], runners/rome16k/triangulation.py:15-45) and what the ranks of a multi-GPU job gather to rank 0.
 * ints: n, then per image  img_id, n_nb, m (lines), ne (valid edges), nb_ids[n_nb], src[m][2], n_tris[m], edge_cnt[m],
 * edges[ne][2];  dbls: per image  line10[m][10], score[m]  (the layout of limap_amd.dist.pack_image_results, so blobs packed
 * either way are interchangeable).  lt_export_images_size returns the two lengths; lt_import_images_packed checks the
 * blob against n_ints / n_dbls and every id and count in it before it touches the context (LT_ERR_ARGUMENT otherwise). */
int lt_export_images_size(lt_ctx *ctx, int n, const int32_t *img_ids, int64_t *n_ints, int64_t *n_dbls);
int lt_export_images_packed(lt_ctx *ctx, int n, const int32_t *img_ids, int32_t *ints, double *dbls);
int lt_import_images_packed(lt_ctx *ctx, const int32_t *ints, int64_t n_ints, const double *dbls, int64_t n_dbls);

/* ---- shards of a multi-GPU run, device to device (no reference counterpart: the reference is one process).
 * Images are sharded over the ranks in id order, so a rank's nodes are one range [g_lo, g_hi) of the global node index
 * (node = first node of its image + line id).  A shard travels as two blobs -- lt_shard_node_bytes() bytes per node
 * (best candidate, score, source, candidate count of global_line_triangulator.cc:145-153, as arrays one behind the
 * other) and 8 bytes per valid edge (undirected node-pair keys of run_clustering, :243-290) -- written and read by
 * device copies; the pointers may be device or host memory.  Order of calls: every rank lt_shard_count; lt_shard_build
 * (total_keys = the sum over the ranks on the rank that merges, the own count elsewhere); the other ranks lt_shard_export;
 * the merging rank lt_shard_import once per other rank, then lt_compute_tracks (which needs the device form of the
 * tail).  With min_num_outer_edges > 0 the keys of a shard are DIRECTED (source node << kb | target node): the merging rank
 * runs filterNodeByNumOuterEdges (global_line_triangulator.cc:168-232) over the merged list before it sorts the undirected
 * form.  lt_shard_import checks on the device that every imported key
 * names two nodes of this scene as (min << kb | max) -- LT_ERR_ARGUMENT otherwise; the node blobs are taken as they are. */
int lt_shard_node_bytes(void);
int lt_shard_count(lt_ctx *ctx, int64_t *n_keys);
int lt_shard_build(lt_ctx *ctx, int64_t total_keys);
int lt_shard_export(lt_ctx *ctx, int64_t g_lo, int64_t g_hi, void *nodes_blob, void *keys_blob);
int lt_shard_import(lt_ctx *ctx, int64_t g_lo, int64_t g_hi, const void *nodes_blob, int64_t n_keys, const void *keys_blob);

/* ---- post-triangulation steps of limap.runners.line_triangulation (:171-200), SURVEY 8(f) rank 2:
 * limap.merging.filter_tracks_by_reprojection / remerge / filter_tracks_by_sensitivity /
 * filter_tracks_by_overlap (merging/merging_utils.cc:27-155, merging/merging.cc:513-644).
 * A track set is a host container of LineTracks (base/linetrack.h:21-50); cameras are those of the
 * context's Init.  member arrays: img/lid/nid int32, score f64, line2d4 = x1 y1 x2 y2,
 * line3d10 = start3 end3 depths2 uncertainty score; line7 = start3 end3 uncertainty. ---- */
typedef struct lt_trackset lt_trackset;
lt_trackset *lt_ts_from_ctx(lt_ctx *ctx); /* copy of GetTracks() with the auxiliary lists filled */
lt_trackset *lt_ts_create(int64_t n_tracks, const double *line7, const uint8_t *active, const int64_t *off,
                          const int32_t *img, const int32_t *lid, const int32_t *nid, const double *score,
                          const double *line2d4, const double *line3d10);
void lt_ts_destroy(lt_trackset *ts);
int64_t lt_ts_num_tracks(lt_trackset *ts);
int64_t lt_ts_num_members(lt_trackset *ts);
int lt_ts_get(lt_trackset *ts, double *line7, uint8_t *active, int64_t *off, int32_t *img, int32_t *lid,
              int32_t *nid, double *score, double *line2d4, double *line3d10);
/* _FilterSupportLines (merging_utils.cc:51-83) */
int lt_ts_filter_by_reprojection(lt_ctx *ctx, lt_trackset *ts, double th_angular2d, double th_perp2d,
                                 int num_outliers);
/* _FilterTracksBySensitivity (merging_utils.cc:105-128) */
int lt_ts_filter_by_sensitivity(lt_ctx *ctx, lt_trackset *ts, double th_angular3d, int min_supports);
/* _FilterTracksByOverlap (merging_utils.cc:130-155) */
int lt_ts_filter_by_overlap(lt_ctx *ctx, lt_trackset *ts, double th_overlap, int min_supports);
/* one pass of _RemergeLineTracks (merging/merging.cc:513-644); the LineLinker3d is read from the
 * l3_* fields of linker_cfg; the all-pairs connection test runs on the GPU */
int lt_ts_remerge_once(lt_ctx *ctx, lt_trackset *ts, const lt_config *linker_cfg, int num_outliers);
/* The device part of lt_ts_remerge_once alone, for tests: the all-pairs LineLinker3d::check_connection of
 * merging/merging.cc:519-556 (k_track_connect) over n_tracks lines (line7 = start3 end3 uncertainty) with their active
 * flags; the linker as above.  edges_out: the connected pairs as (min << 32 | max), sorted and unique; *n_unique their
 * number -- set also when edges_out (edges_cap entries) is too small, which returns LT_ERR_ARGUMENT.  capacity0: edge
 * slots of the first launch, 0 = the default max(65536, 32 n_tracks); a launch that finds more is repeated once with
 * room for all.  *n_raw: the device's edge counter of the launch that fitted (a pair of two active tracks counts from
 * both sides, unless every track is active: then each pair is tested once), *attempts: launches. */
int lt_fn_track_connect(lt_ctx *ctx, int64_t n_tracks, const double *line7, const uint8_t *active, const lt_config *linker_cfg,
                        int64_t capacity0, uint64_t *edges_out, int64_t edges_cap, int64_t *n_unique, int64_t *n_raw,
                        int32_t *attempts);

/* The per-connection decisions of candidate generation alone, for tests: n connections, each conn30 = seg1[4] cam1[11]
 * seg2[4] cam2[11] (cam = fx fy cx cy, qvec[4], tvec[3]), against the thresholds, bands and ranges of this context -- the
 * generation configuration a job of the context would run with.  One lane per connection builds the camera, segment
 * and pair records as a job does and writes, with plain stores,
 *   out10[10 i + 0] fast      the three-way stage-A gate (0 certainly skipped, 1 certainly passed, 2 undecided); the
 *                             LT_TEST_NO_FAST_GATES switch is ignored for this entry alone
 *   out10[10 i + 1] exact     the reference-exact stage-A gates
 *   out10[10 i + 2] tri_ok    the triangulation of stage B succeeded (the endpoint form under
 *                             use_endpoints_triangulation)
 *   out10[10 i + 3 .. 4]      the three-way sensitivity test in view 1 / view 2 (1 greater, 0 not, 2 undecided)
 *   out10[10 i + 5 .. 6]      the reference-exact `sensitivity > threshold` in view 1 / view 2
 *   out10[10 i + 7]           the stage-B pre-test (false: stage B certainly fails)
 *   out10[10 i + 8]           stage B as a whole
 *   out10[10 i + 9]           0
 * (entries 3 .. 6 are -1 where tri_ok is 0; under LT_TEST_NO_FAST_GATES the context's bands of the sensitivity test are
 * open, as in a job, and entries 3 .. 4 are 2 throughout), and iou_bits[i] = the 64 bits of compute_epipolar_IoU.  n in [0, 2^24];
 * arguments are checked before anything is launched; out10 holds 10 n and iou_bits n entries. */
int lt_fn_gate_outcomes(lt_ctx *ctx, int64_t n, const double *conn30, int32_t *out10, uint64_t *iou_bits);

/* ---- limap.merging.merging / MergeToLineTracks (merging/merging.py:6-21, merging/merging.cc:347-511): the merge of
 * one fitted 3D segment per 2D segment (runners/line_fitnmerge.py) into line tracks.  The context is initialised
 * (lt_init / lt_init_device, the images in any order) with the cameras and the 2D segments.  The merge reads the 2D
 * segments as given: a context created with add_halfpix = 1 does not shift them by half a pixel here, like the
 * reference's MergeToLineTracks (the triangulation on the same context still does).  seg3d = per image in ascending
 * id order, per line, start3 end3
 * (seg3d_off[n_img+1] offsets in segments: each image needs as many 3D as 2D segments, else LT_ERR_ARGUMENT); a
 * zero-length segment is not a node.  Neighbours as CSR over the images in ascending id order: nb_ids[nb_off[i] ..
 * nb_off[i+1]) in list order (an id that is not an image: LT_ERR_ARGUMENT).  The 2D linker is read from the l2_* fields
 * of linker_cfg, the 3D linker from the l3_* fields, switched to set_to_spatial_merging().  Every line gets
 * uncertainty = computeUncertainty(view, var2d).  The pair tests run on the GPU.  *out: a new track set (members in node
 * order, score = length, line3d10 with depths 0 and score -1, track line = aggregate with num_outliers 0); free it with
 * lt_ts_destroy.  The graph stays in the context until the next call. ---- */
int lt_merge_to_tracks(lt_ctx *ctx, const int64_t *seg3d_off, const double *seg3d, const int64_t *nb_off,
                       const int32_t *nb_ids, const lt_config *linker_cfg, double var2d, lt_trackset **out);
/* the graph of the last lt_merge_to_tracks: node count, edge count */
int lt_merge_graph_size(lt_ctx *ctx, int64_t *n_nodes, int64_t *n_edges);
/* nodes (image id, line id) in node order; edges (node_idx1, node_idx2, sim) in the reference's insertion order
 * (Graph::undirected_edges); any pointer may be NULL */
int lt_merge_graph_get(lt_ctx *ctx, int32_t *node_img, int32_t *node_line, int32_t *edge_n1, int32_t *edge_n2,
                       double *edge_sim);
/* of the last lt_merge_to_tracks: [0] device ms of the pair kernels (HIP events, last attempt), [1] host ms of the
 * whole call, [2] kernel attempts (more than 1 after an edge-buffer overflow), [3] edges */
int lt_merge_get_timers(lt_ctx *ctx, double out[4]);

/* ---- limap.fitting on the GPU (fitting/fitting.py:8-53, fitting/line3d_estimator.cc:7-109) ----
 * LO-MSAC options (LORansacOptions as estimators/bindings.cc:50-75 exposes them) plus the parameters of
 * estimate_seg3d_from_depth.  random_seed_ is honoured (`seed`): the reference reseeds from std::random_device. */
typedef struct lt_fit_config {
  double ransac_th;                /* 0.75: threshold = ransac_th * var2d * median(depth) / ((fx + fy) / 2) */
  double min_percentage_inliers;   /* 0.6: a fit with inlier ratio below it fails */
  double var2d;                    /* 5.0 */
  double squared_inlier_threshold; /* 1.0: lt_fit_points only (squared_inlier_threshold_) */
  double success_probability;      /* 0.9999, in [0, 1] */
  double threshold_multiplier;     /* sqrt(2) */
  int32_t min_num_iterations;      /* 100 */
  int32_t max_num_iterations;      /* 10000 */
  int32_t num_lo_steps;            /* 10 */
  int32_t num_lsq_iterations;      /* 4 */
  int32_t min_sample_multiplicator;  /* 7 */
  int32_t non_min_sample_multiplier; /* 3 */
  int32_t lo_starting_iterations;  /* 50 */
  int32_t final_least_squares;     /* 0 or 1 */
  uint64_t seed;                   /* 0 */
} lt_fit_config;

#define LT_DEPTH_F32 0
#define LT_DEPTH_F64 1
/* one depth map: h rows of w values, row r at ptr + r * row_stride elements; on_device = 1: a device pointer of the
 * context's device (read in place), 0: host memory (uploaded by the call) */
typedef struct lt_depth_map {
  const void *ptr;
  int64_t h, w, row_stride;
  int32_t dtype; /* LT_DEPTH_F32 or LT_DEPTH_F64 */
  int32_t on_device;
} lt_depth_map;

#define LT_FIT_OK 0
#define LT_FIT_TOO_FEW_POINTS 1  /* 6 or fewer pixels with a non-inf depth (fitting.py:46-47) */
#define LT_FIT_LOW_INLIER_RATIO 2 /* inlier ratio below min_percentage_inliers, no model counting as 0 (fitting.py:13) */

void lt_fit_config_default(lt_fit_config *cfg);
/* estimate_seg3d_from_depth (fitting/fitting.py:20-53) for every 2D segment of the images [img_begin, img_begin +
 * n_maps) of an initialised context (ascending id order; the segments as given, never shifted by add_halfpix), maps[k]
 * being the depth map of image img_begin + k.  Per segment, in the context's order from the first segment of img_begin:
 * seg3d = start3 end3 (zeros when the fit fails, like runners/line_fitnmerge.py:38-39), status = LT_FIT_*, stats (may be
 * NULL) = 5 int32: points kept, inliers, num_iterations, number_lo_iterations, 1 if the final model came from the
 * least-squares solver.  Validation (sizes, pointers, dtype, option ranges, segment coordinates finite and below 2^29 in
 * magnitude) happens before any device work: LT_ERR_ARGUMENT. */
int lt_fit_segs(lt_ctx *ctx, int img_begin, int n_maps, const lt_depth_map *maps, const lt_fit_config *cfg,
                double *seg3d, int32_t *status, int32_t *stats);
/* Fit3DPoints + estimate_seg3d (fitting/line3d_estimator.cc:7-44, fitting/fitting.py:8-18) over a CSR of point sets:
 * set s = xyz[3 off[s] .. 3 off[s+1]) (host memory, off[0] = 0), squared threshold cfg->squared_inlier_threshold.  Same
 * outputs as lt_fit_segs (status LT_FIT_OK or LT_FIT_LOW_INLIER_RATIO); inlier_mask (may be NULL): off[n_sets] bytes, 1
 * for the final inliers (stats.inlier_indices).  Needs no lt_init. */
int lt_fit_points(lt_ctx *ctx, int64_t n_sets, const int64_t *off, const double *xyz, const lt_fit_config *cfg,
                  double *seg3d, int32_t *status, int32_t *stats, uint8_t *inlier_mask);
/* one 3D point scan (estimate_seg3d_from_points3d, fitting/fitting.py:56-102): h rows of w pixels
 * of 3 channels (x, y, z in the camera frame, NaN where the scan has no point), channel c of pixel (r, x) at ptr + r *
 * row_stride + x * pix_stride + c * chan_stride elements (strides >= 0); img_h, img_w: the camera's image size (the
 * reference's camview.h(), camview.w()), which need not be the scan's.  dtype LT_DEPTH_F32 / LT_DEPTH_F64: float32 is
 * widened to double exactly (an extension: the reference's grid_sample refuses float32 scans).  on_device as
 * lt_depth_map. */
typedef struct lt_scan_map {
  const void *ptr;
  int64_t h, w, row_stride, pix_stride, chan_stride;
  int64_t img_h, img_w;
  int32_t dtype;
  int32_t on_device;
} lt_scan_map;

#define LT_FIT_SCAN_OUT_OF_RANGE 3 /* a kept sample normalises outside (-1, 1) of the scan (hloc's interpolate_scan assert) */

/* estimate_seg3d_from_points3d for every 2D segment of the images [img_begin, img_begin + n_maps), maps[k] being the
 * scan of image img_begin + k: linspace samples of the segment (int(2 |seg|) of them) strictly inside the camera's
 * image, bilinear scan interpolation with a per-channel nearest fallback, the samples without a NaN channel kept; the
 * threshold from the median ray depth; points R^T p - R^T t, or Tr[:3, :3] p + Tr[:3, 3] with Tr = scan_poses[12 k ..
 * 12 k + 12) (row-major 3 x 4; NULL: the camera transform for every image).  Outputs, timers and validation as
 * lt_fit_segs (h, w, img_h, img_w >= 2, the camera's below 2^24, poses finite); status LT_FIT_SCAN_OUT_OF_RANGE skips
 * the fit of that segment. */
int lt_fit_scans(lt_ctx *ctx, int img_begin, int n_maps, const lt_scan_map *maps, const double *scan_poses,
                 const lt_fit_config *cfg, double *seg3d, int32_t *status, int32_t *stats);
/* of the last lt_fit_segs / lt_fit_scans / lt_fit_points: [0] device ms of the fit kernel (HIP events, last attempt),
 * [1] device ms of the depth-map / scan upload, [2] host ms of the call, [3] kernel attempts (more than 1 when the scratch of long segments
 * overflowed) */
int lt_fit_get_timers(lt_ctx *ctx, double out[4]);

/* ---- limap.evaluation (evaluation/point_cloud_evaluator.cc, base_evaluator.cc, refline_evaluator.cc) on the GPU.
 * Lines are 6 doubles (start, end).  Distances are the reference's expressions bit for bit.
 * Inputs must be finite (LT_ERR_ARGUMENT otherwise).  chunk: queries (or cloud points) per launch, 0 = default.
 *
 * A point index on the context's device: the cloud in Morton order, buckets of 32 points, an implicit hierarchy of
 * bounding boxes.  xyz: n x 3 points, dtype 0 float32 (widened exactly) or 1 float64, on the host or (on_device) a
 * device pointer of the context's device.  perm (may be NULL): the order of a saved index (lt_pcd_get_perm), which
 * skips the sort; the points must be the ones it was saved with. */
typedef struct lt_pcd lt_pcd;
int lt_pcd_build(lt_ctx *ctx, const void *xyz, int64_t n, int dtype, int on_device, const uint32_t *perm,
                 lt_pcd **out);
void lt_pcd_free(lt_pcd *pcd);
/* the index order: perm[k] = input index of the k-th point in Morton order */
int lt_pcd_get_perm(lt_ctx *ctx, const lt_pcd *pcd, uint32_t *perm);
/* ComputeDistPoint over n query points (n x 3): the exact distance to the nearest cloud point */
int lt_pcd_nearest_dists(lt_ctx *ctx, const lt_pcd *pcd, const double *query, int64_t n, int64_t chunk,
                         double *dist);
#define LT_SAMPLE_CENTER 0 /* start + ((i + 0.5) / n) (end - start): ComputeInlierRatio, Compute*Segs */
#define LT_SAMPLE_ENDS 1   /* start + (i / (n - 1)) (end - start): ComputeDistLine (n >= 2) */
/* n_samples samples of each line against the cloud: dists (may be NULL) n_lines x n_samples nearest distances;
 * counts (may be NULL) n_lines x n_th samples with distance <= thresholds[t] (n_th <= 64) */
int lt_pcd_line_samples(lt_ctx *ctx, const lt_pcd *pcd, const double *lines, int64_t n_lines, int mode,
                        int n_samples, const double *thresholds, int n_th, int64_t chunk, double *dists,
                        int32_t *counts);
/* ComputeDistsforEachPoint: per cloud point (input order) the minimum of Line3d::point_distance over the lines,
 * DBL_MAX when there are none */
int lt_lines_point_dists(lt_ctx *ctx, const lt_pcd *pcd, const double *lines, int64_t n_lines, int64_t chunk,
                         double *dist);
/* RefLineEvaluator::ComputeRecallLength's counters: counts[r * n_th + t] = samples i < n_samples of query line r
 * (start + (length / (n - 1) * i) * direction) whose DistPointLines to `lines` is < thresholds[t] */
int lt_refline_counts(lt_ctx *ctx, const double *query_lines, int64_t n_query, const double *lines, int64_t n_lines,
                      int n_samples, const double *thresholds, int n_th, int64_t chunk, int32_t *counts);
/* MeshEvaluator (evaluation/mesh_evaluator.cc): distances to a triangle mesh (Ericson's
 * closest point on a triangle in a stated FP64 operation order, a project rule for faces whose interior denominator is
 * not > 0).  A triangle index on the context's device: faces in the Morton order of their centroids, buckets of
 * consecutive faces, the implicit hierarchy of lt_pcd.  V: nv x 3 vertices, dtype 0 float32 (widened exactly) or 1
 * float64, on the host or (on_device) a device pointer of the context's device; each coordinate is multiplied by scale
 * once (the reference's V_ *= mpau).  F: nf x 3 vertex indices (0-based, host memory).  LT_ERR_ARGUMENT for nf == 0,
 * a face index outside [0, nv), a non-finite scale or scaled coordinate. */
typedef struct lt_mesh lt_mesh;
int lt_mesh_build(lt_ctx *ctx, const void *V, int64_t nv, int dtype, int on_device, const int64_t *F, int64_t nf,
                  double scale, lt_mesh **out);
void lt_mesh_free(lt_mesh *mesh);
/* ComputeDistPoint over n query points (n x 3): the exact distance to the nearest face */
int lt_mesh_nearest_dists(lt_ctx *ctx, const lt_mesh *mesh, const double *query, int64_t n, int64_t chunk,
                          double *dist);
/* as lt_pcd_line_samples, against the mesh */
int lt_mesh_line_samples(lt_ctx *ctx, const lt_mesh *mesh, const double *lines, int64_t n_lines, int mode,
                         int n_samples, const double *thresholds, int n_th, int64_t chunk, double *dists,
                         int32_t *counts);
/* of the last evaluation call: [0] device ms of its kernels (HIP events), [1] host ms of the call, [2] launches,
 * [3] index levels (lt_pcd_build, lt_mesh_build) */
int lt_eval_get_timers(lt_ctx *ctx, double out[4]);

/* ---- limap.structures.PL_Bipartite2d (structures/pl_bipartite.cc) on the GPU, for a batch of images per call
 * (DESIGN.md section 16).  Images are given as CSR: the lines of image m are lines[4 line_off[m] .. 4 line_off[m+1])
 * (x1, y1, x2, y2; in ascending line-id order, which is the order of the reference's std::map), its points
 * pts[2 pt_off[m] .. 2 pt_off[m+1]); offsets start at 0.  Lines are named by their index within the image.  Needs no
 * lt_init.  Coordinates must be finite and no threshold NaN: LT_ERR_ARGUMENT before any launch otherwise (the reference
 * has no defined behaviour there).  An image without lines yields no edge and no junction (the reference's loop bounds
 * `count_lines() - 1` and `n_inters - 1` wrap around in size_t, pl_bipartite.cc:112,129).
 * PL_Bipartite2dConfig (structures/pl_bipartite.h:22-33), in pixels. */
typedef struct lt_bpt_config {
  double threshold_keypoints;
  double threshold_intersection;
  double threshold_merge_junctions;
} lt_bpt_config;
void lt_bpt_config_default(lt_bpt_config *cfg); /* 2.0 each */
/* PL_Bipartite2d::add_keypoint for every point (pl_bipartite.cc:56-67 under :69-82): point p is connected to line l
 * iff !(Line2d::point_distance(p) > threshold_keypoints) (base/linebase.cc:20-33, bit for bit).  The result stays in
 * the context: n_edges (may be NULL) receives its size, lt_bpt_associate_get copies it out -- edge_off[pt_off[n_img]
 * + 1] (may be NULL), and per point its line indices in ascending order, edge_line[n_edges] (may be NULL). */
int lt_bpt_associate(lt_ctx *ctx, int n_img, const int64_t *line_off, const double *lines, const int64_t *pt_off,
                     const double *pts, const lt_bpt_config *cfg, int64_t *n_edges);
int lt_bpt_associate_get(lt_ctx *ctx, int64_t *edge_off, int32_t *edge_line);
/* PL_Bipartite2d::compute_intersection_with_points(kps) on a bipartite that holds the lines only (pl_bipartite.cc:91-164):
 * the junction candidates -- both endpoints of every line, then intersect() (:166-204) of every line pair i < j in the
 * order of :112-124 -- merged by the union-find of :128-143 (union_find_get_root, base/graph.cc:157-166) over the pairs
 * within threshold_merge_junctions, each cluster replaced by merge_junctions (:206-223), and a merged junction dropped
 * iff the image has keypoints and KDTree::point_distance (util/kd_tree.h:96-98, taken as the exact minimum) is <
 * threshold_merge_junctions (:155-161).  The surviving junctions come in the order add_junction sees them, which is
 * the order of their point ids.  LT_ERR_ARGUMENT when an accepted intersection or a merged junction is not finite, for
 * more than 2^32 - 1 candidates or 2^31 close candidate pairs.  The result stays in the context; sizes (may be NULL)
 * receives {junctions, line indices of all junctions, candidates, close candidate pairs}.  lt_bpt_junctions_get copies
 * out (any pointer may be NULL) junc_off[n_img + 1], junc_xy[2 sizes[0]], id_off[sizes[0] + 1] and the ascending line
 * indices of every junction, line_idx[sizes[1]].  lt_bpt_junctions_get_candidates (for tests) copies out
 * cand_off[n_img + 1], cand_xy[2 sizes[2]], cand_lines[2 sizes[2]] (the candidate's one or two lines, -1 for none) and
 * parents[sizes[2]]: the union-find's array after the last root look-ups of :145-146, indices within the image. */
int lt_bpt_junctions(lt_ctx *ctx, int n_img, const int64_t *line_off, const double *lines, const int64_t *kp_off,
                     const double *kps, const lt_bpt_config *cfg, int64_t sizes[4]);
int lt_bpt_junctions_get(lt_ctx *ctx, int64_t *junc_off, double *junc_xy, int64_t *id_off, int32_t *line_idx);
int lt_bpt_junctions_get_candidates(lt_ctx *ctx, int64_t *cand_off, double *cand_xy, int32_t *cand_lines,
                                    int32_t *parents);
/* host ms of the stages of the last lt_bpt_associate / lt_bpt_junctions, each ended by a stream synchronisation:
 * [0] upload, [1] kernels (with the counts and prefix sums that size their outputs), [2] sorts, [3] download and host
 * replay */
int lt_bpt_get_timers(lt_ctx *ctx, double out[4]);
/* The grid prefilter of lt_bpt_junctions on the host, for tests (no context, no device; the expressions are the ones
 * the device compiles, limap_amd/csrc/lt_bpt.h).  lt_fn_bpt_grid_keys: the grid of one image from its lines
 * (grid_out, may be NULL: lo x, lo y, cell size) and the sort key of every point xy[2 n_pts] as a candidate of image
 * img: img << 40 | cell y << 20 | cell x.  lt_fn_bpt_close_pairs_host: what k_bpt_close_pairs finds over n candidates
 * with these keys (candidates into cell order, the 3 x 3 cell scan, the reference's distance test): n_pairs receives
 * the number of pairs, pairs_out the first min(cap, n_pairs) of them in ascending order as i << 32 | j, i < j.
 * LT_ERR_ARGUMENT for null pointers, non-finite coordinates or a NaN threshold. */
int lt_fn_bpt_grid_keys(int img, int64_t n_lines, const double *lines4, double th_merge, int64_t n_pts, const double *xy,
                        double grid_out[3], uint64_t *keys_out);
int lt_fn_bpt_close_pairs_host(int64_t n, const uint64_t *keys, const double *xy, double th_merge, int64_t cap,
                               uint64_t *pairs_out, int64_t *n_pairs);

/* ---- limap.line2d matchers that are pure linear algebra: L2D2Matcher (line2d/L2D2/matcher.py) and the top-k form of
 * NNEndpointsMatcher (line2d/endpoints/matcher.py:71-111), a whole scene in one call.
 * score(i, j) of two descriptors is the FP32 fmaf chain over the dimension in ascending order from +0.0f; the endpoints
 * line score is 0.5f * max(S[2i,2j] + S[2i+1,2j+1], S[2i,2j+1] + S[2i+1,2j]) in FP32 (the first sum when both are equal).
 * Columns rank by score descending, equal scores by ascending column.  topk > 0: min(topk, lines of the neighbour) rows
 * per line; topk == 0 (L2D2 only): mutual nearest neighbours, arg-max = first maximum. */
#define LT_MATCH_L2D2 0
#define LT_MATCH_ENDPOINTS 1
#define LT_MATCH_MAX_TOPK 64
#define LT_MATCH_MAX_DIM 256
typedef struct lt_match_config {
  int32_t kind;           /* LT_MATCH_L2D2: a descriptor row per line; LT_MATCH_ENDPOINTS: two rows (endpoints) per line */
  int32_t topk;           /* 0 .. LT_MATCH_MAX_TOPK; limap's default is 10 */
  int32_t desc_on_device; /* desc is device memory of the context's device, read in place on the context's stream */
  int32_t want_scores;    /* also download the FP32 scores of the returned rows (lt_match_get_scores) */
} lt_match_config;
/* Images as CSR over descriptor rows: image m owns rows desc_off[m] .. desc_off[m+1] of desc (row-major, dim floats per
 * row, FP32; for the endpoints kind rows 2 l and 2 l + 1 are the endpoints of line l -- the transpose of limap's
 * (256, 2 M) array).  Pairs as CSR over images: image m is matched against images pair_nb[pair_off[m] .. pair_off[m+1])
 * (indices into this call's images).  Rejected with LT_ERR_ARGUMENT before any matching launch: a value that is not
 * finite or above 2^57 in magnitude (no score can then overflow), dim not a multiple of 8 in [8, LT_MATCH_MAX_DIM],
 * topk outside [0, LT_MATCH_MAX_TOPK], topk == 0 with the endpoints kind, more than 65 535 lines in an image, an odd
 * endpoint count, a neighbour that is not an image.  The rows stay in the context: n_rows (may be NULL) receives their
 * number; lt_match_get copies out row_off[pairs + 1] and rows2[2 * n_rows] = (line, neighbour line) per row, pairs in
 * call order, within a pair by line, within a line best first; lt_match_get_scores the score of every row. */
int lt_match_scene(lt_ctx *ctx, int n_img, const int64_t *desc_off, const float *desc, int dim, const int64_t *pair_off,
                   const int32_t *pair_nb, const lt_match_config *cfg, int64_t *n_rows);
int lt_match_get(lt_ctx *ctx, int64_t *row_off, int32_t *rows2);
int lt_match_get_scores(lt_ctx *ctx, float *scores);
/* host ms of the last lt_match_scene: [0] validation and upload, [1] kernels, [2] download, [3] host row bookkeeping */
int lt_match_get_timers(lt_ctx *ctx, double out[4]);
/* The same semantics on the host, no context and no device (std::fmaf in a plain loop): exposed for tests.  desc1: n1
 * rows, desc2: n2 rows.  rows2 / scores (either may be NULL) need room for (lines of 1) * max(1, min(topk, lines of 2))
 * rows; n_rows receives the count. */
int lt_fn_match_pair_host(const float *desc1, int64_t n1, const float *desc2, int64_t n2, int dim,
                          const lt_match_config *cfg, int32_t *rows2, float *scores, int64_t *n_rows);

/* ---- the SOLD2 line matcher (line2d/SOLD2/model/line_matching.py: WunschLineMatcher; DESIGN section 17, "SOLD2").
 * An image is n lines of num_samples (S) point descriptors each: row l * S + s of its descriptor rows is sample s of line
 * l (the transpose of limap's (dim, S n) array), valid[l * S + s] != 0 says that the sample is real.  Point score
 * P[i, s, j, t]: the FP32 fmaf chain of the two descriptors in ascending k from +0.0f, -1.0f where either sample is not
 * valid.  Line score L[i, j] = ((mean over s of max_t P) + (mean over t of max_s P)) * 0.5f, every operation in FP32, the
 * means over the maxima that differ from -1.0f, their sums in the fixed tree ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7))
 * over 8 sample slots (absent terms +0.0f), a mean without any term -1.0f.  Lines rank by L descending, equal scores by
 * ascending line.  topk > 0: min(topk, lines of the neighbour) rows per line.  topk == 0: per line the
 * min(top_k_candidates, lines of the neighbour) best lines, ascending in that order, then the same with t reversed; the
 * Needleman-Wunsch value (FP64, gap 0.1f subtracted in FP32) of every block; the first maximum's candidate; the same from
 * the neighbour's side; (i, j) is a row iff each is the other's match. */
typedef struct lt_match_wunsch_config {
  int32_t topk;             /* 0 (mutual form) .. LT_MATCH_MAX_TOPK */
  int32_t num_samples;      /* S in [2, 8]; limap: 5 */
  int32_t top_k_candidates; /* 1 .. LT_MATCH_MAX_TOPK, used by the mutual form; limap: 10 */
  int32_t desc_on_device;   /* desc is device memory of the context's device (valid is always host memory) */
  int32_t want_scores;      /* also download L of every returned row (lt_match_get_scores) */
  int32_t reserved;         /* 0 */
} lt_match_wunsch_config;
/* Images as CSR over lines (line_off) and over descriptor rows (desc_off; image m must own S times as many rows as
 * lines), pairs as in lt_match_scene.  Rejected with LT_ERR_ARGUMENT before any matching launch: a value that is not
 * finite or above 2^57 in magnitude, dim not a multiple of 8 in [8, LT_MATCH_MAX_DIM], num_samples outside [2, 8], topk
 * outside [0, LT_MATCH_MAX_TOPK], top_k_candidates outside [1, LT_MATCH_MAX_TOPK], more than 65 535 lines in an image, a
 * descriptor count that is not S times the line count, a line without a valid sample, a neighbour that is not an image.
 * The rows are read with lt_match_get / lt_match_get_scores / lt_match_get_timers, exactly as after lt_match_scene. */
int lt_match_wunsch_scene(lt_ctx *ctx, int n_img, const int64_t *line_off, const int64_t *desc_off, const float *desc,
                          const uint8_t *valid, int dim, const int64_t *pair_off, const int32_t *pair_nb,
                          const lt_match_wunsch_config *cfg, int64_t *n_rows);
/* device ms (HIP events) of the last lt_match_wunsch_scene: [0] the line-score / top-k kernel, [1] the NW kernel (0 unless
 * topk == 0) */
int lt_match_wunsch_get_kernel_ms(lt_ctx *ctx, double out[2]);
/* The same semantics on the host, no context and no device: exposed for tests.  n1, n2: lines.  rows2 / scores (either may
 * be NULL) need room for n1 * max(1, min(topk, n2)) rows. */
int lt_fn_match_wunsch_pair_host(const float *desc1, const uint8_t *valid1, int64_t n1, const float *desc2,
                                 const uint8_t *valid2, int64_t n2, int dim, const lt_match_wunsch_config *cfg,
                                 int32_t *rows2, float *scores, int64_t *n_rows);
/* its intermediate values: point_scores (n1, n2, S, S) and line_scores (n1, n2), either may be NULL */
int lt_fn_match_wunsch_scores_host(const float *desc1, const uint8_t *valid1, int64_t n1, const float *desc2,
                                   const uint8_t *valid2, int64_t n2, int dim, int num_samples, float *point_scores,
                                   float *line_scores);
/* the Needleman-Wunsch value of one masked S x S block (row-major): out[0] as given, out[1] with its columns reversed */
int lt_fn_match_wunsch_nw_host(const float *block, int num_samples, double out[2]);

/* ---- the dense-warp line matcher (line2d/dense/matcher.py: BaseDenseLineMatcher behind get_warping_symmetric; DESIGN
 * section 17, "Dense").  A pair of images comes with a warp (hw, ww, 2) of normalised target coordinates and a certainty
 * map (hw, ww) in either direction, FP32, row-major.  Sample k of a line is r_k start + (1 - r_k) end with
 * r = linspace(0, 1, S); it is normalised by its image's shape, looked up bilinearly (align_corners = False, zero padding)
 * in warp and cert and unnormalised by the target image's shape.  A sample is good for a target line iff its certainty
 * exceeds sample_thresh and its projection on the line's unit direction lies strictly between those of the line's ends
 * (and nothing about it is non-finite).  Per (line, target line): overlap = count / S, weighted distance = the fmaf chain
 * over the good samples in sample order of |p . l| times 1 / count, 10000 where overlap < segment_percentage_th.  Both
 * directions combine as dists = overlap_12 > overlap_21 ? d_12 : d_21, 10000 where the smaller overlap is below
 * segment_percentage_th or the larger distance above pixel_th.  (i, j) is a row iff dists <= pixel_th and, unless
 * one_to_many, dists equals its row's minimum (every tie is kept).  Rows by line, then by neighbour line.  All FP32,
 * no contraction; the device equals lt_fn_match_dense_pair_host bit for bit. */
typedef struct lt_match_dense_config {
  int32_t n_samples;            /* S in [2, 64]; limap: 21 */
  int32_t one_to_many;          /* limap: 0 */
  float segment_percentage_th;  /* limap: 0.2 */
  float pixel_th;               /* limap: 10 */
  float sample_thresh;          /* the dense matcher's get_sample_thresh() */
  int32_t on_device;            /* warp and cert pointers are device memory of the context's device, read in place */
  int32_t want_scores;          /* also download dists of every row (lt_match_get_scores) */
  int32_t want_dirs;            /* also keep d_12, overlap_12, d_21, overlap_21, dists of every entry (..._get_dirs) */
} lt_match_dense_config;
/* Images as CSR over lines (line_off; lines: 4 floats sx, sy, ex, ey per line, host memory), shapes[2 m], [2 m + 1] =
 * height and width of image m.  Pair q matches image pair_img[2 q] (lines i) against pair_img[2 q + 1] (lines j);
 * warp[2 q], cert[2 q] take image 1 to image 2, warp[2 q + 1], cert[2 q + 1] back; dims[4 (2 q + d) ..] = warp height,
 * warp width, cert height, cert width of direction d.  Rejected with LT_ERR_ARGUMENT before any launch, the message
 * naming the argument: n_samples outside [2, 64], a NaN threshold, a warp side below 1 or above 16384, cert and warp
 * shapes that differ, a shape that is not positive, more than 65 535 lines in an image, a pair that names no image.
 * The rows are read with lt_match_get / lt_match_get_scores / lt_match_get_timers, as after lt_match_scene. */
int lt_match_dense_pairs(lt_ctx *ctx, int n_img, const int64_t *line_off, const float *lines, const int32_t *shapes,
                         int64_t n_pairs, const int32_t *pair_img, const float *const *warp, const float *const *cert,
                         const int32_t *dims, const lt_match_dense_config *cfg, int64_t *n_rows);
/* device ms (HIP events) of the last lt_match_dense_pairs: k_dense_warp, k_dense_pairs, k_dense_select (both passes and
 * the prefix sum between them) */
int lt_match_dense_get_kernel_ms(lt_ctx *ctx, double out[3]);
/* after a call with want_dirs: per entry (pairs behind each other, entry i * n2 + j of a pair) d_12, overlap_12 and, as
 * seen from (i, j), d_21 and overlap_21, and dists; any pointer may be NULL */
int lt_match_dense_get_dirs(lt_ctx *ctx, float *d12, float *o12, float *d21, float *o21, float *dists);
/* The same semantics on the host, no context and no device: exposed for tests.  rows2 / scores (either may be NULL)
 * need room for n1 * n2 rows. */
int lt_fn_match_dense_pair_host(const float *lines1, int64_t n1, const int32_t *shape1, const float *lines2, int64_t n2,
                                const int32_t *shape2, const float *warp12, const float *cert12, const int32_t *dims12,
                                const float *warp21, const float *cert21, const int32_t *dims21,
                                const lt_match_dense_config *cfg, int32_t *rows2, float *scores, int64_t *n_rows);
/* its matrices: d12, o12 and dists are (n1, n2), d21 and o21 (n2, n1) as upstream returns them; any may be NULL */
int lt_fn_match_dense_dists_host(const float *lines1, int64_t n1, const int32_t *shape1, const float *lines2, int64_t n2,
                                 const int32_t *shape2, const float *warp12, const float *cert12, const int32_t *dims12,
                                 const float *warp21, const float *cert21, const int32_t *dims21,
                                 const lt_match_dense_config *cfg, float *d12, float *o12, float *d21, float *o21,
                                 float *dists);

/* ---- limap.vplib: the JLinkage vanishing-point detector (vplib/JLinkage/JLinkage.cc, vplib/base_vp_detector.cc) for a
 * batch of images per call.  Images as CSR over lines, as for lt_bpt_*.  limap's own code around
 * the two calls into its J-Linkage third party is reproduced bit for bit: the `length() < min_length` filter, endpoints
 * rounded to FP32, the guard `valid lines < 2 * max(min_num_supports, 10)` (all labels -1), per cluster the size test and
 * count_valid_supports_2d, the compaction of the surviving clusters in label order, fitVP (the third right singular
 * vector of the rows Line2d::coords(), normalised) and AssociateVPs.  The two calls themselves -- upstream samples
 * 5000 hypotheses at random -- are this project's deterministic definition: hypothesis m is the cross product of the
 * lines (a, b) a counter-based generator draws from (seed, m) and the number of valid lines; a line prefers the
 * hypotheses within inlier_threshold by Tardif's measure; clusters merge by the greatest Jaccard ratio of their
 * preference sets, ties to the smallest (i, j), until no two sets intersect.  Labels therefore do not equal those of a
 * particular upstream run.  th_perp_supports is carried for as_dict only: upstream's count_valid_supports_2d reads the
 * base class's default-constructed configuration, so 3.0 is used whatever the value (section 18).
 * LT_ERR_ARGUMENT before any launch: non-finite coordinates, a NaN threshold, min_num_supports outside [3, 2^20] (fitVP
 * is undefined below three lines), num_hypotheses outside [1, 2^20]; after the clustering: a support line on which a
 * check of InfiniteLine2d throws upstream. */
typedef struct lt_vp_config {
  double min_length;        /* 40, pixels */
  double inlier_threshold;  /* 1.0, pixels */
  double th_perp_supports;  /* 3.0, pixels (see above) */
  int32_t min_num_supports; /* 5 */
  int32_t num_hypotheses;   /* 5000 (JLinkage.cc:44); not a key of upstream's configuration */
  uint64_t seed;            /* 0; not a key of upstream's configuration */
} lt_vp_config;
void lt_vp_config_default(lt_vp_config *cfg);
/* The result stays in the context: n_vps (may be NULL) receives the number of vanishing points of all images; lt_vp_get
 * copies out (any pointer may be NULL) labels[line_off[n_img]] (VPResult::labels, -1: none), vp_off[n_img + 1],
 * vps[3 n_vps] and clusters[line_off[n_img]]: the cluster of every line before the filters (the third party's Labels;
 * -1 for a line the length filter or the guard dropped). */
int lt_vp_detect(lt_ctx *ctx, int n_img, const int64_t *line_off, const double *lines, const lt_vp_config *cfg,
                 int64_t *n_vps);
int lt_vp_get(lt_ctx *ctx, int32_t *labels, int64_t *vp_off, double *vps, int32_t *clusters);
/* of the last lt_vp_detect: host ms of [0] upload, length filter and tables, [1] kernels, [2] download, [3] host tail;
 * device ms (HIP events) of [4] the preference kernel, [5] the clustering kernel */
int lt_vp_get_timers(lt_ctx *ctx, double out[6]);
/* The whole detector on the host, no context and no device: the same expressions and the same order, images spread
 * over n_threads OpenMP threads (0: the default).  vps has room for vps_cap vanishing points (sum over the images of
 * lines / 3 always suffices); LT_ERR_ARGUMENT when it does not. */
int lt_fn_vp_detect_host(int n_img, const int64_t *line_off, const double *lines, const lt_vp_config *cfg, int n_threads,
                         int32_t *labels, int64_t *vp_off, double *vps, int64_t vps_cap, int32_t *clusters);
/* The clustering alone on the host, for tests: pref is n rows of n_words 64-bit words (the preference sets), roots[n]
 * receives the id of the cluster every row ends in (the smallest row index of the cluster). */
int lt_fn_vp_cluster_host(int64_t n, int64_t n_words, const uint64_t *pref, int32_t *roots);
/* Its device twin, for tests: the clustering kernel of lt_vp_detect alone (same launch, same buffers of the context) on
 * preference sets the caller supplies, a batch of images per call.  pref is row_off[n_img] rows of n_words words in the
 * layout above, image m owning the rows [row_off[m], row_off[m + 1]); roots[k] is the cluster row k ends in, as an index
 * within its own image.  Images of 0 or 1 rows are legal.  LT_ERR_ARGUMENT before any launch: null pointers where rows
 * exist, offsets that do not start at 0 or decrease, n_words outside [1, 2^14], more than 2^32 words in the call. */
int lt_vp_cluster_sets(lt_ctx *ctx, int n_img, const int64_t *row_off, int64_t n_words, const uint64_t *pref,
                       int32_t *roots);

/* ---- limap.optimize: the geometric refinement of line tracks with constant cameras -- step [E] of
 * limap.runners.line_triangulation (:208-219, optimize/hybrid_bundle_adjustment/hybrid_bundle_adjustment.cc) and the
 * geometric terms of limap.optimize.line_refinement.  With constant intrinsics and poses every
 * track is its own problem: a Pluecker line in the orthonormal form (uvec in S^3, wvec in S^1), two residuals per
 * supporting 2D segment (optimize/line_refinement/cost_functions.h:106-127), ScaledLoss(CauchyLoss(0.25), length / 30)
 * per support.  limap's own code -- MinimalInfiniteLine3d, GetInfiniteLine, ComputeLineWeights, the residual, the
 * residual order (sorted image ids, list order within an image), GetLineSegmentFromInfiniteLine3d over the track's
 * line3d_list, applied to every track, constant ones included -- is restated; the minimiser (a Levenberg-Marquardt
 * iteration per track on the device) is this project's definition: refined lines are minimisers of upstream's cost, not
 * the iterates of a particular Ceres run.
 * LT_ERR_ARGUMENT before any launch, where upstream CHECK-fails or indexes out of range: a track line of zero length, a
 * track without supports, num_outliers_aggregator outside [0, 2 K - 1] for a track of K supports, an image id that is
 * not in the collection; also non-finite input, geometric_alpha outside [0, 700], max_num_iterations < 0. */
typedef struct lt_refine_config {
  double geometric_alpha;          /* 10.0 */
  int32_t min_num_images;          /* 4: a track seen in fewer images is held constant */
  int32_t num_outliers_aggregator; /* 2: the num_outliers of GetOutputLineTracks; the entry points below cut with it */
  int32_t num_outliers_aggregate;  /* 2: RefinementConfig's key (GetLine3d); carried, the Python layer selects */
  int32_t max_num_iterations;      /* 100 */
  int32_t constant_line;           /* 0 */
  int32_t pad_;
} lt_refine_config;
void lt_refine_config_default(lt_refine_config *cfg);
/* Termination codes: 0 max_num_iterations, 1 radius below 1e-32, 2 zero gradient, 3 non-positive or non-finite pivot,
 * 4 non-positive or non-finite model decrease, 5 held constant, 6 evaluation failed at the initial point (only with
 * the heatmap term, below).
 * Tracks as CSR: track n owns the supports [off[n], off[n + 1]) in the order of its lists; line6 = start, end of
 * track.line; img = image_id_list; line2d4 = line2d_list; line3d6 = start, end of line3d_list.  Cameras: n_img ids (any
 * order, distinct) with kvec4 (fx, fy, cx, cy), qvec4 (w, x, y, z), tvec3.  The result stays in the context. */
int lt_refine_arrays(lt_ctx *ctx, int n_img, const int32_t *img_ids, const double *kvec4, const double *qvec4,
                     const double *tvec3, int64_t n_tracks, const double *line6, const int64_t *off, const int32_t *img,
                     const double *line2d4, const double *line3d6, const lt_refine_config *cfg);
/* The same on a track set, with the cameras the context holds on the device since lt_init: every track's line becomes
 * the re-cut segment of its refined line (uncertainty -1, like a fresh Line3d). */
int lt_refine_tracks(lt_ctx *ctx, lt_trackset *ts, const lt_refine_config *cfg);
/* of the last lt_refine_arrays / lt_refine_tracks (any pointer may be NULL): per track params6 = uvec (w, x, y, z),
 * wvec; seg6 = start, end; cost2 = initial, final cost (1/2 sum rho); iterations; termination code */
int64_t lt_refine_num(lt_ctx *ctx);
int lt_refine_get(lt_ctx *ctx, double *params6, double *seg6, double *cost2, int32_t *iters, int32_t *codes);
/* host ms of [0] validation, tables and upload, [1] the kernels, [2] download; device ms (HIP events) of [3] k_refine_lm */
int lt_refine_get_timers(lt_ctx *ctx, double out[4]);
/* The whole step on the host, no context and no device: the same inline functions and the same reduction order, tracks
 * spread over n_threads OpenMP threads (0: the default).  Outputs as lt_refine_get. */
int lt_fn_refine_host(int n_img, const int32_t *img_ids, const double *kvec4, const double *qvec4, const double *tvec3,
                      int64_t n_tracks, const double *line6, const int64_t *off, const int32_t *img,
                      const double *line2d4, const double *line3d6, const lt_refine_config *cfg, int n_threads,
                      double *params6, double *seg6, double *cost2, int32_t *iters, int32_t *codes);
/* the message of the calling thread's last lt_fn_refine_host that returned LT_ERR_ARGUMENT ("" after a success) */
const char *lt_fn_refine_host_error(void);
/* GetLineSegmentFromInfiniteLine3d alone (host): the segment of the line params6 over the K 3D supports line3d6 with
 * num_outliers in [0, 2 K - 1]; what a second num_outliers on solved tracks needs, without a new solve */
int lt_fn_refine_cut(int64_t K, const double *line3d6, const double params6[6], int num_outliers, double seg6[6]);
/* For tests: one track of K supports (cam11 = kvec | qvec | tvec per support, in residual order) at the given minimal
 * parameters: residuals[2 K], cost, g[4] and H[16] of the linearisation (any pointer may be NULL). */
int lt_fn_refine_eval(int64_t K, const double *cam11, const double *line2d4, const double params6[6], double alpha,
                      double *residuals, double *cost, double g[4], double H[16]);
/* For tests: out[k] = lt_exp(x[k]) (which = 0, x in [0, 700]) or lt_log(x[k]) (which = 1, x >= 1), the module's own
 * exponential and logarithm; MinimalInfiniteLine3d of a segment; GetInfiniteLine (d, m) of minimal parameters. */
int lt_fn_refine_explog(int which, int64_t n, const double *x, double *out);
int lt_fn_refine_minimal(const double line6[6], double params6[6]);
int lt_fn_refine_infinite(const double params6[6], double dm6[6]);
/* For tests: the minimisers' damped step (lm_step of lt_lm.h) on the sums acc of a linearisation with n = 4 or 6
 * unknowns (n (n + 1) / 2 entries of the upper triangle of H by rows, then g) at the radius mu.  Returns 0 with the step
 * dl[n] and the model decrease *md, or the termination code 3 (bad pivot; dl and *md NaN) or 4 (bad model; dl and *md
 * as computed); -1 on another n or a NULL pointer. */
int lt_fn_lm_step(int n, const double *acc, double mu, double *dl, double *md);

/* ---- the VP and the heatmap term of limap.optimize.line_refinement (runners/refinement.py with
 * cfgs/refinement/default.yaml; refine.cc:87-126,315-360).  Per support of a track, after its
 * geometric block: a VP block where its VPResult labels the line -- one residual, the sine between the line's direction
 * in the camera frame and the direction of the vanishing point, TrivialLoss scaled by (length / 30) vp_multiplier -- and a
 * heatmap block of n_samples_heatmap residuals 1 - f(xy_j), xy_j the intersection of the projected line with sample line
 * j of the support, f the bilinear interpolation of the image's heatmap with upstream's forward-difference derivatives,
 * HuberLoss(0.001) scaled by (length / 30) heatmap_multiplier / (n_samples_heatmap / 10.0).
 * Evaluation failure: a sample whose intersection has |p_homo[2]| < 1e-12 (or is not a number) fails; a cost evaluation
 * with a failed sample is +inf, so the step is rejected and the radius shrinks; at the initial point the track ends with
 * termination code 6, its parameters unchanged, its segment re-cut.
 * Texels are binary16 or binary32 in memory and widen to FP64 exactly. */
#define LT_TEXEL_F16 0
#define LT_TEXEL_F32 1
typedef struct lt_refine_terms {
  int32_t use_geometric;      /* 1 */
  int32_t use_vp;             /* 0 */
  int32_t use_heatmap;        /* 0 */
  int32_t n_samples_heatmap;  /* 10 */
  double vp_multiplier;       /* 1.0 */
  double sample_range_min;    /* 0.05 */
  double sample_range_max;    /* 0.95 */
  double heatmap_multiplier;  /* 1.0 */
  int32_t texel_type;         /* LT_TEXEL_F16: the type of the heatmaps the call reads */
  int32_t pad_;
} lt_refine_terms;
void lt_refine_terms_default(lt_refine_terms *terms);
/* The scene's heatmaps, uploaded once and kept in the context until they are set again or cleared: n images with
 * distinct ids, h[i] x w[i] texels of texel_type each, row-major without padding, at the host pointers data[i].  The
 * call returns after the copy. */
int lt_refine_set_heatmaps(lt_ctx *ctx, int n, const int32_t *img_ids, const int32_t *h, const int32_t *w,
                           const void *const *data, int texel_type);
int lt_refine_clear_heatmaps(lt_ctx *ctx);
/* Counts the calls that changed the context's heatmaps (a set that passed its argument checks, whether its copy then
 * succeeded or not, and every clear): a caller that remembers the value after its own lt_refine_set_heatmaps knows that
 * its heatmaps are still the resident ones while the value stands. */
int64_t lt_refine_heatmaps_generation(lt_ctx *ctx);
/* lt_refine_arrays with the terms.  vp_flag[s] != 0 where support s (the caller's order, like img) has a vanishing
 * point, vp3 its homogeneous image coordinates (read only there; both may be NULL without use_vp); view_hw: (h, w) of
 * every camera row, or NULL, an entry <= 0 meaning that the view carries no size.  With neither use_vp nor use_heatmap
 * the call is lt_refine_arrays: the same launches, the same bits.  The getters and timers are lt_refine_arrays'; [3] is
 * the device time of k_refine_lm_terms.
 * LT_ERR_ARGUMENT before any launch, besides lt_refine_arrays' cases: no term enabled; n_samples_heatmap outside
 * [2, 1024]; a multiplier, a sample range or a flagged vanishing point that is not finite; with use_heatmap a supporting image
 * without a heatmap in the context, heatmaps of another texel type than the terms', a heatmap whose size is not its
 * view's, a 2D support of zero length. */
int lt_refine_arrays_terms(lt_ctx *ctx, int n_img, const int32_t *img_ids, const double *kvec4, const double *qvec4,
                           const double *tvec3, int64_t n_tracks, const double *line6, const int64_t *off,
                           const int32_t *img, const double *line2d4, const double *line3d6, const lt_refine_config *cfg,
                           const lt_refine_terms *terms, const int32_t *vp_flag, const double *vp3,
                           const int32_t *view_hw);
/* lt_fn_refine_host with the terms: the heatmaps are the caller's n_hm host images (as lt_refine_set_heatmaps takes
 * them, of terms->texel_type).  Errors through lt_fn_refine_host_error. */
int lt_fn_refine_host_terms(int n_img, const int32_t *img_ids, const double *kvec4, const double *qvec4, const double *tvec3,
                            int64_t n_tracks, const double *line6, const int64_t *off, const int32_t *img,
                            const double *line2d4, const double *line3d6, const lt_refine_config *cfg,
                            const lt_refine_terms *terms, const int32_t *vp_flag, const double *vp3, const int32_t *view_hw,
                            int n_hm, const int32_t *hm_ids, const int32_t *hm_h, const int32_t *hm_w,
                            const void *const *hm_data, int n_threads, double *params6, double *seg6, double *cost2,
                            int32_t *iters, int32_t *codes);
/* For tests: lt_fn_refine_eval with the terms; support k reads the heatmap hm_data[k] of hm_h[k] x hm_w[k] texels.
 * residuals[K (3 + n)], n = n_samples_heatmap with use_heatmap and 0 without: per support 2 geometric, 1 VP and n heatmap
 * residuals, NaN where the block is absent; *failed = 1 where a sample fails (then the cost is +inf). */
int lt_fn_refine_eval_terms(int64_t K, const double *cam11, const double *line2d4, const double params6[6], double alpha,
                            const lt_refine_terms *terms, const int32_t *vp_flag, const double *vp3, const int32_t *hm_h,
                            const int32_t *hm_w, const void *const *hm_data, double *residuals, int32_t *failed,
                            double *cost, double g[4], double H[16]);

/* ---- the feature-consistency term of limap.optimize.line_refinement (use_feature; refine.cc:363-543,
 * pixel_cost_functions.h:198-400, linetrack.cc:353-454).  Samples are taken once per track on
 * the host from its initial line (ComputeFConsistencySamples); every (sample, target image) is one block of 128
 * residuals f_tgt[c](xy_tgt) - f_ref[c](xy_ref) under ScaledLoss(CauchyLoss(0.25), fconsis_multiplier /
 * ((n_kept / 100.0) (n_targets / 5.0))), added after the track's geometric, VP and heatmap blocks, by sample, then by
 * target.  use_ref_descriptor is not built.  The sample range is the terms' (sample_range_min / max); with use_heatmap
 * the heatmaps and the features have one texel type.  A failed intersection follows the heatmap term's rule. */
typedef struct lt_refine_feature {
  int32_t use_feature;        /* 1 */
  int32_t n_samples_feature;  /* 100 */
  double fconsis_multiplier;  /* 1.0 */
  int32_t channels;           /* 128, the only count built */
  int32_t texel_type;         /* LT_TEXEL_F16 */
} lt_refine_feature;
void lt_refine_feature_default(lt_refine_feature *feat);
/* The grid an image of a track is sampled on: h x w x 128 texels, row-major, channels interleaved, aligned to two
 * texels; local_xy = R (xy - tvec) (R row-major), sampled bilinearly at (row = local y, col = local x) with rows and
 * columns clamped.  A patch of limap_amd.features carries its R and tvec; a whole map is the identity.  on_device: data
 * is a device address and is read in place. */
typedef struct lt_refine_grid {
  const void *data;
  int32_t h, w;
  double R[4];
  double tvec[2];
  int32_t on_device;
  int32_t pad_;
} lt_refine_grid;
/* The scene's feature maps (the map form), kept in the context like the heatmaps: n images with distinct ids,
 * h[i] x w[i] x 128 texels each; on_device != 0: data[i] are device addresses, kept and read in place (the caller keeps
 * them alive), otherwise host pointers that are uploaded before the call returns.  The generation counts sets and
 * clears like lt_refine_heatmaps_generation. */
int lt_refine_set_feature_maps(lt_ctx *ctx, int n, const int32_t *img_ids, const int32_t *h, const int32_t *w,
                               const void *const *data, int texel_type, int on_device);
int lt_refine_clear_feature_maps(lt_ctx *ctx);
int64_t lt_refine_feature_maps_generation(lt_ctx *ctx);
/* lt_refine_arrays_terms with the feature term (any of the four terms may be the only one).  grids: one per (track,
 * image of the track in ascending id), track after track, n_grids in all -- the patch form; NULL with n_grids 0: the
 * map form, every image reads its map of the context.  Host grids are uploaded for the call, device grids are read in
 * place.  Results through lt_refine_get; timer [3] is the device time of k_refine_lm_feat.
 * LT_ERR_ARGUMENT besides lt_refine_arrays_terms' cases: channels other than 128, n_samples_feature outside [2, 4096],
 * a grid count that is not the tracks', an empty or misaligned grid, a track of more than 64 images, an image without
 * a map, maps of another texel type or size than the configuration's or the view's. */
int lt_refine_arrays_feature(lt_ctx *ctx, int n_img, const int32_t *img_ids, const double *kvec4, const double *qvec4,
                             const double *tvec3, int64_t n_tracks, const double *line6, const int64_t *off,
                             const int32_t *img, const double *line2d4, const double *line3d6, const lt_refine_config *cfg,
                             const lt_refine_terms *terms, const int32_t *vp_flag, const double *vp3,
                             const int32_t *view_hw, const lt_refine_feature *feat, int64_t n_grids,
                             const lt_refine_grid *grids);
/* The host twin: lt_fn_refine_host_terms with the feature term; grids are host grids (a map: the identity transform).
 * Errors through lt_fn_refine_host_error. */
int lt_fn_refine_host_feature(int n_img, const int32_t *img_ids, const double *kvec4, const double *qvec4, const double *tvec3,
                              int64_t n_tracks, const double *line6, const int64_t *off, const int32_t *img,
                              const double *line2d4, const double *line3d6, const lt_refine_config *cfg,
                              const lt_refine_terms *terms, const int32_t *vp_flag, const double *vp3, const int32_t *view_hw,
                              int n_hm, const int32_t *hm_ids, const int32_t *hm_h, const int32_t *hm_w,
                              const void *const *hm_data, const lt_refine_feature *feat, int64_t n_grids,
                              const lt_refine_grid *grids, int n_threads, double *params6, double *seg6, double *cost2,
                              int32_t *iters, int32_t *codes);
/* For tests: one track (K supports in the caller's order) at params6 (NULL: the minimal parameters of line6), the
 * geometric term as terms->use_geometric says, no VP or heatmap term.  The kept samples in order: *n_kept of them,
 * sample_ref[i] the reference image id, sample_line[3 i ..] the sample line, sample_ntgt[i] its number of targets,
 * targets the target image ids of all samples one after the other; the blocks in (sample, target) order: *n_blocks of
 * them, residuals[128 b ..] and failed[b].  cap_samples / cap_blocks: what the outputs hold.  cost, g, H of all enabled
 * terms (cost +inf where a block fails).  Any output may be NULL. */
int lt_fn_refine_eval_feature(int n_img, const int32_t *img_ids, const double *kvec4, const double *qvec4, const double *tvec3,
                              const double line6[6], int64_t K, const int32_t *img, const double *line2d4, double alpha,
                              const lt_refine_terms *terms, const lt_refine_feature *feat, int64_t n_grids,
                              const lt_refine_grid *grids, const double *params6, int64_t cap_samples, int64_t cap_blocks,
                              int32_t *n_kept, int32_t *sample_ref, double *sample_line, int32_t *sample_ntgt,
                              int32_t *targets, int32_t *n_blocks, double *residuals, int32_t *failed, double *cost,
                              double g[4], double H[16]);

/* ---- limap.pointsfm: the visual neighbours of every image and the robust ranges of the point cloud -- step [A] of
 * limap.runners.line_triangulation, `compute_metainfos` (pointsfm/functions.py:20-55) over SfmModel
 * (pointsfm/sfm_model.{h,cc}, colmap::mvs::Model).  DESIGN.md section 21 is the definition: shared points and the 75th
 * percentile of the triangulation angles per image pair, the gate by min_triangulation_angle, the score of `kind`
 * (0 overlap: GetMaxOverlapImages, 1 IoU: GetMaxIoUImages, 2 Dice: GetMaxDiceCoeffImages), the first num_images partners
 * by (score descending, image index ascending).
 * The model as arrays: image m (an index, 0 .. n_img - 1; n_img <= 65535) has R9 (row-major) and T3 as the float32
 * values upstream stores; point p has xyz (float32) and the track track_img[track_off[p] .. track_off[p + 1]) of image
 * indices (an index may repeat).  LT_ERR_ARGUMENT before any launch for: an index outside [0, n_img) (message starts
 * with "unknown": upstream's std::out_of_range), non-finite values, offsets that do not start at 0 or decrease, kind
 * outside 0 .. 2, num_images < 0; and for a model whose E = sum L (L - 1) / 2 pair instances (track length L) need more
 * key memory than the budget of 32 GiB (16 E bytes and the sort's scratch): the message names E and the budget.
 * The result stays in the context; n_neighbors / n_pairs (may be NULL) receive the sizes lt_sfm_get /
 * lt_sfm_get_pairs need. */
int lt_sfm_neighbors(lt_ctx *ctx, int n_img, const float *R9, const float *T3, int64_t n_pts, const float *xyz,
                     const int64_t *track_off, const int32_t *track_img, int kind, int64_t num_images,
                     double min_triangulation_angle, int64_t *n_neighbors, int64_t *n_pairs);
/* of the last lt_sfm_neighbors (any pointer may be NULL): nb_off[n_img + 1], nb = neighbour image indices in order */
int lt_sfm_get(lt_ctx *ctx, int64_t *nb_off, int32_t *nb);
/* the image pairs that share a point, ascending in (i, j), i < j: ij[2 k], ij[2 k + 1]; shared = ComputeSharedPoints;
 * angle = the percentile angle (radians, float32) the gate tests */
int lt_sfm_get_pairs(lt_ctx *ctx, int32_t *ij, int32_t *shared, float *angle);
/* of the last lt_sfm_neighbors: host ms of [0] validation, tables and upload, [1] the device stage, [2] download; device
 * ms (HIP events) of [3] k_sfm_pairs, [4] the key sort, [5] k_sfm_segments, [6] partner lists, selection and
 * compaction; [7] launches of k_sfm_segments (2: the first had too little room for the pair records) */
int lt_sfm_get_timers(lt_ctx *ctx, double out[8]);
/* The same definition on the host, no context and no device: the same inline functions, OpenMP over n_threads threads
 * (0: the default).  The result stays with the calling thread until its next call: lt_fn_sfm_host_get copies it out
 * (arrays as lt_sfm_get and lt_sfm_get_pairs), lt_fn_sfm_host_error is the message of the thread's last
 * lt_fn_sfm_neighbors_host / lt_fn_sfm_ranges that returned LT_ERR_ARGUMENT ("" after a success). */
int lt_fn_sfm_neighbors_host(int n_img, const float *R9, const float *T3, int64_t n_pts, const float *xyz,
                             const int64_t *track_off, const int32_t *track_img, int kind, int64_t num_images,
                             double min_triangulation_angle, int n_threads, int64_t *n_neighbors, int64_t *n_pairs);
int lt_fn_sfm_host_get(int64_t *nb_off, int32_t *nb, int32_t *ij, int32_t *shared, float *angle);
const char *lt_fn_sfm_host_error(void);
/* SfmModel::ComputeRanges(range_robust, k_stretch): per axis, in float32 as get_robust_range writes it.  Host work.
 * LT_ERR_ARGUMENT where upstream is undefined: no points, an index float(n) * float(p) outside [0, n), a non-finite
 * coordinate. */
int lt_fn_sfm_ranges(int64_t n_pts, const float *xyz, double range_lo, double range_hi, double k_stretch, double lo[3],
                     double hi[3]);

/* ---- limap.undistortion: images and points of distorted COLMAP cameras brought to pinhole cameras -- the step
 * limap.runners.functions.undistort_images puts in front of line_triangulation (undistortion/undistort.{cc,py} over
 * COLMAP's UndistortImage).  DESIGN.md section 22 is the definition: the camera models, the iterative undistortion
 * (Newton, central differences, at most 100 updates), the warp with bilinear interpolation, the in-range test on the
 * doubles and the rounding rule.  Everything is FP64; the device and the host path agree bit for bit. */
typedef struct lt_undist_camera {
  int32_t model;      /* COLMAP model id: 0 SIMPLE_PINHOLE, 1 PINHOLE, 2 SIMPLE_RADIAL, 3 RADIAL, 4 OPENCV, 6 FULL_OPENCV */
  int32_t n_params;   /* 3, 4, 4, 5, 8, 12 */
  double params[12];  /* in COLMAP's order */
} lt_undist_camera;
typedef struct lt_undist_image {
  const void *src;    /* uint8, rows of src_w * channels bytes, src_stride bytes apart */
  void *dst;          /* uint8, rows of dst_w * channels bytes, dst_stride bytes apart */
  int64_t src_stride, dst_stride;
  int32_t src_w, src_h, dst_w, dst_h;
  int32_t channels;   /* 1, 3 or 4 */
  int32_t src_cam, dst_cam; /* rows of the camera table: the distorted camera, the pinhole camera of the target */
  int32_t on_device;  /* src and dst are device memory, read and written in place on the context's stream */
} lt_undist_image;
/* One launch set over a whole batch of images, which may differ in size, channels and camera.  Host images go through
 * one upload and one download; a batch is either all host or all device.  Returns after the stream has finished.
 * LT_ERR_ARGUMENT before any launch for: a model that is not built or a wrong parameter count, non-finite parameters, a
 * focal length that is 0, a size below 1, a channel count outside {1, 3, 4}, a stride shorter than a row, a camera
 * index outside the table, a target camera that is not a pinhole model, a mixed batch. */
int lt_undist_warp(lt_ctx *ctx, int n_cam, const lt_undist_camera *cams, int n_img, const lt_undist_image *imgs);
/* UndistortPoint for n points (host arrays): point i goes through CamFromImg of camera cam_src[i] and ImgFromCam of camera
 * cam_dst[i].  out_xy[2 n]; status[n] is 0, or 1 with the point the canonical quiet NaN (a singular Jacobian, an
 * overflow); iters[n] is the number of Newton updates (0 for a pinhole source). */
int lt_undist_points(lt_ctx *ctx, int n_cam, const lt_undist_camera *cams, int64_t n, const double *xy,
                     const int32_t *cam_src, const int32_t *cam_dst, double *out_xy, int32_t *status, int32_t *iters);
/* of the last lt_undist_warp / lt_undist_points: host ms of [0] validation, packing and upload, [2] download and
 * unpacking; [1] device ms (HIP events) of the kernel; [3] its work units (runs of 4 target pixels) or points */
int lt_undist_get_timers(lt_ctx *ctx, double out[4]);
/* the yardstick of the warp's measurement (tools/time_undist.py): device ms of a copy kernel that moves `bytes` bytes,
 * 16 per lane, between two buffers of the context */
int lt_undist_copy_yardstick(lt_ctx *ctx, int64_t bytes, double *ms);
/* The same definition on the host, no context and no device: the same inline functions, OpenMP over n_threads threads
 * (0: the default).  lt_fn_undist_host_error is the message of the calling thread's last lt_fn_undist_* call that
 * returned LT_ERR_ARGUMENT ("" after a success). */
int lt_fn_undist_warp_host(int n_cam, const lt_undist_camera *cams, int n_img, const lt_undist_image *imgs,
                           int n_threads);
int lt_fn_undist_points_host(int n_cam, const lt_undist_camera *cams, int64_t n, const double *xy,
                             const int32_t *cam_src, const int32_t *cam_dst, double *out_xy, int32_t *status,
                             int32_t *iters, int n_threads);
const char *lt_fn_undist_host_error(void);
/* The scale rule of UndistortCamera for a camera of size w x h with principal point (cx, cy): ext = the extremes of
 * the undistorted border {left min x, left max x, right min x, right max x, top min y, top max y, bottom min y, bottom
 * max y}; out = {new_w, new_h, new_cx, new_cy}.  LT_ERR_ARGUMENT for COLMAP's range checks of the options and for a
 * border that is not finite. */
int lt_fn_undist_scale(int32_t w, int32_t h, double cx, double cy, const double ext[8], double blank_pixels,
                       double min_scale, double max_scale, double out[4]);

/* ---- limap_amd.line2d: SOLD2 line detection from junctions and line heatmaps -- LineSegmentDetectionModule.detect of
 * line2d/SOLD2/model/line_detection.py (heatmap refinement, candidate suppression, sampling of all junction pairs, the
 * inlier test, junction refinement) for a whole scene in one set of launches, and the descriptor sampling of
 * WunschLineMatcher.compute_descriptors.  DESIGN.md section 23 is the definition.  FP32 throughout; thresholds are
 * rounded to FP32 before they are compared, as torch does. */
typedef struct lt_sold2_config {
  double detect_thresh, inlier_thresh, lambda_radius, nms_dist_tolerance;
  double refine_ratio, refine_valid_thresh, refine_overlap_ratio;
  int32_t num_samples;               /* 2 .. 64 */
  int32_t sampling_method;           /* 0 local_max, 1 bilinear */
  int32_t max_local_patch_radius;    /* 0 .. 4 */
  int32_t use_candidate_suppression;
  int32_t use_heatmap_refinement;
  int32_t refine_mode;               /* 0 global, 1 local */
  int32_t refine_num_blocks;         /* 1 .. 32 (local) */
  int32_t use_junction_refinement;
  int32_t num_perturbs;              /* odd, 1 .. 9 */
  int32_t lds_window_floats;         /* junction refinement: largest heatmap window staged in LDS; < 0: the default */
  const float *sampler;              /* num_samples floats: torch.linspace(0, 1, num_samples) */
  const float *perturb_vec;          /* num_perturbs floats: the reference's torch.arange */
} lt_sold2_config;
/* one image: junctions (n_junc, 2) in (h, w) order and the heatmap (H, W) with heat_stride floats per row.  on_device
 * != 0: both are device addresses, read in place.  cand_in / det_in (host form only, n_junc x n_junc bytes, the upper
 * triangle is read): stand in for the result of the suppression / of the detection, so that a stage can be fed the
 * output of the stage before it. */
typedef struct lt_sold2_image {
  const float *junctions;
  const float *heatmap;
  int64_t heat_stride;
  int32_t n_junc, H, W, on_device;
  const uint8_t *cand_in;
  const uint8_t *det_in;
} lt_sold2_image;
int lt_sold2_detect_scene(lt_ctx *ctx, const lt_sold2_config *cfg, int n_img, const lt_sold2_image *imgs);
/* the same definition on the host: no context, no device; OpenMP over n_threads threads (0: the default).  The result
 * is kept per calling thread and read with the getters below with ctx == NULL. */
int lt_fn_sold2_detect_host(const lt_sold2_config *cfg, int n_img, const lt_sold2_image *imgs, int n_threads);
const char *lt_fn_sold2_host_error(void);
/* pieces of the host form, for tests.  Samples of the given junction pairs of one image on its INPUT heatmap: pos
 * (n_pairs, num_samples, 2) the clamped sample positions (h, w), values (n_pairs, num_samples) the local-max or
 * bilinear sample values.  Block scales of the heatmap refinement: scales (nb, nb), negative where a block's maximum
 * is not above valid_thresh, bounds4 (nb, 4) = row begin, row end, column begin, column end of block index a. */
int lt_fn_sold2_samples_host(const lt_sold2_config *cfg, const lt_sold2_image *img, int64_t n_pairs,
                             const int32_t *pairs2, float *pos, float *values);
int lt_fn_sold2_block_scales_host(const lt_sold2_config *cfg, const lt_sold2_image *img, float *scales,
                                  int32_t *bounds4);
/* Getters of the last detection (ctx == NULL: of the calling thread's last host detection).  counts[n_img]: detected
 * segments per image.  Segments of image img in candidate order: segs4 = (h1, w1, h2, w2) after junction refinement
 * (the junctions themselves without it), pairs2 = the junction indexes i < j, perturb = index of the chosen
 * perturbation in the reference's meshgrid order (-1 without refinement). */
int lt_sold2_get_counts(lt_ctx *ctx, int64_t *counts);
int lt_sold2_get_segments(lt_ctx *ctx, int img, float *segs4, int32_t *pairs2, int32_t *perturb);
/* stages of image img, any may be NULL: heat (H, W) the refined heatmap (the input without refinement), cand / det
 * (n_junc, n_junc) bytes: upper triangle = candidates after suppression / detected pairs */
int lt_sold2_get_stages(lt_ctx *ctx, int img, float *heat, uint8_t *cand, uint8_t *det);
/* device ms of the last lt_sold2_detect_scene: [0] block scales, [1] refined pixels, [2] suppression, [3] scoring,
 * [4] compaction, [5] junction refinement, [6] all kernels, [7] whole call on the host clock */
int lt_sold2_get_kernel_ms(lt_ctx *ctx, double out[8]);
/* compute_descriptors, "regular" mode, after sample_line_points: per image a channel-last descriptor map (Hd, Wd, C),
 * n_points points (h, w) in image coordinates (host memory) and the output (C, n_points): bilinear grid_sample with
 * zero padding and align_corners = False, then L2 normalisation per point.  on_device != 0: map and out are device
 * addresses.  out_ms (may be NULL): device ms of the kernel. */
typedef struct lt_sold2_desc_image {
  const float *map;
  const float *points;
  float *out;
  int64_t n_points;
  int32_t Hd, Wd, C, grid_size, on_device, pad_;
} lt_sold2_desc_image;
int lt_sold2_descinfo_scene(lt_ctx *ctx, int n_img, const lt_sold2_desc_image *imgs, double *out_ms);
int lt_fn_sold2_descinfo_host(int n_img, const lt_sold2_desc_image *imgs, int n_threads);

/* ---- limap_amd.features: line patches resampled from dense feature maps -- limap.features' LinePatchExtractor
 * (features/line_patch_extractor.cc, featurepatch.h, extract_line_patches.py) and the patch side of
 * optimize/extract_track_patches_s2dnet.py.  DESIGN.md section 24 is the definition: the geometry of a patch, the
 * global coordinate of a texel, the clamped bilinear sample, the single rounding to the output type and
 * GetLine2DRange.  Everything is FP64; the device and the host path agree bit for bit. */
#define LT_PATCH_F16 0
#define LT_PATCH_F32 1
#define LT_PATCH_F64 2
/* a feature map of h x w texels of c channels: channel ch of texel (r, x) at ptr + r * row_stride + x * pix_stride +
 * ch * chan_stride elements (strides of either sign); dtype LT_PATCH_F16 / _F32 / _F64, widened to double exactly.
 * on_device != 0: ptr is device memory, read in place on the context's stream. */
typedef struct lt_feature_map {
  const void *ptr;
  int64_t h, w, c, row_stride, pix_stride, chan_stride;
  int32_t dtype;
  int32_t on_device;
} lt_feature_map;
typedef struct lt_patch_config {
  double k_stretch;   /* 1.0 */
  int32_t t_stretch;  /* 10 */
  int32_t range_perp; /* 20 (cfgs/refinement/default.yaml passes 16) */
} lt_patch_config;
void lt_patch_config_default(lt_patch_config *cfg);
/* The patches of n lines (lines4 = x1, y1, x2, y2 each) of one feature map: patch i is an array (h_i, range_perp + 1,
 * c) of out_dtype, and the patches lie behind one another in line order.  out in host memory (out_on_device == 0): the
 * packed output goes there through chunks of whole patches of at most max_chunk_bytes each (at least one patch; <= 0:
 * 2^30), one launch per chunk.  out in device memory (out_on_device != 0, on a 16-byte boundary): one launch writes it in
 * place.  out == NULL: one launch, and the packed output stays in the context until its next patch call (the two
 * getters below).  Returns after the stream has finished.  LT_ERR_ARGUMENT before any work for: a line
 * coordinate that is not finite, range_perp < 0 or above 4096, t_stretch < 0, a k_stretch that is not finite, h, w or c
 * below 1, an unknown dtype, a null map, a patch of more than 2^20 rows or whose geometry is not finite. */
int lt_patch_extract(lt_ctx *ctx, const lt_patch_config *cfg, const lt_feature_map *map, int64_t n, const double *lines4,
                     int32_t out_dtype, void *out, int32_t out_on_device, int64_t max_chunk_bytes);
/* of the last lt_patch_extract, any may be NULL: R4[4 n] = perp.x, perp.y, direc.x, direc.y (PatchInfo::R, row-major),
 * tvec2[2 n] the corner, h[n] the rows, off[n + 1] the first element of every patch in the packed output */
int lt_patch_get_geometry(lt_ctx *ctx, double *R4, double *tvec2, int32_t *h, int64_t *off);
/* the packed output a call with out == NULL left on the device: its address and size, or a host copy */
int lt_patch_get_device_out(lt_ctx *ctx, void **ptr, int64_t *bytes);
int lt_patch_get_out(lt_ctx *ctx, void *dst);
/* of the last lt_patch_extract: host ms of [0] validation, tables and the map's upload, [2] the downloads; [1] device ms
 * (HIP events) of the kernel over all chunks; [3] patches, [4] chunks, [5] 1 when the vector form of the kernel ran and 0
 * for the scalar form, [6] workgroups, [7] bytes of the packed output */
int lt_patch_get_timers(lt_ctx *ctx, double out[8]);
/* the yardstick of the measurement (tools/time_patch.py): device ms of a copy kernel that moves `bytes` bytes, 16 per
 * lane, between two buffers of the context */
int lt_patch_copy_yardstick(lt_ctx *ctx, int64_t bytes, double *ms);
/* The same definition on the host, no context and no device: the same inline functions, OpenMP over n_threads threads
 * (0: the default); out is the whole packed output.  lt_fn_patch_geometry is the geometry alone (c: the channels the
 * offsets count).  lt_fn_patch_host_error is the message of the calling thread's last lt_fn_patch_* call that returned
 * LT_ERR_ARGUMENT ("" after a success). */
int lt_fn_patch_extract_host(const lt_patch_config *cfg, const lt_feature_map *map, int64_t n, const double *lines4,
                             int32_t out_dtype, void *out, int n_threads);
int lt_fn_patch_geometry(const lt_patch_config *cfg, int64_t c, int64_t n, const double *lines4, double *R4,
                         double *tvec2, int32_t *h, int64_t *off);
const char *lt_fn_patch_host_error(void);
/* GetLine2DRange for n_pairs (track, image) pairs.  Tracks as CSR arrays: line6[6 n_tracks] the 3D lines, sup_off[n_tracks
 * + 1] their supports, sup_img the supports' image ids, sup_seg4 their 2D lines.  Pair i: track pair_track[i], image id
 * pair_img[i], camera pair_cam11[11 i ..] = kvec, qvec, tvec.  range4[4 n_pairs]; status[n_pairs]: 0, 1 when the track has
 * no support in that image, 2 when an endpoint of the 3D line is not in front of the camera or a coordinate of the
 * range is not finite. */
int lt_fn_patch_ranges(int64_t n_tracks, const double *line6, const int64_t *sup_off, const int32_t *sup_img,
                       const double *sup_seg4, int64_t n_pairs, const int32_t *pair_track, const int32_t *pair_img,
                       const double *pair_cam11, double *range4, int32_t *status);

/* ---- limap.optimize.hybrid_localization: point-line pose refinement (LineLocEngine, JointLocEngine, solve_jointloc;
 * DESIGN.md section 25).  Every problem refines one camera pose (qvec, tvec; kvec = fx, fy, cx, cy of a PINHOLE camera
 * is constant) from its 2D-3D line and point correspondences: residual blocks in JointLocEngine::AddResiduals' order
 * (hybrid_localization.cc:91-134) -- per 3D line its 2D segments with ScaledLoss(loss, weight_line length / sum_lengths),
 * then the points with ScaledLoss(loss, weight_point) -- and the cost 1/2 sum rho_k(|r_k|^2).  All problems of a call
 * run in one launch, one wave per problem.  The minimiser is the Levenberg-Marquardt definition of section 19 with six
 * unknowns: refined poses are minimisers of upstream's cost, not the iterates of a Ceres run. */
#define LT_LOC_COST_MIDPOINT2 0       /* LineLocCostFunction, upstream's order */
#define LT_LOC_COST_MIDPOINT_ANGLE3 1
#define LT_LOC_COST_PERPENDICULAR2 2
#define LT_LOC_COST_PERPENDICULAR4 3
#define LT_LOC_COST_LINELINE2 4
#define LT_LOC_COST_PLANELINE2 5
#define LT_LOC_WEIGHT_NONE 0          /* LineLocCostFunctionWeight, upstream's order */
#define LT_LOC_WEIGHT_COSINE 1
#define LT_LOC_WEIGHT_LINE3DPP 2      /* rejected: it needs an arccosine */
#define LT_LOC_WEIGHT_LENGTH 3
#define LT_LOC_WEIGHT_INVLENGTH 4
#define LT_LOC_LOSS_TRIVIAL 0
#define LT_LOC_LOSS_HUBER 1
#define LT_LOC_LOSS_SOFTLONE 2
#define LT_LOC_LOSS_CAUCHY 3
typedef struct lt_loc_config {
  int32_t cost_function;       /* LT_LOC_COST_*; the 3D forms switch the points to their 3D distance too */
  int32_t weight_function;     /* LT_LOC_WEIGHT_* */
  int32_t loss;                /* LT_LOC_LOSS_* */
  int32_t max_num_iterations;  /* 100 */
  double loss_a;               /* the parameter of Huber, SoftLOne and Cauchy; > 0 */
  double weight_line, weight_point;
} lt_loc_config;
void lt_loc_config_default(lt_loc_config *cfg);
/* n_prob problems as CSR arrays.  Problem n: kvec4[4 n ..], the initial pose qvec4[4 n ..] (normalised once, as
 * CameraPose does) and tvec3[3 n ..]; its 3D lines line_off[n] .. line_off[n + 1] of line3d6 (start, end); 3D line l is
 * observed by the 2D segments seg_off[l] .. seg_off[l + 1] of seg4 (x1 y1 x2 y2); its points pt_off[n] .. pt_off[n + 1]
 * of p3d3 / p2d2.  LineLocEngine is the call without points and weight_line = 1.
 * LT_ERR_ARGUMENT before any launch: non-finite input, a zero focal length or quaternion, a 3D line of zero length
 * (upstream divides its direction by sqrt(1e-8) and constrains against a zero direction), a 3D line whose segments have
 * sum_lengths == 0 (0 / 0 upstream), LT_LOC_WEIGHT_LINE3DPP, a loss parameter <= 0, negative weights or iterations. */
int lt_loc_solve(lt_ctx *ctx, int64_t n_prob, const double *kvec4, const double *qvec4, const double *tvec3,
                 const int64_t *line_off, const double *line3d6, const int64_t *seg_off, const double *seg4,
                 const int64_t *pt_off, const double *p3d3, const double *p2d2, const lt_loc_config *cfg);
/* of the last lt_loc_solve (any pointer may be NULL): per problem the refined pose, cost2 = the cost at the initial and
 * at the final pose (GetInitialCost / GetFinalCost are sqrt(cost / num_res)), the number of residuals, the iterations
 * and the termination code: 0 max_num_iterations, 1 radius, 2 zero gradient (IsSolutionUsable for 0-2), 3 pivot,
 * 4 model decrease, 6 the cost at the initial pose is not finite, 7 no residual block (Solve() returns false); 6 and 7
 * keep the pose */
int64_t lt_loc_num(lt_ctx *ctx);
int lt_loc_get(lt_ctx *ctx, double *qvec4, double *tvec3, double *cost2, int32_t *num_res, int32_t *iters, int32_t *codes);
/* host ms of [0] validation, tables and upload, [1] the kernel, [2] download; device ms (HIP events) of [3] k_loc_lm */
int lt_loc_get_timers(lt_ctx *ctx, double out[4]);
/* The same definition on the host, no context and no device: the same inline functions, the reductions in the device's
 * order, bit-identical results; OpenMP over n_threads threads (0: the default).  Outputs as lt_loc_get. */
int lt_fn_loc_host(int64_t n_prob, const double *kvec4, const double *qvec4, const double *tvec3, const int64_t *line_off,
                   const double *line3d6, const int64_t *seg_off, const double *seg4, const int64_t *pt_off,
                   const double *p3d3, const double *p2d2, const lt_loc_config *cfg, int n_threads, double *qvec4_out,
                   double *tvec3_out, double *cost2, int32_t *num_res, int32_t *iters, int32_t *codes);
/* the message of the calling thread's last lt_fn_loc_* call that returned LT_ERR_ARGUMENT ("" after a success) */
const char *lt_fn_loc_host_error(void);
/* For tests: one problem at a given pose -- residuals (4 slots per block in block order, NaN where a block has fewer),
 * the cost, the gradient g = sum rho' J^T r and H = sum rho' J^T J over the six local directions (rotation, translation) */
int lt_fn_loc_eval(const double kvec4[4], const double qvec4[4], const double tvec3[3], int64_t n_lines,
                   const double *line3d6, const int64_t *seg_off, const double *seg4, int64_t n_points, const double *p3d3,
                   const double *p2d2, const lt_loc_config *cfg, double *residuals, double *cost, double g[6], double H[36]);
/* For tests: lt_fn_loc_eval at the quaternion as given -- an iterate of the solve, which normalises its input once and
 * then evaluates the retracted quaternions as they are -- not normalised once more. */
int lt_fn_loc_eval_at(const double kvec4[4], const double qvec4[4], const double tvec3[3], int64_t n_lines,
                      const double *line3d6, const int64_t *seg_off, const double *seg4, int64_t n_points,
                      const double *p3d3, const double *p2d2, const lt_loc_config *cfg, double *residuals, double *cost,
                      double g[6], double H[36]);
/* Pose scoring: JointPoseEstimator::EvaluateModelOnPoint (estimators/absolute_pose/joint_pose_estimator.cc:176-251) for
 * n_poses hypotheses x N = n_pts + n_seg correspondences of one camera in one launch, the points first.  2D segment s
 * observes 3D line l3d_ids[s].  A cell is the squared norm of the correspondence's residuals (lines with ENoneWeight),
 * or DBL_MAX where a cheirality test fails: a NaN pose; a point below cheirality_min_depth; for a line a ray through a
 * 2D endpoint within 1 degree of the 3D line, an unprojection below cheirality_min_depth, or less than
 * cheirality_overlap_pixels between the projections of the 2D endpoints onto the reprojected segment.  With want_msac
 * each pose also gets the MSAC score sum_i min(r2_i, squared_thresholds[type]) weights[type] and the counts of
 * r2_i < squared_thresholds[type] per type (0 points, 1 lines), pl_absolute_pose_hybrid_ransac.h:338-393.
 * LT_ERR_ARGUMENT before any launch: LT_LOC_COST_MIDPOINT_ANGLE3 (upstream throws), non-finite correspondences or
 * intrinsics (poses may be non-finite), a 3D line of zero length that a segment refers to, an l3d_id out of range. */
typedef struct lt_loc_score_config {
  int32_t cost_function;  /* LT_LOC_COST_* */
  int32_t want_msac;
  double cheirality_min_depth, cheirality_overlap_pixels;  /* 0.0, 10.0 */
  double squared_thresholds[2], weights[2];
} lt_loc_score_config;
int lt_loc_score(lt_ctx *ctx, const double kvec4[4], int64_t n_l3d, const double *line3d6, int64_t n_seg,
                 const int32_t *l3d_ids, const double *seg4, int64_t n_pts, const double *p3d3, const double *p2d2,
                 int64_t n_poses, const double *qvec4, const double *tvec3, const lt_loc_score_config *cfg);
/* of the last lt_loc_score: the sizes; table[n_poses N] row-major by pose, scores[n_poses], inliers2[2 n_poses] (any
 * may be NULL; the last two are an LT_ERR_STATE where the call did not ask for them) */
int lt_loc_score_size(lt_ctx *ctx, int64_t *n_poses, int64_t *n_corr);
int lt_loc_score_get(lt_ctx *ctx, double *table, double *scores, int32_t *inliers2);
/* host ms of [0] validation, table and upload, [1] the kernel, [2] download; device ms (HIP events) of [3] k_loc_score */
int lt_loc_score_get_timers(lt_ctx *ctx, double out[4]);
/* The same definition on the host, bit-identical results (the score summed in the device's order); errors through
 * lt_fn_loc_host_error */
int lt_fn_loc_score_host(const double kvec4[4], int64_t n_l3d, const double *line3d6, int64_t n_seg, const int32_t *l3d_ids,
                         const double *seg4, int64_t n_pts, const double *p3d3, const double *p2d2, int64_t n_poses,
                         const double *qvec4, const double *tvec3, const lt_loc_score_config *cfg, int n_threads,
                         double *table, double *scores, int32_t *inliers2);
/* CameraPose(R, T)'s quaternion: Eigen's Quaternion(Matrix3) of the row-major R9, (w, x, y, z) */
int lt_fn_loc_qvec_from_R(const double R9[9], double qvec4[4]);

/* ---- Minimal absolute-pose solvers from points and lines: the solvers
 * JointPoseEstimator::MinimalSolver calls (p3p, p2p1ll, p1p2ll, p3ll) as one problem with one core.  A sample of kind k
 * is 3 - k points (unit bearing x, world point X) and k lines (unit image-line normal l, a point C and the unit direction
 * V of the 3D line), built as joint_pose_estimator.cc:80-110 builds them.  The arithmetic is this project's definition
 * (PoseLib's is not restated): poses are solutions of the sample's six constraints with positive point depths, at most 8,
 * in ascending order of z / w of the quaternion, which is normalised with w > 0.  A degenerate sample returns fewer
 * poses, or none; no pose holds a NaN. ---- */
#define LT_EST_P3P 0
#define LT_EST_P2P1LL 1
#define LT_EST_P1P2LL 2
#define LT_EST_P3LL 3
#define LT_EST_MAX_SOLUTIONS 8
/* n samples of one kind on the device, one lane per sample.  xs, Xs: n x (3 - kind) x 3; ls, Cs, Vs: n x kind x 3 (an
 * array of a kind without such data may be NULL).  Non-finite input is LT_ERR_ARGUMENT. */
int lt_est_minimal(lt_ctx *ctx, int kind, int64_t n, const double *xs, const double *Xs, const double *ls, const double *Cs,
                   const double *Vs);
int64_t lt_est_minimal_num(lt_ctx *ctx);
/* of the last lt_est_minimal (any pointer may be NULL): poses[n][8][7] (qvec w x y z, tvec; rows past the count are 0),
 * counts[n] */
int lt_est_minimal_get(lt_ctx *ctx, double *poses56, int32_t *counts);
/* host ms of [0] validation, table and upload, [1] the kernel, [2] download; device ms (HIP events) of [3] k_est_minimal */
int lt_est_minimal_get_timers(lt_ctx *ctx, double out[4]);
/* The same inline functions in plain C++: bit-identical results; OpenMP over n_threads threads (0: the default).
 * Errors through lt_fn_est_host_error. */
int lt_fn_est_minimal_host(int kind, int64_t n, const double *xs, const double *Xs, const double *ls, const double *Cs,
                           const double *Vs, int n_threads, double *poses56, int32_t *counts);
const char *lt_fn_est_host_error(void);

/* ---- The hybrid LO-MSAC around these solvers: PointLineAbsolutePoseHybridRansac::EstimateModel
 * (estimators/absolute_pose/pl_absolute_pose_hybrid_ransac.h:63-249) for Q independent queries in one set of launches.
 * limap's control flow, score, thresholds, weights, cheirality tests and refinements (section 25) are restated; the
 * minimal solvers, the sampler, the shuffles and NumRequiredIterations are this project's seedable definition, which the
 * device and the host twin compute bit-identically.  The loop advances in rounds of round_size iterations whose solver
 * types are drawn under the probabilities frozen at the round's start; everything else is upstream's sequential
 * semantics, replayed in iteration order on the device.  Poses are those of a hybrid LO-MSAC, not the iterates of a
 * RansacLib run. ---- */
typedef struct lt_est_config {
  double squared_inlier_thresholds[2]; /* 1, 1: points, lines */
  double data_type_weights[2];         /* 1, 1 */
  double success_probability;          /* 0.9999 */
  double threshold_multiplier;         /* sqrt(2) */
  double cheirality_min_depth;         /* 0 */
  double cheirality_overlap_pixels;    /* 10 */
  uint64_t random_seed;                /* 0 */
  uint32_t min_num_iterations;         /* 100 */
  uint32_t max_num_iterations;         /* 10000 */
  uint32_t max_num_iterations_per_solver; /* 10000 */
  uint32_t lo_starting_iterations;     /* 50 */
  int32_t num_lo_steps;                /* 10 */
  int32_t num_lsq_iterations;          /* 4 */
  int32_t min_sample_multiplicator;    /* 7 */
  int32_t non_min_sample_multiplier;   /* 3 */
  int32_t final_least_squares;         /* 0 */
  int32_t round_size;                  /* 64: iterations per round; 1 is upstream's control flow exactly */
  int32_t solver_flags[4];             /* 1 1 1 1: p3p, p2p1ll, p1p2ll, p3ll */
  int32_t poll_interval;               /* 4: rounds enqueued between two looks at the count of finished queries */
  lt_loc_config loc;                   /* LeastSquares: cost function, weight, loss, block weights, iteration cap */
} lt_est_config;
void lt_est_config_default(lt_est_config *cfg);
#define LT_EST_TRACE_DOUBLES 12
/* Q queries as CSR: per query its camera and input pose (returned where no solver can run), points [pt_off[q],
 * pt_off[q + 1]), 3D lines [l3d_off[q], ..) and 2D segments [seg_off[q], ..) with l3d_ids[s] the index of the segment's
 * 3D line within its query.  trace_cap > 0 keeps up to that many records of the loop's decisions per query. */
int lt_est_solve(lt_ctx *ctx, int64_t n_query, const double *kvec4, const double *qvec4, const double *tvec3,
                 const int64_t *pt_off, const double *p3d3, const double *p2d2, const int64_t *l3d_off, const double *line3d6,
                 const int64_t *seg_off, const int32_t *l3d_ids, const double *seg4, const lt_est_config *cfg,
                 int64_t trace_cap);
/* of the last lt_est_solve (any pointer may be NULL): pose7[Q][7] (qvec, tvec); dstats3[Q][3] = best_model_score and
 * the two inlier ratios; istats12[Q][12] = num_iterations_total, num_iterations_per_solver[4], best_num_inliers,
 * best_solver_type, number_lo_iterations, inlier counts (points, lines), VerifyData (1: the loop ran), trace records;
 * inliers[pt_off[Q] + seg_off[Q]]: at pt_off[q] + seg_off[q] the query's inlier points, then its inlier segments, as
 * indices within their type; trace[Q][trace_cap][12] */
int lt_est_get(lt_ctx *ctx, double *pose7, double *dstats3, int32_t *istats12, int32_t *inliers, double *trace);
/* host ms of [0] validation, tables and upload, [1] the rounds, [2] download; [3] rounds enqueued; device ms (HIP
 * events, summed over the polls) of [4] all rounds */
int lt_est_get_timers(lt_ctx *ctx, double out[8]);
/* The same definition in plain C++ from the same inline functions: bit-identical results; OpenMP over the queries */
int lt_fn_est_host(int64_t n_query, const double *kvec4, const double *qvec4, const double *tvec3, const int64_t *pt_off,
                   const double *p3d3, const double *p2d2, const int64_t *l3d_off, const double *line3d6,
                   const int64_t *seg_off, const int32_t *l3d_ids, const double *seg4, const lt_est_config *cfg,
                   int64_t trace_cap, int host_threads, double *pose7, double *dstats3, int32_t *istats12, int32_t *inliers,
                   double *trace);
/* the definition's arithmetic, for tests: NumRequiredIterations, the logarithm, the frozen solver probabilities
 * (prob4 from ratios2, iterations per solver and priors) and the priors of a query's data counts */
uint32_t lt_fn_est_num_required(const double ratios2[2], double success_probability, int solver, uint32_t min_it, uint32_t max_it);
double lt_fn_est_log(double x);
int lt_fn_est_probabilities(const double ratios2[2], const uint32_t its4[4], const int32_t flags4[4], int32_t n_pts,
                            int32_t n_lines, uint32_t min_it, double prior4[4], double prob4[4]);

/* ---- 2D-3D line matching for localization: optimize/hybrid_localization/functions.py as
 * runners/hybrid_localization.py:277-340 runs it, for Q queries in one set of launches.  A pair (query line i, database
 * line j) of a task (query q, retrieved database image d) survives if compute_epipolar_IoU(l_i, view_q, l_j, view_d) >
 * IoU_threshold (strict: a NaN fails) and db_track[j] != -1.  mode 0 (all_pairs, the "epipolar" matcher) tests every
 * (i, j) of every task; mode 1 (listed) takes the pairs per task from pairs2 and applies only the track lookup; mode 2
 * (listed_filtered, epipolar_filter) puts the listed pairs through the IoU test too.  Rows come in upstream's order:
 * query lines in the order of their first survivor (task position, then i * n_d + j or the position in the list), a
 * line's rows in that order too, duplicates kept.  filter 1 Perpendicular, 2 Midpoint, 3 Midpoint_Perpendicular is
 * reprojection_filter_matches_2to3: at most one (line, best track) per line, the strict minimum of the loss over the
 * line's distinct tracks in ascending id order. ---- */
typedef struct lt_l23_config {
  int32_t mode;         /* 0 */
  int32_t filter;       /* 0: none */
  double IoU_threshold; /* 0.2 (cfgs/localization/default.yaml) */
  double dist_thres;    /* 10 (the function's default; the runner passes 2) */
  double sine_thres;    /* 0.4 */
  double angle_scale;   /* 1 */
} lt_l23_config;
void lt_l23_config_default(lt_l23_config *cfg);
/* The scene as flat arrays.  Database images: db_cam11[n_db][11] (kvec, qvec, tvec), their segments [db_seg_off[d],
 * db_seg_off[d + 1]) of db_seg4 and db_track (the track of each segment, -1: none).  Queries: q_cam11 (the coarse pose),
 * q_seg_off, q_seg4.  Tasks: query q owns [task_off[q], task_off[q + 1]) of task_db, the database image rows in
 * retrieval order (a row may repeat, a query may have none).  Listed modes: task t owns [pair_off[t], pair_off[t + 1])
 * of pairs2 (query line, database line); NULL in mode 0.  track6[n_tracks][6]: start and end of every track's line
 * (read only with a filter).  Refused with LT_ERR_ARGUMENT and the offending index: offsets that do not ascend,
 * non-finite cameras, segments or tracks, an image row or a line index out of range, a track id >= n_tracks or < -1,
 * any count above 2^31 - 1, more than 2^31 - 1 (task, query line) units or rows in one call. */
typedef struct lt_l23_input {
  int64_t n_db;
  const double *db_cam11;
  const int64_t *db_seg_off;
  const double *db_seg4;
  const int32_t *db_track;
  int64_t n_query;
  const double *q_cam11;
  const int64_t *q_seg_off;
  const double *q_seg4;
  const int64_t *task_off;
  const int32_t *task_db;
  const int64_t *pair_off;
  const int32_t *pairs2;
  int64_t n_tracks;
  const double *track6;
} lt_l23_input;
int lt_l23_match(lt_ctx *ctx, const lt_l23_input *in, const lt_l23_config *cfg);
/* rows of the last lt_l23_match */
int64_t lt_l23_num(lt_ctx *ctx);
/* of the last lt_l23_match (any pointer may be NULL): q_off[Q + 1], rows2[rows][2] = (query line, track id),
 * loss[rows] = the winning loss (with a filter; zeros without) */
int lt_l23_get(lt_ctx *ctx, int64_t *q_off, int32_t *rows2, double *loss);
/* host ms of [0] validation and upload, [1] the launches, [2] download; device ms (HIP events) of [3] the records,
 * [4] the count pass or the listed pairs' flags, [5] the scan, [6] the fill, [7] the filter and its compaction */
int lt_l23_get_timers(lt_ctx *ctx, double out[8]);
/* The same definition in plain C++ from the same inline functions: bit-identical results; OpenMP over queries and
 * lines.  The result stays with the calling thread: *n_rows says how many rows lt_fn_l23_host_get then copies. */
int lt_fn_l23_host(const lt_l23_input *in, const lt_l23_config *cfg, int host_threads, int64_t *n_rows);
int lt_fn_l23_host_get(int64_t *q_off, int32_t *rows2, double *loss);
const char *lt_fn_l23_host_error(void);

/* ---- Bundle adjustment with free poses, points and lines: limap.optimize's
 * solve_hybrid_bundle_adjustment / solve_point_bundle_adjustment, HybridBAEngine with constant intrinsics.  Every image
 * that carries a residual block is a parameter (quaternion and translation), every point track (3 unknowns) and every
 * line track (4, section 19's chart) unless its switch holds it constant.  limap's residuals, weights, losses, block
 * order and segment cut are restated; the minimiser is this project's definition: one Levenberg-Marquardt loop over all
 * unknowns with one radius, its linear step by a Schur complement over the images and a dense Cholesky factorisation in
 * a fixed order.  The results are a stationary point of upstream's cost reached from the input, not the iterates of a
 * Ceres run; upstream does not fix the gauge, so compare costs and reprojections, never parameters. ---- */
#define LT_BA_MAX_IMAGES 128 /* images that carry residuals; above it LT_ERR_ARGUMENT before any launch */
typedef struct lt_ba_config {
  double geometric_alpha;          /* 10 */
  double lw_point;                 /* 0.1; <= 0 adds no point block */
  int32_t min_num_images;          /* 4: a line track seen in fewer images keeps its line and still constrains its cameras */
  int32_t num_outliers_aggregator; /* 2: GetOutputLineTracks' cut */
  int32_t max_num_iterations;      /* 100; an attempt counts whether accepted or not */
  int32_t constant_intrinsics;     /* 1; 0 is LT_ERR_ARGUMENT (free intrinsics are not built) */
  int32_t constant_principal_point; /* accepted, no effect with constant intrinsics */
  int32_t constant_pose;           /* 0; 1: the tracks separate -- point tracks only (line tracks are lt_refine_arrays'), every
                                      one its own 3-unknown problem under section 19's loop with its own radius */
  int32_t constant_point, constant_line;
  int32_t poll_interval;           /* attempts enqueued between two reads of the status record; 0: the default (8).
                                      The result does not depend on it */
  int32_t kernel_timers;           /* 1: HIP events around every kernel of every attempt (the interval becomes 1) */
} lt_ba_config;
void lt_ba_config_default(lt_ba_config *cfg);
int lt_ba_max_images(void);   /* LT_BA_MAX_IMAGES */
int lt_ba_poll_default(void);
/* Cameras as lt_refine_arrays takes them.  Point track n: pt3[3 n ..] and its observations pt_off[n] .. pt_off[n + 1] of
 * pt_img (image ids) / pt_xy2, in list order; tracks in ascending id.  Line tracks as lt_refine_arrays: line6, ln_off,
 * ln_img, l2d4, l3d6.  LT_ERR_ARGUMENT before any launch: constant_intrinsics = 0, constant_pose = 1 with line tracks, an image id that is
 * not in the collection, non-finite input, a track line of zero length, a line track without supports, a zero focal
 * length or quaternion of an image with residuals, more than LT_BA_MAX_IMAGES images with residuals. */
int lt_ba_arrays(lt_ctx *ctx, int n_img, const int32_t *img_ids, const double *kvec4, const double *qvec4,
                 const double *tvec3, int64_t n_pt, const double *pt3, const int64_t *pt_off, const int32_t *pt_img,
                 const double *pt_xy2, int64_t n_ln, const double *line6, const int64_t *ln_off, const int32_t *ln_img,
                 const double *l2d4, const double *l3d6, const lt_ba_config *cfg);
/* of the last lt_ba_arrays (any pointer may be NULL): the poses of all n_img images in input order (an image without a
 * residual block keeps its input bit for bit, the others carry a unit quaternion), the points, the lines' minimal
 * parameters (uvec, wvec) and segments, cost2 = the cost at the initial and at the final point, the iterations and
 * the termination code of the solve: 0 max_num_iterations, 1 radius, 2 zero gradient, 6 the cost at the initial point
 * is not finite, 7 no residual block (Solve() returns false); 6 and 7 change nothing.  With constant_pose = 1 the
 * poses are the input's, cost2 sums the tracks' costs in ascending order, iters is the largest count and code the largest
 * of the free tracks' section 19 codes (0-4, 6; 5 where every track is constant) */
int lt_ba_get(lt_ctx *ctx, double *qvec4, double *tvec3, double *pt3, double *params6, double *seg6, double *cost2,
              int32_t *iters, int32_t *code);
/* host ms of [0] validation, tables and upload, [1] the loop, [2] download; [3] attempts enqueued; with kernel_timers the
 * device ms of [4] k_ba_linearize [5] k_ba_blocks [6] k_ba_images [7] k_ba_damp [8] k_ba_schur [9] k_ba_chol
 * [10] k_ba_backsub [11] k_ba_cost [12] k_ba_decide, summed over the attempts */
int lt_ba_get_timers(lt_ctx *ctx, double out[16]);
/* The same definition on the host, no context and no device: bit-identical results for every n_threads (0: default) */
int lt_fn_ba_host(int n_img, const int32_t *img_ids, const double *kvec4, const double *qvec4, const double *tvec3,
                  int64_t n_pt, const double *pt3, const int64_t *pt_off, const int32_t *pt_img, const double *pt_xy2,
                  int64_t n_ln, const double *line6, const int64_t *ln_off, const int32_t *ln_img, const double *l2d4,
                  const double *l3d6, const lt_ba_config *cfg, int n_threads, double *qvec4_out, double *tvec3_out,
                  double *pt3_out, double *params6, double *seg6, double *cost2, int32_t *iters, int32_t *code);
const char *lt_fn_ba_host_error(void);
/* For tests: the problem at its initial point (params6_in, when given, replaces the lines' minimal parameters).
 * dims4 = images with residuals, blocks, unknowns, structures; with every other output NULL only dims4 is written.
 * The unknowns: (dq, dt) of the images with residuals in ascending id, then the free structures in order (3 / 4 each).
 * blk_info3 per block: image row, structure, first unknown of the structure (-1: constant).  residuals: 2 per block;
 * cost; g = sum rho' J^T r; H = sum rho' J^T J (dense, unknowns x unknowns); step: the Schur route's step at radius mu
 * (NaN where a factorisation fails). */
int lt_fn_ba_eval(int n_img, const int32_t *img_ids, const double *kvec4, const double *qvec4, const double *tvec3,
                  int64_t n_pt, const double *pt3, const int64_t *pt_off, const int32_t *pt_img, const double *pt_xy2,
                  int64_t n_ln, const double *line6, const int64_t *ln_off, const int32_t *ln_img, const double *l2d4,
                  const double *l3d6, const lt_ba_config *cfg, const double *params6_in, int64_t *dims4, int32_t *blk_info3,
                  double *residuals, double *cost, double *g, double *H, double mu, double *step);
/* For tests: point track `track` of a constant_pose = 1 problem at the point p3, as the separated solve sums it over
 * the track's blocks: the cost, g[4] and H[16] of section 19's sums (the fourth direction is the literal zero). */
int lt_fn_ba_point_eval(int n_img, const int32_t *img_ids, const double *kvec4, const double *qvec4, const double *tvec3,
                        int64_t n_pt, const double *pt3, const int64_t *pt_off, const int32_t *pt_img, const double *pt_xy2,
                        int64_t n_ln, const double *line6, const int64_t *ln_off, const int32_t *ln_img, const double *l2d4,
                        const double *l3d6, const lt_ba_config *cfg, int64_t track, const double p3[3], double *cost,
                        double g[4], double H[16]);
/* For tests: the minimisers' loop (lm_loop of lt_lm.h over the additive point chart) from the point p3 with the cost F,
 * its reductions read from a script: the k-th cost evaluation returns costs[k], the k-th linearisation the 14 sums
 * acc14[14 k ..].  p3 becomes the final point; used2 (may be NULL; no other output may) = cost evaluations and
 * linearisations consumed.  LT_ERR_STATE, with the outputs written, where the script is shorter than the solve. */
int lt_fn_lm_loop_script(double F, int max_iter, int64_t n_costs, const double *costs, int64_t n_lin, const double *acc14,
                         double p3[3], double *cost1, int32_t *iters, int32_t *code, int64_t used2[2]);
/* For tests: the free-pose solve of lt_fn_ba_host (one thread) with what every attempt hands to its decision recorded.
 * *total0: the sum of the blocks' cost terms at the initial point.  rec5[5 a ..] of attempt a (the first `cap` are
 * written, *n_attempts counts all): the radius it ran with, 1 where a factorisation failed (-1: the attempt ended the
 * solve by the zero gradient and no decision was taken), 1 where it linearised anew, the cost total and the total of the
 * model-decrease terms.  cost2, iters, code (any may be NULL) as lt_fn_ba_host. */
int lt_fn_ba_host_trace(int n_img, const int32_t *img_ids, const double *kvec4, const double *qvec4, const double *tvec3,
                        int64_t n_pt, const double *pt3, const int64_t *pt_off, const int32_t *pt_img, const double *pt_xy2,
                        int64_t n_ln, const double *line6, const int64_t *ln_off, const int32_t *ln_img, const double *l2d4,
                        const double *l3d6, const lt_ba_config *cfg, int64_t cap, int64_t *n_attempts, double *total0,
                        double *rec5, double *cost2, int32_t *iters, int32_t *code);
/* the defined factorisation alone: L (n x n by rows, zero above the diagonal) of S (its lower triangle is read),
 * L_ij = (S_ij - sum_{k<j} L_ik L_jk) / L_jj with the sum in ascending k from S_ij, and, with rhs and x, the solution
 * of S x = rhs by substitutions under the same rule.  LT_ERR_STATE: a pivot is not positive or not finite */
int lt_fn_ba_cholesky(int64_t n, const double *S, const double *rhs, double *L, double *x);

/* ---- Global point-line association: limap.optimize.global_pl_association's GlobalAssociator with
 * constant cameras.  The unknowns are the point tracks (3 each), the line tracks (4, section 19's chart) and the
 * vanishing points (2, the chart of DESIGN section 29), coupled by association edges: point-line (R2.1), VP-line (R2.2),
 * VP-VP orthogonality (R2.3) and collinearity (R2.4).  limap's residuals, weights, losses and SetUp switches are
 * restated; the minimiser is this project's definition: section 27's loop with its linear step by preconditioned
 * conjugate gradients on the explicitly assembled block-sparse matrix.  The results are a stationary point of
 * upstream's cost reached from the input, not the iterates of a Ceres run. ---- */
typedef struct lt_assoc_config {
  double geometric_alpha;            /* 10 */
  double lw_point;                   /* 0.1; <= 0 adds no R1.1 block */
  double lw_pointline_association;   /* 10; <= 0 adds no R2.1 block */
  double lw_vpline_association;      /* 1; <= 0 adds no R2.2 block */
  double lw_vp_orthogonality;        /* 1; <= 0 adds no R2.3 block */
  double lw_vp_collinearity;         /* 0; <= 0 adds no R2.4 block */
  double cg_eta;                     /* 0.1 (Ceres' eta): CG stops at sqrt(r.z) <= eta sqrt(r0.z0) */
  int32_t cg_max_iterations;         /* 500 (Ceres' max_linear_solver_iterations) */
  int32_t min_num_images;            /* 4: a line track seen in fewer images keeps its line */
  int32_t max_num_iterations;        /* 100; an attempt counts whether accepted or not */
  int32_t constant_intrinsics, constant_pose; /* 1, 1; 0 is LT_ERR_ARGUMENT (free cameras are not built here) */
  int32_t constant_point, constant_line, constant_vp; /* 0 */
  int32_t enable_pointline, enable_vpline; /* 1: Init2DBipartites_PointLine / _VPLine was called */
  int32_t poll_interval;             /* batches enqueued between two reads of the status record; 0: the default (4) */
  int32_t cg_batch;                  /* CG iterations enqueued per batch; 0: the default (4), at most 64.  The result
                                        depends on neither */
  int32_t kernel_timers;             /* 1: HIP events around every kernel (poll_interval becomes 1) */
  int32_t pad_;
} lt_assoc_config;
void lt_assoc_config_default(lt_assoc_config *cfg);
/* The problem.  Cameras, point tracks and line tracks as lt_ba_arrays takes them (no 3D supports: the segment cut is
 * lt_fn_refine_cut's).  vp3: the vanishing points' directions.  Edges in the order upstream's maps give them:
 * edge_kind 0 point-line (a = point track, b = line track; w = the count of supports within th_pixel), 1 VP-line
 * (a = VP, b = line track; w = the count), 2 VP-VP orthogonality, 3 VP-VP collinearity (a < b VPs; w unused); a, b
 * index the arrays.  The ScaledLoss weights (w lw, w 1e2 lw, 1e2 lw) and SetUp's switches are applied here. */
typedef struct lt_assoc_input {
  int32_t n_img, pad_;
  const int32_t *img_ids;
  const double *kvec4, *qvec4, *tvec3;
  int64_t n_pt;
  const double *pt3;
  const int64_t *pt_off;
  const int32_t *pt_img;
  const double *pt_xy2;
  int64_t n_ln;
  const double *line6;
  const int64_t *ln_off;
  const int32_t *ln_img;
  const double *l2d4;
  int64_t n_vp;
  const double *vp3;
  int64_t n_edge;
  const int32_t *edge_kind, *edge_a, *edge_b;
  const double *edge_w;
} lt_assoc_input;
/* LT_ERR_ARGUMENT before any launch: constant_pose = 0 or constant_intrinsics = 0, non-finite input, an image id or an
 * edge's index that is not in the collection, a vanishing point or a track line of zero length. */
int lt_assoc_arrays(lt_ctx *ctx, const lt_assoc_input *in, const lt_assoc_config *cfg);
/* of the last lt_assoc_arrays (any pointer may be NULL): the points, the lines' minimal parameters (uvec, wvec), the
 * vanishing points (a free one is a unit vector, a constant one its input), cost2 = the cost at the initial and at the
 * final point, the iterations, the CG iterations of all attempts, and the termination code: 0 max_num_iterations,
 * 1 radius, 2 zero gradient, 6 the cost at the initial point is not finite, 7 no residual block; 6 and 7 change nothing */
int lt_assoc_get(lt_ctx *ctx, double *pt3, double *params6, double *vp3, double *cost2, int32_t *iters, int64_t *cg_iters,
                 int32_t *code);
/* host ms of [0] validation, tables and upload, [1] the loop, [2] download; [3] batches enqueued; with kernel_timers the
 * device ms of [4] k_as_linearize [5] k_as_diag [6] k_as_diag_vp [7] k_as_precond [8] k_as_cg_begin [9] k_as_matvec
 * [10] k_as_alpha [11] k_as_update [12] k_as_beta [13] k_as_dir [14] k_as_backsub [15] k_as_cost [16] k_as_decide,
 * summed over the batches */
int lt_assoc_get_timers(lt_ctx *ctx, double out[20]);
/* The same definition on the host, no context and no device: bit-identical results for every host_threads (0: default).
 * For tests, with trace_cap > 0: rec6[6 a ..] of attempt a (the first trace_cap are written, *n_attempts counts all):
 * the radius it ran with, 1 where the linear solve failed (-1: the attempt ended the solve by the zero gradient), 1
 * where it linearised anew, the cost total, the total of the model-decrease terms, its CG iterations; *total0: the sum
 * of the blocks' cost terms at the initial point (n_attempts, total0, rec6 may be NULL). */
int lt_fn_assoc_host(const lt_assoc_input *in, const lt_assoc_config *cfg, int host_threads, double *pt3, double *params6,
                     double *vp3, double *cost2, int32_t *iters, int64_t *cg_iters, int32_t *code, int64_t trace_cap,
                     int64_t *n_attempts, double *total0, double *rec6);
const char *lt_fn_assoc_host_error(void);
/* For tests: the problem at the point sp6 (6 doubles per unknown -- point p[3], line uvec wvec, VP v[3] -- or NULL: the
 * initial point).  dims8 = unknowns, points, lines, VPs, R1 blocks, edges, 0, 0; with every other output NULL only dims8
 * is written.  unk_nd per unknown (0: constant); blk_unk per R1 block its unknown; edge_info3 per edge kind, a, b
 * (unknowns) and edge_w its ScaledLoss weight; sp6_out the point; res_blk 2 per R1 block, res_edge 3 per edge; cost;
 * g4 and diag16 per unknown (the 4 x 4 diagonal block, undamped); off16 per edge (rho' J_a^T J_b, 4 x 4 row-major). */
int lt_fn_assoc_eval(const lt_assoc_input *in, const lt_assoc_config *cfg, const double *sp6, int64_t *dims8,
                     int32_t *unk_nd, int32_t *blk_unk, int32_t *edge_info3, double *edge_w, double *sp6_out,
                     double *res_blk, double *res_edge, double *cost, double *g4, double *diag16, double *off16);
/* LineLinker2d(LineLinker2dConfig()).check_connection(l1, l2) on two segments (x1 y1 x2 y2): the default 2D linker of
 * GlobalAssociator::test_linetrack_validity.  1 connected, 0 not.  No context, no device. */
int lt_fn_assoc_link2d(const double l1[4], const double l2[4]);
/* For tests: the linear solve alone.  n_unk unknowns of nd (0 .. 4) dimensions with their (damped) diagonal blocks
 * diag16, n_edge off-diagonal blocks off16 between the unknowns edge_a, edge_b (rows a's, columns b's), the right-hand
 * side rhs4: preconditioned CG from x = 0 in the defined orders.  x4 = the step; *iters; *end = 0 converged, 1 the cap,
 * 2 p.Ap or r0.z0 not positive and finite, 3 a pivot of a diagonal block; rz2 (may be NULL) = r0.z0 and the last r.z */
int lt_fn_assoc_pcg(int64_t n_unk, const int32_t *nd, const double *diag16, int64_t n_edge, const int32_t *edge_a,
                    const int32_t *edge_b, const double *off16, const double *rhs4, double eta, int32_t cap, double *x4,
                    int32_t *iters, int32_t *end, double *rz2);

/* Counters of the last device run: [0] connections tested, [1] candidates, [2] ordered candidate
 * pairs swept by the scoring kernel (sum n_tris^2), [3] valid edges, [4] graph nodes,
 * [5] graph edges, [6] tracks, [7] nodes. */
int lt_get_stats(lt_ctx *ctx, int64_t out[8]);
/* HIP-event timings (ms) of the last lt_run_device on the context's stream:
 * [0] whole run, [1], [2] unused (0), [3] generation (incl. the per-pair records), [4] placement of the
 * candidates, [5] scoring (incl. its per-candidate records), [6] selection, [7] unused (0); host: [8] upload, [9] download,
 * [10] tail (lt_compute_tracks); [11] candidate pairs that reached the dense evaluation in k_score3;
 * [12] host ms spent inside lt_triangulate_image* buffering the match rows of the batch;
 * single-kernel durations (HIP events around the launch): [13] k_gates, [14] k_tri_rows (only with LT_FINE_TIMERS=2
 * in the environment at the time of the run), [15] k_score3 (default; LT_FINE_TIMERS=0 turns every per-kernel event off);
 * [16] connections that passed the stage-A gates (k_gates);
 * one-pass exhaustive mode: [17] staging slots needed (fullest region x regions), [18] staging slots provided;
 * [19] 1 when this context scores with the fused kernel because the split form's pair store overflowed once, else 0;
 * [20] 1 when stage A of the last TriangulateImage job ran in the line-slot form (k_gates_ln: one lane per line), else 0;
 * [21] 1 when this context scores in the two-kernel form because the one-kernel form (k_score_q) raised its flag once, else 0;
 * [22], [23] of the last lt_compute_tracks ([10]): its device half + graph, its edge order + union-find (the rest of [10] is
 * the track members and their aggregation).
 * [15] spans the whole scoring stage (one kernel, k_score_q, by default for TriangulateImage jobs; two in the fallback form).
 * SAMPLING: an event between two kernels costs a ~5 us bubble in the stream, so a run enqueued BEHIND one still in flight
 * (lt_run_device_async back to back) carries the stage events -- [3]-[6], [13]-[15] -- only every LT_TIMER_SAMPLE-th time
 * (environment, read per run; default 8, 1 = every run); in between those slots keep the values of the last run that
 * did.  A run that starts on an idle context always carries them; [0] is measured for every run. */
int lt_get_timers(lt_ctx *ctx, double out[24]);
/* The same slots summed over every lt_run_device since the last reset ([8]-[10], [12] are not summed), and
 * the number of runs ([16] is not summed either: lt_get_timers counts it on demand with a device readback,
 * which is why a caller that times many runs should read the sums once instead of lt_get_timers per run).
 * reset != 0 clears the sums after reading.  The sampled stage slots (above) are summed over the sampled runs and
 * scaled to the number of runs. */
int lt_get_timer_sums(lt_ctx *ctx, double out[24], int64_t *n_runs, int reset);

/* The library keeps released device blocks and page-locked staging blocks in a process-wide cache
 * (contexts are typically created once per scene; hipMalloc / hipHostMalloc / hipFree are the slow part
 * of that).  This returns the cached memory of all devices to the driver; live contexts are unaffected.
 * No reference counterpart (the reference holds everything in host std::maps). */
void lt_release_cached_memory(void);

/* Puts `blocks` page-locked staging blocks of `bytes` each (rounded up to the cache's size class) into that cache, so
 * that the first scene of a process does not pin its match-row staging inside TriangulateImage (pinning costs
 * ~0.1 ms per MB).  Used by limap_amd.warmup(); LT_OK or LT_ERR_HIP.  No reference counterpart. */
int lt_reserve_host(uint64_t bytes, int blocks);

/* ---- free functions of limap.triangulation (bindings.cc:22-31) on raw arrays, run on the GPU
 * one query per call (convenience / parity checks; the batch path is the API above).
 * cam = kvec[4] | qvec[4] | tvec[3]; seg = x1,y1,x2,y2; line10 as above. */
int lt_fn_get_normal_direction(lt_ctx *ctx, const double seg[4], const double cam[11], double out[3]);
/* get_direction_from_VP(vp, view): functions.cc:37-42 */
int lt_fn_get_direction_from_vp(lt_ctx *ctx, const double vp[3], const double cam[11], double out[3]);
/* triangulate_point(p1, view1, p2, view2) -> (point, ok): functions.cc:100-117 */
int lt_fn_triangulate_point(lt_ctx *ctx, const double p1[2], const double cam1[11], const double p2[2],
                            const double cam2[11], double out[3], int *ok);
/* triangulate_line_with_direction(l1, view1, l2, view2, direction): functions.cc:385-442 */
int lt_fn_triangulate_line_with_direction(lt_ctx *ctx, const double seg1[4], const double cam1[11],
                                          const double seg2[4], const double cam2[11], const double direction[3],
                                          double out_line10[10]);
/* triangulate_line_with_one_point(l1, view1, l2, view2, point): functions.cc:325-383.  The reference's
 * solver (solvers/triangulation, a generated quartic + PoseLib's root finder) is restated from the
 * optimisation problem it solves, so this proposal agrees to rounding, not bit for bit. */
int lt_fn_triangulate_line_with_one_point(lt_ctx *ctx, const double seg1[4], const double cam1[11],
                                          const double seg2[4], const double cam2[11], const double point[3],
                                          double out_line10[10]);
int lt_fn_compute_fundamental_matrix(lt_ctx *ctx, const double cam1[11], const double cam2[11],
                                     double out[9]);
int lt_fn_compute_epipolar_IoU(lt_ctx *ctx, const double seg1[4], const double cam1[11],
                               const double seg2[4], const double cam2[11], double *out);
int lt_fn_triangulate_line(lt_ctx *ctx, const double seg1[4], const double cam1[11],
                           const double seg2[4], const double cam2[11], int by_endpoints,
                           double out_line10[10]);

/* merging::Aggregator::aggregate_line3d_list(lines, scores, num_outliers) (merging/aggregator.cc:53-101; takebest
 * :8-29 below four lines) as ComputeLineTracks and the track post-processing apply it (call sites
 * global_line_triangulator.cc:348, merging/merging_utils.cc:77, merging/merging.cc:509,635).  Host code of the tail: no
 * context, no device.  lines10 = n x line10 (uncertainty at [8]); out7 = start, end, uncertainty.  The orientation of
 * the result (which end is `start`) follows the sign rule documented in DESIGN.md section 5. */
int lt_fn_aggregate_line3d_list(int n, const double *lines10, const double *scores, int num_outliers, double out7[7]);

/* The host pass TriangulateImage / TriangulateAll make over one (image, neighbour) block of match rows -- the (n, 2)
 * int32 matrix `matches[ng_img_id]` of base_line_triangulator.cc:82-98 -- exposed for tests: out[r] = rows[r][0] |
 * rows[r][1] << 16 (the staged form), stats = {largest rows[:,0], largest rows[:,1] (as unsigned: a negative id wraps),
 * 1 if any rows[r][0] < rows[r-1][0]}.  The out-of-index error of :87-94 is raised from these maxima.  level: 0 = the
 * widest vector path the CPU has, 1 = scalar, 2 = AVX2, 3 = AVX-512 (a level the CPU lacks falls back to the widest).
 * No context, no device. */
int lt_fn_pack_match_rows(const int32_t *rows, int64_t n, uint32_t *out, uint32_t stats[3], int level);
/* the same pass into the COMPRESSED block form the rows cross PCIe in since round 4 (17 bits per row: the neighbour line
 * of every row + one "a new line starts here" bit; limap_amd/csrc/lt_rows.h), for blocks sorted by line id with steps of
 * 0 / +1 -- what limap's matchers write.  out: lt_fn_compressed_block_words(n) words, 8-byte aligned; stats[3] != 0: the
 * block is not of that shape (it is then staged in the plain form above). */
int64_t lt_fn_compressed_block_words(int64_t n);
int lt_fn_pack_match_rows_compressed(const int32_t *rows, int64_t n, uint32_t *out, uint32_t stats[4], int level);

#ifdef __cplusplus
}
#endif
#endif /* LIMAP_AMD_H */
