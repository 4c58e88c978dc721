// lt_merge.cpp -- limap.merging.merging / MergeToLineTracks (merging/merging.py:6-21, merging/merging.cc:347-511) on a
// context initialised with the cameras and the 2D segments.
//
// Host: the per-line records (uncertainty of _SetUncertaintySegs3d, merging_utils.cc:15-25; length; unit direction),
// node numbering, the reference's edge insertion order, the greedy labels (lt_tail.h) and the aggregation of every track
// (lt_tail.h aggregate_impl, num_outliers 0).  Device: every pair test of the self and the cross pass
// (lt_kernels_merge.hip).  The result is a track set (lt_tracks.cpp), so that the filters and the remerge of the
// fit-and-merge runner (runners/line_fitnmerge.py:229-258) apply to it directly.

#include "lt_host.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>
#include <tuple>
#include <vector>

using namespace lt;
using namespace lt_impl;

extern "C" {

int lt_merge_to_tracks(lt_ctx *ctx, const int64_t *seg3d_off, const double *seg3d, const int64_t *nb_off,
                       const int32_t *nb_ids, const lt_config *linker_cfg, double var2d, lt_trackset **out) {
  if (out) *out = nullptr;
  if (!ctx->inited) return fail(ctx, LT_ERR_STATE, "lt_merge_to_tracks before lt_init");
  if (!seg3d_off || !nb_off || !linker_cfg || !out) return fail(ctx, LT_ERR_ARGUMENT, "null argument");
  const double t_start = now_ms();
  const int n_img = ctx->n_img;
  // THROW_CHECK_EQ(all_lines_2d.at(image_id).size(), all_lines_3d.at(image_id).size()) (merging.cc:367-368)
  for (int n = 0; n < n_img; ++n) {
    const long long m2 = ctx->seg_off[(size_t)n + 1] - ctx->seg_off[(size_t)n];
    const long long m3 = (long long)(seg3d_off[n + 1] - seg3d_off[n]);
    if (m2 != m3)
      return fail(ctx, LT_ERR_ARGUMENT, "image " + std::to_string(ctx->img_ids[(size_t)n]) + ": " + std::to_string(m2) +
                                            " 2D segments but " + std::to_string(m3) + " 3D segments");
  }
  // neighbors.at(image_id)[ng_id] -> all_lines_2d.at(ng_image_id) (merging.cc:422-424)
  std::vector<int> nb_idx;
  nb_idx.reserve((size_t)std::max<int64_t>(nb_off[n_img] - nb_off[0], 0));
  for (int64_t k = nb_off[0]; k < nb_off[n_img]; ++k) {
    auto it = ctx->id2idx.find(nb_ids[k]);
    if (it == ctx->id2idx.end())
      return fail(ctx, LT_ERR_ARGUMENT, "unknown neighbour image id " + std::to_string(nb_ids[k]));
    nb_idx.push_back(it->second);
  }
  // the linkers: the caller's 2D config, the 3D config switched to set_to_spatial_merging() (line_linker.h:123-129)
  const LinkCfg2 l2 = make_l2(*linker_cfg);
  LinkCfg3 l3 = make_l3(*linker_cfg);
  l3.use_angle = 1; l3.use_overlap = 1; l3.use_perp = 0; l3.use_innerseg = 1; l3.use_scaleinv = 0;
  const double th = l3.th_angle * (1.0 + 1e-6) + 1e-6;
  double cos_guard = (th < 90.0) ? std::cos(th * kPi / 180.0) : -1.0;
  if (test_switch("LT_TEST_MERGE_NO_GUARD")) cos_guard = -1.0;  // every pair through the exact 3D test

  // per-line records, nodes in (ascending image id, line) order (merging.cc:360-374)
  const long long G = ctx->G;
  std::vector<MLine> lines((size_t)std::max<long long>(G, 1));
  std::vector<int> node_of((size_t)std::max<long long>(G, 1), -1);
  ctx->mg.node_img.clear(); ctx->mg.node_line.clear();
  for (int n = 0; n < n_img; ++n) {
    const Cam &cam = ctx->h_cams[(size_t)n];
    const long long g0 = ctx->seg_off[(size_t)n], m = ctx->seg_off[(size_t)n + 1] - g0;
    for (long long l = 0; l < m; ++l) {
      const double *p = seg3d + 6 * (seg3d_off[n] + l);
      MLine &r = lines[(size_t)(g0 + l)];
      const L3 ln{mk3(p[0], p[1], p[2]), mk3(p[3], p[4], p[5])};
      for (int k = 0; k < 3; ++k) { r.s[k] = p[k]; r.e[k] = p[3 + k]; }
      const d3 dv = dir(ln);
      r.dir[0] = dv.x; r.dir[1] = dv.y; r.dir[2] = dv.z;
      // Line3d::computeUncertainty (linebase.cc:109-116), Camera::uncertainty (camera.cc:228-242)
      const double d = (cam_depth(cam, ln.s) + cam_depth(cam, ln.e)) / 2.0;
      r.unc = var2d * d / cam.f;
      r.len = len(ln);
      // the segments as given: MergeToLineTracks never shifts them by half a pixel, whatever the context's add_halfpix
      const double *s2 = ctx->h_segs_ptr + 4 * (g0 + l);
      for (int k = 0; k < 4; ++k) r.seg[k] = s2[k];
      r.pad_ = 0.0;
      if (r.len == 0) continue;  // merging.cc:370-371: exact test
      node_of[(size_t)(g0 + l)] = (int)ctx->mg.node_img.size();
      ctx->mg.node_img.push_back(ctx->img_ids[(size_t)n]);
      ctx->mg.node_line.push_back((int)l);
    }
  }
  const int n_nodes = (int)ctx->mg.node_img.size();

  // workgroups: self pass of every image, then one per (image, neighbour slot), each in tiles of 256 rows
  std::vector<MBlock> self_blks, cross_blks;
  long long max_id = 0, max_lines = 0;
  bool ids_nonneg = true;
  for (int n = 0; n < n_img; ++n) {
    const int rows = (int)(ctx->seg_off[(size_t)n + 1] - ctx->seg_off[(size_t)n]);
    max_lines = std::max<long long>(max_lines, rows);
    const int id = ctx->img_ids[(size_t)n];
    ids_nonneg = ids_nonneg && id >= 0;
    max_id = std::max<long long>(max_id, std::llabs((long long)id));
    for (int r0 = 0; r0 < rows; r0 += 256) self_blks.push_back(MBlock{n, n, -1, r0, id, id, {0, 0}});
    for (int64_t k = nb_off[n]; k < nb_off[n + 1]; ++k) {
      const int nb = nb_idx[(size_t)(k - nb_off[0])];
      if (ctx->seg_off[(size_t)nb + 1] == ctx->seg_off[(size_t)nb]) continue;
      for (int r0 = 0; r0 < rows; r0 += 256)
        cross_blks.push_back(MBlock{n, nb, (int)(k - nb_off[n]), r0, id, ctx->img_ids[(size_t)nb], {0, 0}});
    }
  }
  int parity_fast = (ids_nonneg && 2 * max_id + 2 * max_lines < (1ll << 30)) ? 1 : 0;
  if (test_switch("LT_TEST_MERGE_PARITY_SLOW")) parity_fast = 0;  // the reference's int key on every pair

  // device: both passes into one edge buffer; an overflow is counted, never truncated, and runs again
  hipStream_t st = ctx->stream;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::vector<MBlock> blks(self_blks);
  blks.insert(blks.end(), cross_blks.begin(), cross_blks.end());
  unsigned long long capacity = std::max<unsigned long long>(1ull << 16, 8ull * (unsigned long long)n_nodes);
  if (const char *e = test_switch("LT_TEST_MERGE_EDGE_CAP")) capacity = std::max(1ull, std::strtoull(e, nullptr, 10));
  std::vector<MEdge> h_edges;
  unsigned long long n_found = 0;
  int attempts = 0;
  Events<2> ev;  // around the two launches of the attempt that fitted
  if (!blks.empty()) {
    if (int rc = upload_vec(ctx, ctx->mg.d_lines, lines)) return rc;
    if (int rc = upload_vec(ctx, ctx->mg.d_blks, blks)) return rc;
    if (int rc = ev.create(ctx)) return rc;
    const MBlock *d_blks = ctx->mg.d_blks.as<MBlock>();
    // [counter (8 B, padded to 16) | capacity edges of 16 B]
    if (int rc = run_counted(ctx, ctx->mg.d_edges, 16, sizeof(MEdge), capacity,
                             [&](void *items, unsigned long long cap, unsigned long long *d_cnt) {
          MEdge *d_edges = static_cast<MEdge *>(items);
          if (int rc = ev.record(ctx, 0)) return rc;
          launch_merge_pairs(st, true, (int)self_blks.size(), d_blks, ctx->d_seg_off.as<long long>(),
                             ctx->mg.d_lines.as<MLine>(), ctx->d_cams.as<Cam>(), l2, l3, cos_guard, parity_fast, d_edges,
                             cap, d_cnt);
          launch_merge_pairs(st, false, (int)cross_blks.size(), d_blks + self_blks.size(),
                             ctx->d_seg_off.as<long long>(), ctx->mg.d_lines.as<MLine>(), ctx->d_cams.as<Cam>(), l2, l3,
                             cos_guard, parity_fast, d_edges, cap, d_cnt);
          return ev.record(ctx, 1);
        }, &n_found, &attempts))
      return rc;
    if (int rc = download(ctx, h_edges, ctx->mg.d_edges.as<char>() + 16, (size_t)n_found)) return rc;
    if (int rc = stream_sync(ctx)) return rc;
  }

  // the reference's insertion order (merging.cc:458-469): image, self pass before cross pass, then the loop indices
  std::sort(h_edges.begin(), h_edges.end(), [](const MEdge &a, const MEdge &b) {
    return std::make_tuple(a.img, a.slot >= 0, a.line, a.slot, a.ng_line) <
           std::make_tuple(b.img, b.slot >= 0, b.line, b.slot, b.ng_line);
  });
  std::vector<UnionEdge> ue(h_edges.size());
  ctx->mg.e1.resize(h_edges.size()); ctx->mg.e2.resize(h_edges.size()); ctx->mg.sim.resize(h_edges.size());
  for (size_t k = 0; k < h_edges.size(); ++k) {
    const MEdge &e = h_edges[k];
    const int nb = e.slot < 0 ? e.img : nb_idx[(size_t)(nb_off[e.img] - nb_off[0] + e.slot)];
    const long long g1 = ctx->seg_off[(size_t)e.img] + e.line, g2 = ctx->seg_off[(size_t)nb] + e.ng_line;
    ue[k] = UnionEdge{lines[(size_t)g1].len + lines[(size_t)g2].len, node_of[(size_t)g1], node_of[(size_t)g2]};
    ctx->mg.e1[k] = ue[k].n1; ctx->mg.e2[k] = ue[k].n2; ctx->mg.sim[k] = ue[k].sim;
  }
  // ComputeLineTrackLabelsGreedy: std::sort of (sim, idx1, idx2) tuples, then reversed (merging.cc:33-34)
  std::sort(ue.begin(), ue.end(), [](const UnionEdge &a, const UnionEdge &b) {
    return std::tie(b.sim, b.n1, b.n2) < std::tie(a.sim, a.n1, a.n2);
  });
  std::vector<int> node_imgidx((size_t)n_nodes);
  std::vector<long long> node_g((size_t)n_nodes);
  for (long long g = 0; g < G; ++g)
    if (node_of[(size_t)g] >= 0) node_g[(size_t)node_of[(size_t)g]] = g;
  for (int i = 0; i < n_nodes; ++i) node_imgidx[(size_t)i] = ctx->mg.node_img[(size_t)i];
  std::vector<int> labels;
  const int n_tracks = n_nodes > 0 ? greedy_track_labels(n_nodes, node_imgidx.data(), ue, labels) : 0;

  // tracks (merging.cc:480-510): members in node order, score = length, line = aggregate(lines, scores, 0)
  std::vector<int64_t> off((size_t)n_tracks + 1, 0);
  for (int i = 0; i < n_nodes; ++i)
    if (labels[(size_t)i] >= 0) ++off[(size_t)labels[(size_t)i] + 1];
  for (int t = 0; t < n_tracks; ++t) off[(size_t)t + 1] += off[(size_t)t];
  const size_t M = (size_t)off[(size_t)n_tracks];
  std::vector<int32_t> m_img(std::max<size_t>(M, 1)), m_lid(std::max<size_t>(M, 1)), m_nid(std::max<size_t>(M, 1));
  std::vector<double> m_sc(std::max<size_t>(M, 1)), m_l2(4 * std::max<size_t>(M, 1)), m_l3(10 * std::max<size_t>(M, 1));
  std::vector<Cand> m_cand(std::max<size_t>(M, 1));
  std::vector<int64_t> wr(off.begin(), off.end() - 1);
  for (int i = 0; i < n_nodes; ++i) {
    const int t = labels[(size_t)i];
    if (t < 0) continue;
    const size_t w = (size_t)wr[(size_t)t]++;
    const MLine &r = lines[(size_t)node_g[(size_t)i]];
    m_img[w] = ctx->mg.node_img[(size_t)i]; m_lid[w] = ctx->mg.node_line[(size_t)i]; m_nid[w] = i;
    m_sc[w] = r.len;
    for (int k = 0; k < 4; ++k) m_l2[4 * w + k] = r.seg[k];
    // Line3d(MatrixXd) (linebase.cc:60-65): score -1; its depths are not set there (0 here, as value-initialised)
    double *o = &m_l3[10 * w];
    for (int k = 0; k < 3; ++k) { o[k] = r.s[k]; o[3 + k] = r.e[k]; }
    o[6] = 0.0; o[7] = 0.0; o[8] = r.unc; o[9] = -1.0;
    Cand &c = m_cand[w];
    for (int k = 0; k < 3; ++k) { c.s[k] = r.s[k]; c.e[k] = r.e[k]; }
    c.depth[0] = c.depth[1] = 0.0; c.unc = r.unc; c.score3 = -1.0;
    for (int k = 0; k < 4; ++k) c.seg[k] = r.seg[k];
  }
  std::vector<double> line7(7 * (size_t)std::max(n_tracks, 1));
  std::vector<uint8_t> active((size_t)std::max(n_tracks, 1), 1);
  {
    AggScratch sc;
    for (int t = 0; t < n_tracks; ++t) {
      const int64_t a = off[(size_t)t], n = off[(size_t)t + 1] - a;
      aggregate_impl([&](int k) -> const Cand & { return m_cand[(size_t)(a + k)]; }, m_sc.data() + a, (int)n, 0,
                     &line7[7 * (size_t)t], sc);
    }
  }
  *out = lt_ts_create(n_tracks, line7.data(), active.data(), off.data(), m_img.data(), m_lid.data(), m_nid.data(),
                      m_sc.data(), m_l2.data(), m_l3.data());
  ctx->mg.timers[0] = ev.ms(0, 1);
  ctx->mg.timers[1] = now_ms() - t_start;
  ctx->mg.timers[2] = attempts;
  ctx->mg.timers[3] = (double)n_found;
  return LT_OK;
}

int lt_merge_graph_size(lt_ctx *ctx, int64_t *n_nodes, int64_t *n_edges) {
  if (n_nodes) *n_nodes = (int64_t)ctx->mg.node_img.size();
  if (n_edges) *n_edges = (int64_t)ctx->mg.e1.size();
  return LT_OK;
}

int lt_merge_graph_get(lt_ctx *ctx, int32_t *node_img, int32_t *node_line, int32_t *edge_n1, int32_t *edge_n2,
                       double *edge_sim) {
  if (node_img) std::copy(ctx->mg.node_img.begin(), ctx->mg.node_img.end(), node_img);
  if (node_line) std::copy(ctx->mg.node_line.begin(), ctx->mg.node_line.end(), node_line);
  if (edge_n1) std::copy(ctx->mg.e1.begin(), ctx->mg.e1.end(), edge_n1);
  if (edge_n2) std::copy(ctx->mg.e2.begin(), ctx->mg.e2.end(), edge_n2);
  if (edge_sim) std::copy(ctx->mg.sim.begin(), ctx->mg.sim.end(), edge_sim);
  return LT_OK;
}

int lt_merge_get_timers(lt_ctx *ctx, double out[4]) {
  for (int k = 0; k < 4; ++k) out[k] = ctx->mg.timers[k];
  return LT_OK;
}

}  // extern "C"
