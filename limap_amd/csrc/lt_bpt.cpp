// lt_bpt.cpp -- limap.structures.PL_Bipartite2d on the GPU (structures/pl_bipartite.cc): the keypoint-line
// association of add_keypoints_with_point3D_ids (lt_bpt_associate) and the junctions of
// compute_intersection_with_points (lt_bpt_junctions), each for a batch of images in one call.  The host validates,
// sizes the compacted outputs from the counts of the first pass of each kernel, replays the union-find of :129-143
// over the close pairs the device found, and merges the clusters (merge_junctions, :206-223); every distance and
// every intersection is computed on the device (lt_kernels_bpt.hip).  DESIGN §16.

#include "lt_host.h"
#include "lt_bpt.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <string>
#include <vector>

using namespace lt;
using namespace lt_impl;

namespace {

constexpr long long kMaxCandidates = (1ll << 32) - 1;  // a pair is (candidate << 32 | candidate)
constexpr long long kMaxPairs = 1ll << 31;
constexpr int kMaxImages = 1 << 23;                    // the image index above the two cell coordinates of a key

int check_common(lt_ctx *ctx, const char *who, int n_img, const int64_t *line_off, const double *lines,
                 const int64_t *pt_off, const double *pts, const lt_bpt_config *cfg) {
  if (!cfg) return fail(ctx, LT_ERR_ARGUMENT, std::string(who) + ": null configuration");
  if (n_img < 0 || n_img > kMaxImages) return fail(ctx, LT_ERR_ARGUMENT, std::string(who) + ": bad image count");
  if (std::isnan(cfg->threshold_keypoints) || std::isnan(cfg->threshold_intersection) ||
      std::isnan(cfg->threshold_merge_junctions))
    return fail(ctx, LT_ERR_ARGUMENT, std::string(who) + ": a threshold is NaN");
  if (int rc = check_offsets(ctx, who, "line", n_img, line_off)) return rc;
  if (int rc = check_offsets(ctx, who, "point", n_img, pt_off)) return rc;
  if ((line_off[n_img] > 0 && !lines) || (pt_off[n_img] > 0 && !pts))
    return fail(ctx, LT_ERR_ARGUMENT, std::string(who) + ": null coordinates");
  if (int rc = check_finite(ctx, who, lines, 4 * line_off[n_img], "line coordinate")) return rc;
  return check_finite(ctx, who, pts, 2 * pt_off[n_img], "point coordinate");
}

// workgroups of kBptBlock items, none across an image
std::vector<BptBlock> make_blocks(int n_img, const long long *off) {
  std::vector<BptBlock> out;
  for (int m = 0; m < n_img; ++m)
    for (long long b = off[m]; b < off[m + 1]; b += kBptBlock)
      out.push_back(BptBlock{m, 0, b, std::min<long long>(b + kBptBlock, off[m + 1])});
  return out;
}

// counts -> exclusive prefix sums (n + 1 values)
std::vector<long long> scan(const std::vector<int> &cnt) {
  std::vector<long long> off(cnt.size() + 1);
  off[0] = 0;
  for (size_t k = 0; k < cnt.size(); ++k) off[k + 1] = off[k] + cnt[k];
  return off;
}

// lines (raw -> prepared) and the CSR of the images; leaves the stream idle
int upload_scene(lt_ctx *ctx, int n_img, const int64_t *line_off, const double *lines, const int64_t *pt_off,
                 const double *pts) {
  const long long nl = line_off[n_img], np = pt_off[n_img];
  hipStream_t st = ctx->stream;
  ENSURE(ctx, ctx->bp.d_raw, 32 * (size_t)std::max<long long>(nl, 1));
  ENSURE(ctx, ctx->bp.d_lines, sizeof(BptLine) * (size_t)std::max<long long>(nl, 1));
  ENSURE(ctx, ctx->bp.d_pts, 16 * (size_t)std::max<long long>(np, 1));
  ENSURE(ctx, ctx->bp.d_off, 8 * (size_t)(n_img + 1));
  ENSURE(ctx, ctx->bp.d_off2, 8 * (size_t)(n_img + 1));
  if (nl) HIPCHK(ctx, hipMemcpyAsync(ctx->bp.d_raw.p, lines, 32 * (size_t)nl, hipMemcpyHostToDevice, st));
  if (np) HIPCHK(ctx, hipMemcpyAsync(ctx->bp.d_pts.p, pts, 16 * (size_t)np, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(ctx->bp.d_off.p, line_off, 8 * (size_t)(n_img + 1), hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(ctx->bp.d_off2.p, pt_off, 8 * (size_t)(n_img + 1), hipMemcpyHostToDevice, st));
  return stream_sync(ctx);
}

}  // namespace

extern "C" {

void lt_bpt_config_default(lt_bpt_config *cfg) {
  if (!cfg) return;
  cfg->threshold_keypoints = 2.0;  // structures/pl_bipartite.h:30-32
  cfg->threshold_intersection = 2.0;
  cfg->threshold_merge_junctions = 2.0;
}

int lt_bpt_associate(lt_ctx *ctx, int n_img, const int64_t *line_off, const double *lines, const int64_t *pt_off,
                     const double *pts, const lt_bpt_config *cfg, int64_t *n_edges) {
  if (!ctx) return LT_ERR_ARGUMENT;
  const char *who = "lt_bpt_associate";
  if (int rc = check_common(ctx, who, n_img, line_off, lines, pt_off, pts, cfg)) return rc;
  const long long nl = line_off[n_img], np = pt_off[n_img];
  if (nl >= (1ll << 31) || np >= (1ll << 31)) return fail(ctx, LT_ERR_ARGUMENT, std::string(who) + ": too many items");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  ctx->bp.edge_off.assign((size_t)np + 1, 0);
  ctx->bp.edge.clear();
  double t0 = now_ms();
  if (int rc = upload_scene(ctx, n_img, line_off, lines, pt_off, pts)) return rc;
  const std::vector<BptBlock> blocks = make_blocks(n_img, (const long long *)pt_off);
  if (int rc = upload_vec(ctx, ctx->bp.d_blk, blocks)) return rc;
  if (int rc = stream_sync(ctx)) return rc;
  double t1 = now_ms();
  ctx->bp.timers[0] = t1 - t0;
  ctx->bp.timers[2] = 0.0;
  std::vector<int> cnt;
  if (np > 0 && nl > 0) {
    ENSURE(ctx, ctx->bp.d_cnt, 4 * (size_t)np);
    launch_bpt_prep(st, ctx->bp.d_raw.as<double>(), nl, ctx->bp.d_lines.as<BptLine>());
    launch_bpt_assoc(st, 0, ctx->bp.d_blk.as<BptBlock>(), (int)blocks.size(), ctx->bp.d_off.as<long long>(),
                     ctx->bp.d_lines.as<BptLine>(), ctx->bp.d_pts.as<double>(), cfg->threshold_keypoints,
                     ctx->bp.d_cnt.as<int>(), nullptr, nullptr);
    if (int rc = download(ctx, cnt, ctx->bp.d_cnt.p, (size_t)np)) return rc;
    if (int rc = stream_sync(ctx)) return rc;
    ctx->bp.edge_off = scan(cnt);
    const long long ne = ctx->bp.edge_off.back();
    if (ne > 0) {
      if (int rc = upload_vec(ctx, ctx->bp.d_scan, ctx->bp.edge_off)) return rc;
      ENSURE(ctx, ctx->bp.d_out, 4 * (size_t)ne);
      launch_bpt_assoc(st, 1, ctx->bp.d_blk.as<BptBlock>(), (int)blocks.size(), ctx->bp.d_off.as<long long>(),
                       ctx->bp.d_lines.as<BptLine>(), ctx->bp.d_pts.as<double>(), cfg->threshold_keypoints, nullptr,
                       ctx->bp.d_scan.as<long long>(), ctx->bp.d_out.as<int>());
      if (int rc = stream_sync(ctx)) return rc;
    }
    double t2 = now_ms();
    ctx->bp.timers[1] = t2 - t1;
    if (int rc = download(ctx, ctx->bp.edge, ctx->bp.d_out.p, (size_t)ne)) return rc;
    if (int rc = stream_sync(ctx)) return rc;
    ctx->bp.timers[3] = now_ms() - t2;
  } else {
    ctx->bp.timers[1] = ctx->bp.timers[3] = 0.0;
  }
  if (n_edges) *n_edges = (int64_t)ctx->bp.edge.size();
  return LT_OK;
}

int lt_bpt_associate_get(lt_ctx *ctx, int64_t *edge_off, int32_t *edge_line) {
  if (!ctx) return LT_ERR_ARGUMENT;
  if (edge_off) std::copy(ctx->bp.edge_off.begin(), ctx->bp.edge_off.end(), edge_off);
  if (edge_line) std::copy(ctx->bp.edge.begin(), ctx->bp.edge.end(), edge_line);
  return LT_OK;
}

int lt_bpt_junctions(lt_ctx *ctx, int n_img, const int64_t *line_off, const double *lines, const int64_t *kp_off,
                     const double *kps, const lt_bpt_config *cfg, int64_t sizes[4]) {
  if (!ctx) return LT_ERR_ARGUMENT;
  const char *who = "lt_bpt_junctions";
  if (int rc = check_common(ctx, who, n_img, line_off, lines, kp_off, kps, cfg)) return rc;
  const long long nl = line_off[n_img], nk = kp_off[n_img];
  if (nl >= (1ll << 30) || nk >= (1ll << 31)) return fail(ctx, LT_ERR_ARGUMENT, std::string(who) + ": too many items");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const double th_m = cfg->threshold_merge_junctions;
  ctx->bp.junc_off.assign((size_t)n_img + 1, 0);
  ctx->bp.jid_off.assign(1, 0);
  ctx->bp.junc_xy.clear();
  ctx->bp.jid.clear();
  ctx->bp.cand_off.assign((size_t)n_img + 1, 0);
  ctx->bp.cand_xy.clear();
  ctx->bp.cand_lines.clear();
  ctx->bp.parents.clear();
  for (int k = 0; k < 4; ++k) ctx->bp.timers[k] = 0.0;
  if (sizes) sizes[0] = sizes[1] = sizes[2] = sizes[3] = 0;
  if (nl == 0) return LT_OK;  // images without lines have no junction (the reference's loops wrap around there)

  // ---- upload: lines, keypoints, the image of every line, the grid of every image ----
  double t0 = now_ms();
  if (int rc = upload_scene(ctx, n_img, line_off, lines, kp_off, kps)) return rc;
  std::vector<int> row_img((size_t)nl);
  std::vector<BptGrid> grid((size_t)n_img);
  for (int m = 0; m < n_img; ++m) {
    for (long long k = line_off[m]; k < line_off[m + 1]; ++k) row_img[(size_t)k] = m;
    grid[(size_t)m] = bpt_grid_of(lines + 4 * line_off[m], line_off[m + 1] - line_off[m], th_m);
  }
  if (int rc = upload_vec(ctx, ctx->bp.d_idx2, row_img)) return rc;
  if (int rc = upload_vec(ctx, ctx->bp.d_misc, grid)) return rc;
  if (int rc = stream_sync(ctx)) return rc;
  double t1 = now_ms();
  ctx->bp.timers[0] = t1 - t0;

  // ---- intersections: count, prefix sums, fill ----
  const long long *d_line_off = ctx->bp.d_off.as<long long>();
  BptLine *d_lines = ctx->bp.d_lines.as<BptLine>();
  ENSURE(ctx, ctx->bp.d_cnt, 4 * (size_t)nl + 4);
  int *d_flag = ctx->bp.d_cnt.as<int>() + nl;
  HIPCHK(ctx, hipMemsetAsync(d_flag, 0, 4, st));
  launch_bpt_prep(st, ctx->bp.d_raw.as<double>(), nl, d_lines);
  launch_bpt_intersect(st, 0, nl, ctx->bp.d_idx2.as<int>(), d_line_off, d_lines, cfg->threshold_intersection,
                       ctx->bp.d_cnt.as<int>(), nullptr, nullptr, d_flag);
  std::vector<int> cnt;
  if (int rc = download(ctx, cnt, ctx->bp.d_cnt.p, (size_t)nl)) return rc;
  if (int rc = stream_sync(ctx)) return rc;
  const std::vector<long long> row_off = scan(cnt);
  const long long n_inter = row_off.back();
  std::vector<long long> inter_off((size_t)n_img + 1), &cand_off = ctx->bp.cand_off;
  for (int m = 0; m <= n_img; ++m) {
    inter_off[(size_t)m] = row_off[(size_t)line_off[m]];
    cand_off[(size_t)m] = 2 * line_off[m] + inter_off[(size_t)m];
  }
  const long long n_cand = cand_off[(size_t)n_img];
  if (n_cand > kMaxCandidates)
    return fail(ctx, LT_ERR_ARGUMENT, std::string(who) + ": more than 2^32 - 1 junction candidates in one call");
  ENSURE(ctx, ctx->bp.d_inter, sizeof(BptInter) * (size_t)std::max<long long>(n_inter, 1));
  if (n_inter > 0) {
    if (int rc = upload_vec(ctx, ctx->bp.d_scan, row_off)) return rc;
    launch_bpt_intersect(st, 1, nl, ctx->bp.d_idx2.as<int>(), d_line_off, d_lines, cfg->threshold_intersection, nullptr,
                         ctx->bp.d_scan.as<long long>(), ctx->bp.d_inter.as<BptInter>(), d_flag);
  }
  // ---- candidates and their cells ----
  if (int rc = upload_vec(ctx, ctx->bp.d_off3, cand_off)) return rc;
  if (int rc = upload_vec(ctx, ctx->bp.d_blk, inter_off)) return rc;
  ENSURE(ctx, ctx->bp.d_cand, 16 * (size_t)n_cand);
  ENSURE(ctx, ctx->bp.d_keys, 8 * (size_t)n_cand);
  ENSURE(ctx, ctx->bp.d_keys2, 8 * (size_t)n_cand);
  ENSURE(ctx, ctx->bp.d_idx, 4 * (size_t)n_cand);
  ENSURE(ctx, ctx->bp.d_out, 4 * (size_t)n_cand);
  launch_bpt_candidates(st, n_img, n_cand, ctx->bp.d_off3.as<long long>(), d_line_off, ctx->bp.d_blk.as<long long>(),
                        d_lines, ctx->bp.d_inter.as<BptInter>(), ctx->bp.d_misc.as<BptGrid>(),
                        ctx->bp.d_cand.as<double>(), ctx->bp.d_keys.as<unsigned long long>(),
                        ctx->bp.d_idx.as<unsigned>());
  int flag = 0;
  HIPCHK(ctx, hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, st));
  if (int rc = stream_sync(ctx)) return rc;
  if (flag)
    return fail(ctx, LT_ERR_ARGUMENT,
                std::string(who) + ": an intersection has a non-finite coordinate (the reference's result is undefined)");
  double t2 = now_ms();
  ctx->bp.timers[1] = t2 - t1;
  // ---- candidates into cell order ----
  size_t tmp = bpt_sort_pairs_temp_bytes(n_cand);
  ENSURE(ctx, ctx->bp.d_tmp, std::max<size_t>(tmp, 16));
  if (launch_bpt_sort_pairs(st, ctx->bp.d_tmp.p, tmp, n_cand, ctx->bp.d_keys.as<unsigned long long>(),
                            ctx->bp.d_keys2.as<unsigned long long>(), ctx->bp.d_idx.as<unsigned>(),
                            ctx->bp.d_out.as<unsigned>()) != 0)
    return fail(ctx, LT_ERR_HIP, "rocprim radix sort failed");
  if (int rc = stream_sync(ctx)) return rc;
  double t3 = now_ms();
  ctx->bp.timers[2] = t3 - t2;
  // ---- close pairs: count, prefix sums, fill ----
  const unsigned long long *d_skeys = ctx->bp.d_keys2.as<unsigned long long>();
  const unsigned *d_sidx = ctx->bp.d_out.as<unsigned>();
  ENSURE(ctx, ctx->bp.d_cnt, 4 * (size_t)n_cand);
  launch_bpt_close_pairs(st, 0, n_cand, d_skeys, d_sidx, ctx->bp.d_cand.as<double>(), th_m, ctx->bp.d_cnt.as<int>(),
                         nullptr, nullptr);
  if (int rc = download(ctx, cnt, ctx->bp.d_cnt.p, (size_t)n_cand)) return rc;
  if (int rc = stream_sync(ctx)) return rc;
  const std::vector<long long> pair_off = scan(cnt);
  const long long n_pairs = pair_off.back();
  if (n_pairs > kMaxPairs)
    return fail(ctx, LT_ERR_ARGUMENT, std::string(who) + ": more than 2^31 junction candidates pairs within the threshold");
  std::vector<unsigned long long> pairs;
  double t4 = now_ms();
  if (n_pairs > 0) {
    if (int rc = upload_vec(ctx, ctx->bp.d_scan, pair_off)) return rc;
    ENSURE(ctx, ctx->bp.d_keys, 8 * (size_t)n_pairs);  // (the unsorted candidate keys are no longer needed)
    ENSURE(ctx, ctx->bp.d_raw, 8 * (size_t)n_pairs);   // (nor the raw lines)
    launch_bpt_close_pairs(st, 1, n_cand, d_skeys, d_sidx, ctx->bp.d_cand.as<double>(), th_m, nullptr,
                           ctx->bp.d_scan.as<long long>(), ctx->bp.d_keys.as<unsigned long long>());
    if (int rc = stream_sync(ctx)) return rc;
    t4 = now_ms();
    tmp = bpt_sort_keys_temp_bytes(n_pairs);
    ENSURE(ctx, ctx->bp.d_tmp, std::max<size_t>(tmp, 16));
    if (launch_bpt_sort_keys(st, ctx->bp.d_tmp.p, tmp, n_pairs, ctx->bp.d_keys.as<unsigned long long>(),
                             ctx->bp.d_raw.as<unsigned long long>()) != 0)
      return fail(ctx, LT_ERR_HIP, "rocprim radix sort failed");
    if (int rc = stream_sync(ctx)) return rc;
  }
  double t5 = now_ms();
  ctx->bp.timers[1] += t4 - t3;
  ctx->bp.timers[2] += t5 - t4;
  // ---- download the pairs and the candidates ----
  if (int rc = download(ctx, pairs, ctx->bp.d_raw.p, (size_t)n_pairs)) return rc;
  if (int rc = download(ctx, ctx->bp.cand_xy, ctx->bp.d_cand.p, 2 * (size_t)n_cand)) return rc;
  std::vector<BptInter> inter;
  if (int rc = download(ctx, inter, ctx->bp.d_inter.p, (size_t)n_inter)) return rc;
  if (int rc = stream_sync(ctx)) return rc;

  // ---- host: the union-find of :128-143 over the close pairs, the clusters of :144-151, merge_junctions ----
  ctx->bp.cand_lines.assign(2 * (size_t)n_cand, -1);
  ctx->bp.parents.assign((size_t)n_cand, -1);
  std::vector<long long> pair_img_off((size_t)n_img + 1, 0);  // the pairs of an image are consecutive
  {
    size_t k = 0;
    for (int m = 0; m < n_img; ++m) {
      pair_img_off[(size_t)m] = (long long)k;
      while (k < pairs.size() && (long long)(pairs[k] >> 32) < cand_off[(size_t)m + 1]) ++k;
    }
    pair_img_off[(size_t)n_img] = (long long)pairs.size();
  }
  struct ImgOut {
    std::vector<double> xy;
    std::vector<long long> id_off;
    std::vector<int> ids;
  };
  std::vector<ImgOut> merged((size_t)n_img);
#pragma omp parallel for schedule(dynamic, 1)
  for (int m = 0; m < n_img; ++m) {
    const long long c0 = cand_off[(size_t)m], J = cand_off[(size_t)m + 1] - c0;
    const long long M = line_off[m + 1] - line_off[m];
    if (J == 0) continue;
    int *cl = ctx->bp.cand_lines.data() + 2 * c0;
    for (long long k = 0; k < 2 * M; ++k) cl[2 * k] = (int)(k >> 1);
    for (long long k = 2 * M; k < J; ++k) {
      const BptInter &I = inter[(size_t)(inter_off[(size_t)m] + k - 2 * M)];
      cl[2 * k] = I.l1;
      cl[2 * k + 1] = I.l2;
    }
    std::vector<int> parents((size_t)J, -1);  // union_find_get_root (base/graph.cc:157-166) is uf_root (lt_tail.h)
    for (long long q = pair_img_off[(size_t)m]; q < pair_img_off[(size_t)m + 1]; ++q) {
      const int i = (int)((long long)(pairs[(size_t)q] >> 32) - c0);
      const int j = (int)((long long)(pairs[(size_t)q] & 0xffffffffull) - c0);
      const int ri = uf_root(i, parents), rj = uf_root(j, parents);
      if (ri == rj) continue;
      parents[(size_t)j] = i;  // `if (i < j) parents[j] = i;`: j itself, not its root
    }
    std::vector<int> root((size_t)J), size((size_t)J, 0);
    for (long long k = 0; k < J; ++k) size[(size_t)(root[(size_t)k] = uf_root((int)k, parents))]++;
    std::copy(parents.begin(), parents.end(), ctx->bp.parents.begin() + c0);
    // the members of each cluster in candidate order (a root is the smallest index of its cluster)
    std::vector<long long> start((size_t)J + 1, 0);
    for (long long k = 0; k < J; ++k) start[(size_t)k + 1] = start[(size_t)k] + size[(size_t)k];
    std::vector<int> member((size_t)J);
    {
      std::vector<long long> fillp(start.begin(), start.end() - 1);
      for (long long k = 0; k < J; ++k) member[(size_t)fillp[(size_t)root[(size_t)k]]++] = (int)k;
    }
    ImgOut &o = merged[(size_t)m];
    o.id_off.push_back(0);
    std::vector<int> ids;
    const double *xy = ctx->bp.cand_xy.data() + 2 * c0;
    for (long long r = 0; r < J; ++r) {
      const int n = size[(size_t)r];
      if (n == 0) continue;
      double px = 0.0, py = 0.0;
      ids.clear();
      for (long long q = start[(size_t)r]; q < start[(size_t)r + 1]; ++q) {
        const int k = member[(size_t)q];
        px += xy[2 * k];
        py += xy[2 * k + 1];
        ids.push_back(cl[2 * k]);
        if (cl[2 * k + 1] >= 0) ids.push_back(cl[2 * k + 1]);
      }
      px /= (double)n;
      py /= (double)n;
      std::sort(ids.begin(), ids.end());
      ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
      o.xy.push_back(px);
      o.xy.push_back(py);
      o.ids.insert(o.ids.end(), ids.begin(), ids.end());
      o.id_off.push_back((long long)o.ids.size());
    }
  }
  std::vector<long long> mj_off((size_t)n_img + 1, 0);
  for (int m = 0; m < n_img; ++m) mj_off[(size_t)m + 1] = mj_off[(size_t)m] + (long long)merged[(size_t)m].xy.size() / 2;
  const long long n_mj = mj_off[(size_t)n_img];
  std::vector<double> mj_xy(2 * (size_t)n_mj);
  for (int m = 0; m < n_img; ++m)
    std::copy(merged[(size_t)m].xy.begin(), merged[(size_t)m].xy.end(), mj_xy.begin() + 2 * mj_off[(size_t)m]);
  if (int rc = check_finite(ctx, who, mj_xy.data(), (long long)mj_xy.size(), "merged junction")) return rc;
  double t6 = now_ms();
  ctx->bp.timers[3] = t6 - t5;

  // ---- the nearest keypoint of every merged junction (:155-161) ----
  std::vector<double> dist((size_t)n_mj, DBL_MAX);
  if (nk > 0 && n_mj > 0) {
    const std::vector<BptBlock> blocks = make_blocks(n_img, mj_off.data());
    if (int rc = upload_vec(ctx, ctx->bp.d_blk, blocks)) return rc;
    if (int rc = upload_vec(ctx, ctx->bp.d_cand, mj_xy)) return rc;
    ENSURE(ctx, ctx->bp.d_keys2, 8 * (size_t)n_mj);
    launch_bpt_nearest(st, ctx->bp.d_blk.as<BptBlock>(), (int)blocks.size(), ctx->bp.d_off2.as<long long>(),
                       ctx->bp.d_pts.as<double>(), ctx->bp.d_cand.as<double>(), ctx->bp.d_keys2.as<double>());
    if (int rc = download(ctx, dist, ctx->bp.d_keys2.p, (size_t)n_mj)) return rc;
    if (int rc = stream_sync(ctx)) return rc;
  }
  double t7 = now_ms();
  ctx->bp.timers[1] += t7 - t6;
  for (int m = 0; m < n_img; ++m) {
    const ImgOut &o = merged[(size_t)m];
    const bool has_kp = kp_off[m + 1] > kp_off[m];  // `if (!tree.empty())`
    for (size_t q = 0; q + 1 < o.id_off.size(); ++q) {
      if (has_kp && dist[(size_t)mj_off[(size_t)m] + q] < th_m) continue;
      ctx->bp.junc_xy.push_back(o.xy[2 * q]);
      ctx->bp.junc_xy.push_back(o.xy[2 * q + 1]);
      ctx->bp.jid.insert(ctx->bp.jid.end(), o.ids.begin() + o.id_off[q], o.ids.begin() + o.id_off[q + 1]);
      ctx->bp.jid_off.push_back((long long)ctx->bp.jid.size());
    }
    ctx->bp.junc_off[(size_t)m + 1] = (long long)ctx->bp.junc_xy.size() / 2;
  }
  ctx->bp.timers[3] += now_ms() - t7;
  if (sizes) {
    sizes[0] = (int64_t)ctx->bp.junc_xy.size() / 2;
    sizes[1] = (int64_t)ctx->bp.jid.size();
    sizes[2] = (int64_t)n_cand;
    sizes[3] = (int64_t)n_pairs;
  }
  return LT_OK;
}

int lt_bpt_junctions_get(lt_ctx *ctx, int64_t *junc_off, double *junc_xy, int64_t *id_off, int32_t *line_idx) {
  if (!ctx) return LT_ERR_ARGUMENT;
  if (junc_off) std::copy(ctx->bp.junc_off.begin(), ctx->bp.junc_off.end(), junc_off);
  if (junc_xy) std::copy(ctx->bp.junc_xy.begin(), ctx->bp.junc_xy.end(), junc_xy);
  if (id_off) std::copy(ctx->bp.jid_off.begin(), ctx->bp.jid_off.end(), id_off);
  if (line_idx) std::copy(ctx->bp.jid.begin(), ctx->bp.jid.end(), line_idx);
  return LT_OK;
}

int lt_bpt_junctions_get_candidates(lt_ctx *ctx, int64_t *cand_off, double *cand_xy, int32_t *cand_lines,
                                    int32_t *parents) {
  if (!ctx) return LT_ERR_ARGUMENT;
  if (cand_off) std::copy(ctx->bp.cand_off.begin(), ctx->bp.cand_off.end(), cand_off);
  if (cand_xy) std::copy(ctx->bp.cand_xy.begin(), ctx->bp.cand_xy.end(), cand_xy);
  if (cand_lines) std::copy(ctx->bp.cand_lines.begin(), ctx->bp.cand_lines.end(), cand_lines);
  if (parents) std::copy(ctx->bp.parents.begin(), ctx->bp.parents.end(), parents);
  return LT_OK;
}

int lt_fn_bpt_grid_keys(int img, int64_t n_lines, const double *lines4, double th_merge, int64_t n_pts, const double *xy,
                        double grid_out[3], uint64_t *keys_out) {
  if (img < 0 || img >= kMaxImages || n_lines < 0 || n_pts < 0 || (n_lines > 0 && !lines4) || (n_pts > 0 && !xy) ||
      (n_pts > 0 && !keys_out) || std::isnan(th_merge))
    return LT_ERR_ARGUMENT;
  for (int64_t k = 0; k < 4 * n_lines; ++k)
    if (!std::isfinite(lines4[k])) return LT_ERR_ARGUMENT;
  for (int64_t k = 0; k < 2 * n_pts; ++k)
    if (!std::isfinite(xy[k])) return LT_ERR_ARGUMENT;
  const BptGrid g = bpt_grid_of(lines4, n_lines, th_merge);
  if (grid_out) {
    grid_out[0] = g.lox;
    grid_out[1] = g.loy;
    grid_out[2] = g.cell;
  }
  for (int64_t k = 0; k < n_pts; ++k) keys_out[k] = bpt_key_of(img, xy[2 * k], xy[2 * k + 1], g);
  return LT_OK;
}

int lt_fn_bpt_close_pairs_host(int64_t n, const uint64_t *keys, const double *xy, double th_merge, int64_t cap,
                               uint64_t *pairs_out, int64_t *n_pairs) {
  if (n < 0 || n > kMaxCandidates || cap < 0 || (n > 0 && (!keys || !xy)) || (cap > 0 && !pairs_out) || !n_pairs ||
      std::isnan(th_merge))
    return LT_ERR_ARGUMENT;
  std::vector<unsigned> idx((size_t)n);
  for (int64_t k = 0; k < n; ++k) idx[(size_t)k] = (unsigned)k;
  std::stable_sort(idx.begin(), idx.end(), [&](unsigned a, unsigned b) { return keys[a] < keys[b]; });
  std::vector<unsigned long long> skeys((size_t)n);
  for (int64_t k = 0; k < n; ++k) skeys[(size_t)k] = keys[idx[(size_t)k]];
  std::vector<int> cnt((size_t)n, 0);  // two passes, as on the device: count, prefix sums, fill
  for (int64_t s = 0; s < n; ++s)
    cnt[idx[(size_t)s]] = bpt_close_pairs_of(n, skeys.data(), idx.data(), xy, th_merge, s, nullptr);
  const std::vector<long long> off = scan(cnt);
  std::vector<unsigned long long> pairs((size_t)off.back());
  for (int64_t s = 0; s < n; ++s)
    bpt_close_pairs_of(n, skeys.data(), idx.data(), xy, th_merge, s, pairs.data() + off[idx[(size_t)s]]);
  std::sort(pairs.begin(), pairs.end());
  *n_pairs = (int64_t)pairs.size();
  std::copy(pairs.begin(), pairs.begin() + std::min<int64_t>(cap, (int64_t)pairs.size()), pairs_out);
  return LT_OK;
}

int lt_bpt_get_timers(lt_ctx *ctx, double out[4]) {
  if (!ctx || !out) return LT_ERR_ARGUMENT;
  for (int k = 0; k < 4; ++k) out[k] = ctx->bp.timers[k];
  return LT_OK;
}

}  // extern "C"
