// lt_vp.cpp -- limap.vplib's JLinkage detector (vplib/JLinkage/JLinkage.cc, vplib/base_vp_detector.cc) for a batch of
// images per call.  The two calls upstream makes into its J-Linkage third party (random sampling of 5000 hypotheses,
// agglomerative clustering) are replaced by this project's deterministic definition: on the device
// (lt_vp_detect: lt_kernels_vp.hip) and, with the same inline expressions and the same total order, on the host
// (lt_fn_vp_detect_host).  Everything around the two calls is limap's own code and is restated here in its operation
// order: the length filter and the guard of ComputeVPLabels, the cluster filter with count_valid_supports_2d, the
// compaction of the labels, fitVP through lt_svd.h, AssociateVPs.

#include "lt_host.h"
#include "lt_geom.h"
#include "lt_svd.h"
#include "lt_vp.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include <omp.h>

using namespace lt;
using namespace lt_impl;

namespace {

// JLinkage declares a `config_` of its own (JLinkage.h:31) next to the one of BaseVPDetector (base_vp_detector.h:42);
// its constructors fill only the former, and count_valid_supports_2d (base_vp_detector.cc:62) reads the latter: the
// threshold there is always the default, whatever th_perp_supports the caller configured
constexpr double kThPerpSupportsUsed = 3.0;

int check_config(const lt_vp_config *cfg, std::string &msg) {
  if (!cfg) { msg = "null configuration"; return 1; }
  if (std::isnan(cfg->min_length) || std::isnan(cfg->inlier_threshold) || std::isnan(cfg->th_perp_supports)) {
    msg = "a threshold is NaN";
    return 1;
  }
  if (cfg->min_num_supports < 3 || cfg->min_num_supports > (1 << 20)) {
    msg = "min_num_supports outside [3, 2^20] (fitVP takes the third right singular vector: it needs three lines)";
    return 1;
  }
  if (cfg->num_hypotheses < 1 || cfg->num_hypotheses > kVpMaxHypotheses) {
    msg = "num_hypotheses outside [1, 2^20]";
    return 1;
  }
  return 0;
}

int check_lines(int n_img, const int64_t *line_off, const double *lines, std::string &msg) {
  if (n_img < 0) { msg = "bad image count"; return 1; }
  msg = offsets_msg("line", n_img, line_off);
  if (!msg.empty()) return 1;
  for (int m = 0; m < n_img; ++m)
    if (line_off[m + 1] - line_off[m] > INT_MAX / 2) { msg = "too many lines in an image"; return 1; }
  if (line_off[n_img] > 0 && !lines) { msg = "null coordinates"; return 1; }
  if (!all_finite(lines, 4 * line_off[n_img])) { msg = "non-finite line coordinate"; return 1; }
  return 0;
}

inline size_t guard_of(const lt_vp_config &cfg) { return 2 * (size_t)std::max(cfg.min_num_supports, 10); }  // JLinkage.cc:37

// ---- the clustering on the host: same order, same records as k_vp_cluster; P row-major (n x W) ----
void cluster_host(int n, int W, uint64_t *P, int *roots) {
  std::vector<int> psize((size_t)n), nn((size_t)n, -1), ni((size_t)n, 0), nu((size_t)n, 1), parent((size_t)n, -1);
  auto inter = [&](int a, int b) {
    const uint64_t *pa = P + (size_t)a * W, *pb = P + (size_t)b * W;
    int c = 0;
    for (int w = 0; w < W; ++w) c += __builtin_popcountll(pa[w] & pb[w]);
    return c;
  };
  auto scan_row = [&](int row) {
    int bc = 0, bu = 1, bj = INT_MAX;
    const int sz = psize[(size_t)row];
    if (sz > 0)
      for (int k = row + 1; k < n; ++k) {
        const int sk = psize[(size_t)k];
        if (sk <= 0) continue;
        const int c = inter(row, k);
        if (c > 0 && vp_better(c, sz + sk - c, row, k, bc, bu, row, bj)) { bc = c; bu = sz + sk - c; bj = k; }
      }
    nn[(size_t)row] = bc > 0 ? bj : -1;
    ni[(size_t)row] = bc;
    nu[(size_t)row] = bu;
  };
  for (int k = 0; k < n; ++k) {
    int c = 0;
    for (int w = 0; w < W; ++w) c += __builtin_popcountll(P[(size_t)k * W + w]);
    psize[(size_t)k] = c;
  }
  for (int row = 0; row < n; ++row) scan_row(row);
  for (;;) {
    int bc = 0, bu = 1, bi = INT_MAX, bj = INT_MAX;
    for (int k = 0; k < n; ++k)
      if (psize[(size_t)k] > 0 && nn[(size_t)k] >= 0 &&
          vp_better(ni[(size_t)k], nu[(size_t)k], k, nn[(size_t)k], bc, bu, bi, bj)) {
        bc = ni[(size_t)k]; bu = nu[(size_t)k]; bi = k; bj = nn[(size_t)k];
      }
    if (bc <= 0) break;
    const int i = bi, j = bj;
    for (int w = 0; w < W; ++w) P[(size_t)i * W + w] &= P[(size_t)j * W + w];
    psize[(size_t)i] = bc;
    psize[(size_t)j] = -1;
    parent[(size_t)j] = i;
    int mc = 0, mu = 1, mj = INT_MAX;
    for (int k = 0; k < n; ++k) {
      const int sk = psize[(size_t)k];
      if (sk < 0 || k == i) continue;
      const int p = nn[(size_t)k];
      const bool again = k < j && (p == i || p == j);
      if (again) nn[(size_t)k] = -2;
      if (sk == 0 || (again && k < i)) continue;
      const int c = inter(i, k);
      if (c <= 0) continue;
      const int u = bc + sk - c;
      if (k < i) {
        if (p < 0 || vp_better(c, u, k, i, ni[(size_t)k], nu[(size_t)k], k, p)) {
          nn[(size_t)k] = i; ni[(size_t)k] = c; nu[(size_t)k] = u;
        }
      } else if (vp_better(c, u, i, k, mc, mu, i, mj)) {
        mc = c; mu = u; mj = k;
      }
    }
    nn[(size_t)i] = mc > 0 ? mj : -1;
    ni[(size_t)i] = mc;
    nu[(size_t)i] = mu;
    for (int row = 0; row < n; ++row)
      if (psize[(size_t)row] >= 0 && nn[(size_t)row] == -2) scan_row(row);
  }
  for (int k = 0; k < n; ++k) {
    int r = k;
    while (parent[(size_t)r] >= 0) r = parent[(size_t)r];
    roots[k] = r;
  }
}

// hypotheses, preference sets and clustering of one image on the host
void host_roots(const double *lines, const std::vector<int> &valid, const lt_vp_config &cfg, std::vector<int> &roots) {
  const int n = (int)valid.size(), M = cfg.num_hypotheses, W = (M + 63) / 64;
  std::vector<VpLine> vl((size_t)n);
  for (int k = 0; k < n; ++k) {
    const double *l = lines + 4 * (size_t)valid[(size_t)k];
    vl[(size_t)k] = vp_line(l[0], l[1], l[2], l[3]);
  }
  std::vector<VpHyp> hyp((size_t)M);
  for (int m = 0; m < M; ++m) {
    unsigned a, b;
    vp_sample(cfg.seed, (unsigned long long)m, (unsigned)n, &a, &b);
    hyp[(size_t)m] = vp_hypothesis(vl[a], vl[b]);
  }
  std::vector<uint64_t> P((size_t)n * W, 0ull);
  for (int k = 0; k < n; ++k) {
    const VpLine &l = vl[(size_t)k];
    for (int m = 0; m < M; ++m)
      if (vp_inlier(l.x1, l.y1, l.cx, l.cy, hyp[(size_t)m], cfg.inlier_threshold))
        P[(size_t)k * W + (m >> 6)] |= 1ull << (m & 63);
  }
  roots.resize((size_t)n);
  cluster_host(n, W, P.data(), roots.data());
}

// ---- limap's own tail ----
inline d3 line_coords(const double *l) {  // Line2d::coords() (linebase.cc:35-39)
  return unit(cross(mk3(l[0], l[1], 1.0), mk3(l[2], l[3], 1.0)));
}

// InfiniteLine2d(line).point_distance(q) (infinite_line.cc:9-33); false where a check of the reference throws
bool inf_line_distance(const double *line, double qx, double qy, double *out) {
  const d3 co = line_coords(line);
  const d2 direc = unit(mk2(co.y, -co.x));           // direction()
  const d2 dp = mk2(direc.y, -direc.x);              // the perpendicular through q
  if (!(std::fabs(std::sqrt(sqn(dp)) - 1.0) < kEps)) return false;  // THROW_CHECK_LT(|direc.norm() - 1|, EPS)
  const d3 cp = unit(mk3(dp.y, (-1) * dp.x, (-1) * dp.y * qx + dp.x * qy));
  const d3 ph = cross(co, cp);
  if (!(ph.z > kEps)) return false;                  // THROW_CHECK_GT(p_homo(2), EPS)
  const double den = ph.z + kEps;                    // dehomogeneous
  const double ux = qx - ph.x / den, uy = qy - ph.y / den;
  *out = std::sqrt(ux * ux + uy * uy);
  return true;
}

// count_valid_supports_2d (base_vp_detector.cc:41-73) over the lines ids[] of an image; -1 where the reference throws
int count_valid_supports(const double *lines, const std::vector<int> &ids, double th) {
  const size_t n = ids.size();
  std::vector<int> parents(n, -1);  // union_find_get_root (base/graph.cc:157-166) is uf_root (lt_tail.h)
  std::vector<double> len(n);
  for (size_t k = 0; k < n; ++k) {
    const double *l = lines + 4 * (size_t)ids[k];
    len[k] = vp_length(l[0], l[1], l[2], l[3]);
  }
  for (size_t i = 0; i + 1 < n; ++i) {
    const int root_i = uf_root((int)i, parents);
    for (size_t j = i + 1; j < n; ++j) {
      const int root_j = uf_root((int)j, parents);
      if (root_j == root_i) continue;
      size_t k1 = i, k2 = j;  // the shorter line is projected on the longer one
      if (len[i] > len[j]) { k1 = j; k2 = i; }
      if (!(len[k2] > 0.0)) return -1;  // CHECK_GT(line.length(), 0.0) of InfiniteLine2d(line)
      const double *a = lines + 4 * (size_t)ids[k1], *b = lines + 4 * (size_t)ids[k2];
      double ds, de;
      if (!inf_line_distance(b, a[0], a[1], &ds) || !inf_line_distance(b, a[2], a[3], &de)) return -1;
      const double dist = dmax(ds, de);
      if (dist > th) continue;
      parents[(size_t)root_j] = root_i;
    }
  }
  int n_supports = 0;
  for (size_t k = 0; k < n; ++k) n_supports += parents[k] == -1;
  return n_supports;
}

struct ImgResult {
  std::vector<int> labels, clusters;  // per line of the image
  std::vector<double> vps;            // 3 per vanishing point
  int err = 0;
};

// ComputeVPLabels after the clustering (JLinkage.cc:55-83) and AssociateVPs (:102-127).  roots: per valid line the
// cluster it ended in (null: the guard returned early)
void tail_image(const double *lines, long long n_lines, const std::vector<int> &valid, const int *roots,
                const lt_vp_config &cfg, ImgResult &out, lt_svd::Scratch &sc) {
  out.labels.assign((size_t)n_lines, -1);
  out.clusters.assign((size_t)n_lines, -1);
  out.vps.clear();
  out.err = 0;
  if (n_lines == 0 || !roots) return;
  const size_t nv = valid.size();
  // Labels: the clusters renumbered in ascending id; LabelCount: their sizes
  std::vector<int> rank(nv, -1), lab(nv);
  int n_clusters = 0;
  for (size_t k = 0; k < nv; ++k) rank[(size_t)roots[k]] = 0;
  for (size_t k = 0; k < nv; ++k)
    if (rank[k] == 0) rank[k] = n_clusters++;
  std::vector<std::vector<int>> supports((size_t)n_clusters);
  for (size_t k = 0; k < nv; ++k) {
    lab[k] = rank[(size_t)roots[k]];
    out.clusters[(size_t)valid[k]] = lab[k];
    supports[(size_t)lab[k]].push_back(valid[k]);
  }
  std::vector<int> vp_ids((size_t)n_clusters, -1);
  int counter = 0;
  for (int c = 0; c < n_clusters; ++c) {
    if (supports[(size_t)c].size() < (size_t)cfg.min_num_supports) continue;
    const int n_sup = count_valid_supports(lines, supports[(size_t)c], kThPerpSupportsUsed);
    if (n_sup < 0) { out.err = 1; return; }
    if (n_sup < cfg.min_num_supports) continue;
    vp_ids[(size_t)c] = counter++;
  }
  for (size_t k = 0; k < nv; ++k)
    if (vp_ids[(size_t)lab[k]] >= 0) out.labels[(size_t)valid[k]] = vp_ids[(size_t)lab[k]];
  if (counter == 0) return;
  // fitVP (:86-100) over the supports in line order
  out.vps.assign(3 * (size_t)counter, 0.0);
  std::vector<std::vector<int>> sup((size_t)counter);
  for (long long k = 0; k < n_lines; ++k)
    if (out.labels[(size_t)k] >= 0) sup[(size_t)out.labels[(size_t)k]].push_back((int)k);
  lt_svd::Mat A, V;
  std::vector<double> sv;
  for (int v = 0; v < counter; ++v) {
    const int rows = (int)sup[(size_t)v].size();
    A.reset(rows, 3);
    for (int r = 0; r < rows; ++r) {
      const d3 co = line_coords(lines + 4 * (size_t)sup[(size_t)v][(size_t)r]);
      A(r, 0) = co.x; A(r, 1) = co.y; A(r, 2) = co.z;
    }
    lt_svd::jacobi_svd_thin_v(A, V, sv, sc);
    const d3 p = unit(mk3(V(0, 2), V(1, 2), V(2, 2)));
    out.vps[3 * (size_t)v] = p.x; out.vps[3 * (size_t)v + 1] = p.y; out.vps[3 * (size_t)v + 2] = p.z;
  }
}

// the valid lines of every image from the flags of the length filter; active: the image passes the guard
void plan_images(int n_img, const int64_t *line_off, const unsigned char *flag, const lt_vp_config &cfg,
                 std::vector<std::vector<int>> &valid, std::vector<char> &active) {
  valid.assign((size_t)n_img, {});
  active.assign((size_t)n_img, 0);
  for (int m = 0; m < n_img; ++m) {
    for (long long k = line_off[m]; k < line_off[m + 1]; ++k)
      if (flag[k]) valid[(size_t)m].push_back((int)(k - line_off[m]));
    active[(size_t)m] = !(valid[(size_t)m].size() < guard_of(cfg));
  }
}

void gather(int n_img, const int64_t *line_off, const std::vector<ImgResult> &res, std::vector<int> &labels,
            std::vector<int> &clusters, std::vector<long long> &vp_off, std::vector<double> &vps) {
  labels.assign((size_t)line_off[n_img], -1);
  clusters.assign((size_t)line_off[n_img], -1);
  vp_off.assign((size_t)n_img + 1, 0);
  vps.clear();
  for (int m = 0; m < n_img; ++m) {
    std::copy(res[(size_t)m].labels.begin(), res[(size_t)m].labels.end(), labels.begin() + line_off[m]);
    std::copy(res[(size_t)m].clusters.begin(), res[(size_t)m].clusters.end(), clusters.begin() + line_off[m]);
    vps.insert(vps.end(), res[(size_t)m].vps.begin(), res[(size_t)m].vps.end());
    vp_off[(size_t)m + 1] = (long long)vps.size() / 3;
  }
}

const char *kThrowMsg =
    ": a check of InfiniteLine2d fails on a support line (zero length, or coordinates beyond its EPS tests)";

}  // namespace

extern "C" {

void lt_vp_config_default(lt_vp_config *cfg) {
  if (!cfg) return;
  cfg->min_length = 40.0;  // vplib/base_vp_detector.h:31-34
  cfg->inlier_threshold = 1.0;
  cfg->th_perp_supports = 3.0;
  cfg->min_num_supports = 5;
  cfg->num_hypotheses = 5000;  // JLinkage.cc:44
  cfg->seed = 0;
}

int lt_vp_detect(lt_ctx *ctx, int n_img, const int64_t *line_off, const double *lines, const lt_vp_config *cfg,
                 int64_t *n_vps) {
  if (!ctx) return LT_ERR_ARGUMENT;
  const std::string who = "lt_vp_detect";
  std::string msg;
  if (check_config(cfg, msg) || check_lines(n_img, line_off, lines, msg)) return fail(ctx, LT_ERR_ARGUMENT, who + ": " + msg);
  const long long nl = line_off[n_img];
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  for (int k = 0; k < 6; ++k) ctx->vp.timers[k] = 0.0;
  ctx->vp.labels.assign((size_t)nl, -1);
  ctx->vp.clusters.assign((size_t)nl, -1);
  ctx->vp.vp_off.assign((size_t)n_img + 1, 0);
  ctx->vp.vps.clear();
  if (n_vps) *n_vps = 0;
  if (nl == 0) return LT_OK;
  const char *too_large = ": the scene is too large for one call (split the images)";
  if (!vp_launch_fits((nl + kVpBlock - 1) / kVpBlock, kVpBlock)) return fail(ctx, LT_ERR_ARGUMENT, who + too_large);

  // ---- upload, length filter ----
  double t0 = now_ms();
  ENSURE(ctx, ctx->vp.d_raw, 32 * (size_t)nl);
  ENSURE(ctx, ctx->vp.d_flag, (size_t)nl);
  HIPCHK(ctx, hipMemcpyAsync(ctx->vp.d_raw.p, lines, 32 * (size_t)nl, hipMemcpyHostToDevice, st));
  launch_vp_prep(st, ctx->vp.d_raw.as<double>(), nl, cfg->min_length, ctx->vp.d_flag.as<unsigned char>());
  std::vector<unsigned char> flag((size_t)nl);
  HIPCHK(ctx, hipMemcpyAsync(flag.data(), ctx->vp.d_flag.p, (size_t)nl, hipMemcpyDeviceToHost, st));
  if (int rc = stream_sync(ctx)) return rc;
  std::vector<std::vector<int>> valid;
  std::vector<char> active;
  plan_images(n_img, line_off, flag.data(), *cfg, valid, active);
  const int M = cfg->num_hypotheses, W = (M + 63) / 64;
  std::vector<VpImg> imgs;
  std::vector<int> act_img;
  std::vector<long long> src;
  std::vector<VpBlock> blocks;
  for (int m = 0; m < n_img; ++m) {
    if (!active[(size_t)m]) continue;
    const int n = (int)valid[(size_t)m].size();
    VpImg im;
    im.v0 = (long long)src.size();
    im.p0 = im.v0 * W;
    im.h0 = (long long)imgs.size() * M;
    im.n = n;
    im.pad_ = 0;
    for (int k0 = 0; k0 < n; k0 += kVpBlock)
      for (int w0 = 0; w0 < W; w0 += kVpPrefWords) blocks.push_back(VpBlock{(int)imgs.size(), k0, w0, 0});
    for (int k : valid[(size_t)m]) src.push_back(line_off[m] + k);
    act_img.push_back(m);
    imgs.push_back(im);
  }
  const long long nv = (long long)src.size();
  const int n_act = (int)imgs.size();
  std::vector<int> roots((size_t)nv);
  if (n_act > 0) {
    if (imgs.size() * (size_t)M > (size_t)1 << 31 || (size_t)nv * (size_t)W > (size_t)1 << 32 ||
        !vp_launch_fits((long long)blocks.size(), kVpBlock) || !vp_launch_fits(n_act, kVpClBlock) ||
        !vp_launch_fits((long long)n_act * ((M + kVpBlock - 1) / kVpBlock), kVpBlock))
      return fail(ctx, LT_ERR_ARGUMENT, who + too_large);
    if (int rc = upload_vec(ctx, ctx->vp.d_src, src)) return rc;
    if (int rc = upload_vec(ctx, ctx->vp.d_imgs, imgs)) return rc;
    if (int rc = upload_vec(ctx, ctx->vp.d_blk, blocks)) return rc;
    ENSURE(ctx, ctx->vp.d_lines, sizeof(VpLine) * (size_t)nv);
    ENSURE(ctx, ctx->vp.d_hyp, sizeof(VpHyp) * (size_t)n_act * (size_t)M);
    ENSURE(ctx, ctx->vp.d_pref, 8 * (size_t)nv * (size_t)W);
    ENSURE(ctx, ctx->vp.d_state, 4 * (size_t)kVpStateInts * (size_t)nv);
    ENSURE(ctx, ctx->vp.d_roots, 4 * (size_t)nv);
    if (int rc = stream_sync(ctx)) return rc;
  }
  double t1 = now_ms();
  ctx->vp.timers[0] = t1 - t0;

  // ---- kernels ----
  if (n_act > 0) {
    Events<3> ev;  // hypotheses done, preference sets done, clustering done
    if (int rc = ev.create(ctx)) return rc;
    launch_vp_lines(st, ctx->vp.d_raw.as<double>(), ctx->vp.d_src.as<long long>(), nv, ctx->vp.d_lines.as<VpLine>());
    launch_vp_hyp(st, ctx->vp.d_imgs.as<VpImg>(), n_act, M, cfg->seed, ctx->vp.d_lines.as<VpLine>(),
                  ctx->vp.d_hyp.as<VpHyp>());
    if (int rc = ev.record(ctx, 0)) return rc;
    launch_vp_pref(st, ctx->vp.d_blk.as<VpBlock>(), (int)blocks.size(), ctx->vp.d_imgs.as<VpImg>(), M, W,
                   cfg->inlier_threshold, ctx->vp.d_lines.as<VpLine>(), ctx->vp.d_hyp.as<VpHyp>(),
                   ctx->vp.d_pref.as<unsigned long long>());
    if (int rc = ev.record(ctx, 1)) return rc;
    launch_vp_cluster(st, ctx->vp.d_imgs.as<VpImg>(), n_act, W, ctx->vp.d_pref.as<unsigned long long>(),
                      ctx->vp.d_state.as<int>(), ctx->vp.d_roots.as<int>());
    if (int rc = ev.record(ctx, 2)) return rc;
    if (int rc = stream_sync(ctx)) return rc;
    ctx->vp.timers[4] = ev.ms(0, 1);
    ctx->vp.timers[5] = ev.ms(1, 2);
    double t2 = now_ms();
    ctx->vp.timers[1] = t2 - t1;
    HIPCHK(ctx, hipMemcpyAsync(roots.data(), ctx->vp.d_roots.p, 4 * (size_t)nv, hipMemcpyDeviceToHost, st));
    if (int rc = stream_sync(ctx)) return rc;
    ctx->vp.timers[2] = now_ms() - t2;
    for (int a = 0; a < n_act; ++a)
      for (int k = 0; k < imgs[(size_t)a].n; ++k) {
        const int r = roots[(size_t)(imgs[(size_t)a].v0 + k)];
        if (r < 0 || r >= imgs[(size_t)a].n) return fail(ctx, LT_ERR_RUNTIME, who + ": the clustering kernel returned a cluster out of range");
      }
  }

  // ---- limap's tail on the host ----
  double t3 = now_ms();
  std::vector<ImgResult> res((size_t)n_img);
  std::vector<long long> first((size_t)n_img, -1);
  for (int a = 0; a < n_act; ++a) first[(size_t)act_img[(size_t)a]] = imgs[(size_t)a].v0;
#pragma omp parallel
  {
    lt_svd::Scratch sc;
#pragma omp for schedule(dynamic, 1)
    for (int m = 0; m < n_img; ++m)
      tail_image(lines + 4 * line_off[m], line_off[m + 1] - line_off[m], valid[(size_t)m],
                 first[(size_t)m] >= 0 ? roots.data() + first[(size_t)m] : nullptr, *cfg, res[(size_t)m], sc);
  }
  for (int m = 0; m < n_img; ++m)
    if (res[(size_t)m].err) return fail(ctx, LT_ERR_ARGUMENT, who + kThrowMsg);
  gather(n_img, line_off, res, ctx->vp.labels, ctx->vp.clusters, ctx->vp.vp_off, ctx->vp.vps);
  ctx->vp.timers[3] = now_ms() - t3;
  if (n_vps) *n_vps = (int64_t)ctx->vp.vp_off.back();
  return LT_OK;
}

int lt_vp_get(lt_ctx *ctx, int32_t *labels, int64_t *vp_off, double *vps, int32_t *clusters) {
  if (!ctx) return LT_ERR_ARGUMENT;
  if (labels) std::copy(ctx->vp.labels.begin(), ctx->vp.labels.end(), labels);
  if (vp_off) std::copy(ctx->vp.vp_off.begin(), ctx->vp.vp_off.end(), vp_off);
  if (vps) std::copy(ctx->vp.vps.begin(), ctx->vp.vps.end(), vps);
  if (clusters) std::copy(ctx->vp.clusters.begin(), ctx->vp.clusters.end(), clusters);
  return LT_OK;
}

int lt_vp_get_timers(lt_ctx *ctx, double out[6]) {
  if (!ctx || !out) return LT_ERR_ARGUMENT;
  for (int k = 0; k < 6; ++k) out[k] = ctx->vp.timers[k];
  return LT_OK;
}

int lt_fn_vp_detect_host(int n_img, const int64_t *line_off, const double *lines, const lt_vp_config *cfg, int n_threads,
                         int32_t *labels, int64_t *vp_off, double *vps, int64_t vps_cap, int32_t *clusters) {
  std::string msg;
  if (check_config(cfg, msg) || check_lines(n_img, line_off, lines, msg) || !vp_off) return LT_ERR_ARGUMENT;
  const long long nl = line_off[n_img];
  std::vector<unsigned char> flag((size_t)nl);
  for (long long k = 0; k < nl; ++k)
    flag[(size_t)k] = vp_length(lines[4 * k], lines[4 * k + 1], lines[4 * k + 2], lines[4 * k + 3]) < cfg->min_length ? 0 : 1;
  std::vector<std::vector<int>> valid;
  std::vector<char> active;
  plan_images(n_img, line_off, flag.data(), *cfg, valid, active);
  std::vector<ImgResult> res((size_t)n_img);
  const int nt = n_threads > 0 ? n_threads : omp_get_max_threads();
#pragma omp parallel num_threads(nt)
  {
    lt_svd::Scratch sc;
    std::vector<int> roots;
#pragma omp for schedule(dynamic, 1)
    for (int m = 0; m < n_img; ++m) {
      const double *l = lines + 4 * line_off[m];
      if (active[(size_t)m]) host_roots(l, valid[(size_t)m], *cfg, roots);
      tail_image(l, line_off[m + 1] - line_off[m], valid[(size_t)m], active[(size_t)m] ? roots.data() : nullptr, *cfg,
                 res[(size_t)m], sc);
    }
  }
  for (int m = 0; m < n_img; ++m)
    if (res[(size_t)m].err) return LT_ERR_ARGUMENT;
  std::vector<int> lab, clu;
  std::vector<long long> off;
  std::vector<double> v;
  gather(n_img, line_off, res, lab, clu, off, v);
  if (off.back() > vps_cap) return LT_ERR_ARGUMENT;
  if (labels) std::copy(lab.begin(), lab.end(), labels);
  if (clusters) std::copy(clu.begin(), clu.end(), clusters);
  std::copy(off.begin(), off.end(), vp_off);
  if (vps) std::copy(v.begin(), v.end(), vps);
  return LT_OK;
}

int lt_vp_cluster_sets(lt_ctx *ctx, int n_img, const int64_t *row_off, int64_t n_words, const uint64_t *pref,
                       int32_t *roots) {
  if (!ctx) return LT_ERR_ARGUMENT;
  const std::string who = "lt_vp_cluster_sets";
  if (n_img < 0) return fail(ctx, LT_ERR_ARGUMENT, who + ": bad image count");
  if (int rc = check_offsets(ctx, who.c_str(), "row", n_img, row_off)) return rc;
  for (int m = 0; m < n_img; ++m)
    if (row_off[m + 1] - row_off[m] > INT_MAX / 2) return fail(ctx, LT_ERR_ARGUMENT, who + ": too many rows in an image");
  if (n_words < 1 || n_words > kVpMaxHypotheses / 64)
    return fail(ctx, LT_ERR_ARGUMENT, who + ": n_words outside [1, 2^14]");
  const long long nv = row_off[n_img];
  if (nv == 0) return LT_OK;
  if (!pref || !roots) return fail(ctx, LT_ERR_ARGUMENT, who + ": null preference sets or roots");
  const int W = (int)n_words;
  if ((size_t)nv * (size_t)W > (size_t)1 << 32 || !vp_launch_fits(n_img, kVpClBlock))
    return fail(ctx, LT_ERR_ARGUMENT, who + ": the scene is too large for one call (split the images)");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  // the VpImg table and the kernel's word-major layout (lt_vp.h), as lt_vp_detect leaves them for k_vp_cluster
  std::vector<VpImg> imgs((size_t)n_img);
  std::vector<unsigned long long> P((size_t)nv * (size_t)W);
  for (int m = 0; m < n_img; ++m) {
    VpImg &im = imgs[(size_t)m];
    im.v0 = row_off[m];
    im.p0 = im.v0 * W;
    im.h0 = 0;
    im.n = (int)(row_off[m + 1] - row_off[m]);
    im.pad_ = 0;
    for (int k = 0; k < im.n; ++k)
      for (int w = 0; w < W; ++w)
        P[(size_t)(im.p0 + (long long)w * im.n + k)] = pref[(size_t)(im.v0 + k) * (size_t)W + (size_t)w];
  }
  if (int rc = upload_vec(ctx, ctx->vp.d_imgs, imgs)) return rc;
  if (int rc = upload_vec(ctx, ctx->vp.d_pref, P)) return rc;
  ENSURE(ctx, ctx->vp.d_state, 4 * (size_t)kVpStateInts * (size_t)nv);
  ENSURE(ctx, ctx->vp.d_roots, 4 * (size_t)nv);
  launch_vp_cluster(st, ctx->vp.d_imgs.as<VpImg>(), n_img, W, ctx->vp.d_pref.as<unsigned long long>(),
                    ctx->vp.d_state.as<int>(), ctx->vp.d_roots.as<int>());
  HIPCHK(ctx, hipMemcpyAsync(roots, ctx->vp.d_roots.p, 4 * (size_t)nv, hipMemcpyDeviceToHost, st));
  if (int rc = stream_sync(ctx)) return rc;
  for (int m = 0; m < n_img; ++m)
    for (long long k = row_off[m]; k < row_off[m + 1]; ++k)
      if (roots[k] < 0 || roots[k] >= imgs[(size_t)m].n)
        return fail(ctx, LT_ERR_RUNTIME, who + ": the clustering kernel returned a cluster out of range");
  return LT_OK;
}

int lt_fn_vp_cluster_host(int64_t n, int64_t n_words, const uint64_t *pref, int32_t *roots) {
  if (n < 0 || n_words < 1 || n > INT_MAX / 2 || n_words > kVpMaxHypotheses / 64 || !roots || (n > 0 && !pref))
    return LT_ERR_ARGUMENT;
  std::vector<uint64_t> P(pref, pref + (size_t)n * (size_t)n_words);
  cluster_host((int)n, (int)n_words, P.data(), roots);
  return LT_OK;
}

}  // extern "C"
