// lt_refine.cpp -- the geometric refinement of line tracks with constant cameras: step [E] of
// limap.runners.line_triangulation (runners/line_triangulation.py:208-219; HybridBAEngine with set_constant_camera,
// optimize/hybrid_bundle_adjustment/hybrid_bundle_adjustment.cc:39-59,106-123,156-197,298-310) and the geometric terms
// of limap.optimize.line_refinement.  Validation, the residual order (AddLineGeometricResiduals: sorted image ids, then
// the id map's order within an image -- a stable sort of the supports by image id), upload, the three launches of
// lt_kernels_refine.hip and the download; lt_fn_refine_host is the whole step in plain C++ from the same inline functions
// (lt_refine.h) with the reductions in the device's order, so both agree bit for bit.

#include "lt_host.h"
#include "lt_refine.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <string>
#include <unordered_map>
#include <vector>

#include <omp.h>

using namespace lt;
using namespace lt_impl;

namespace {

struct Plan {
  std::vector<RfTrack> tracks;
  std::vector<int> sup_cam;    // residual order
  std::vector<double> l2d;     // 4 per support, residual order
  std::vector<double> l3d;     // 6 per support, list order
  std::vector<double> line6;
  long long n_sup = 0;
};

int check_config(const lt_refine_config *cfg, std::string &msg) {
  if (!cfg) { msg = "null configuration"; return 1; }
  if (!(cfg->geometric_alpha >= 0.0) || !(cfg->geometric_alpha <= 700.0)) { msg = "geometric_alpha outside [0, 700]"; return 1; }
  if (cfg->max_num_iterations < 0) { msg = "max_num_iterations is negative"; return 1; }
  return 0;
}

int check_cams(int n_img, const int32_t *ids, const double *k, const double *q, const double *t,
               std::unordered_map<int, int> &id2idx, std::string &msg) {
  if (n_img < 0 || (n_img > 0 && (!ids || !k || !q || !t))) { msg = "bad camera arrays"; return 1; }
  if (!all_finite(k, 4 * (size_t)n_img) || !all_finite(q, 4 * (size_t)n_img) || !all_finite(t, 3 * (size_t)n_img)) {
    msg = "non-finite camera";
    return 1;
  }
  for (int n = 0; n < n_img; ++n)
    if (!id2idx.emplace(ids[n], n).second) { msg = "image id " + std::to_string(ids[n]) + " appears twice"; return 1; }
  return 0;
}

// the checks upstream makes (or fails without) and the tables of the kernels
int make_plan(const std::unordered_map<int, int> &id2idx, int64_t T, const double *line6, const int64_t *off,
              const int32_t *img, const double *l2d4, const double *l3d6, const lt_refine_config &cfg, Plan &pl,
              std::string &msg) {
  if (T < 0 || !off || (T > 0 && !line6)) { msg = "bad track arrays"; return 1; }
  msg = offsets_msg("track", T, off);
  if (!msg.empty()) return 1;
  for (int64_t n = 0; n < T; ++n) {
    if (off[n + 1] <= off[n]) { msg = "track " + std::to_string(n) + " has no supports"; return 1; }  // THROW_CHECK_GT(line3ds.size(), 0)
    if (off[n + 1] - off[n] > (1 << 28)) { msg = "too many supports in a track"; return 1; }
  }
  const long long S = T > 0 ? off[T] : 0;
  if (S > 0 && (!img || !l2d4 || !l3d6)) { msg = "null support arrays"; return 1; }
  if (!all_finite(line6, 6 * (size_t)T) || !all_finite(l2d4, 4 * (size_t)S) || !all_finite(l3d6, 6 * (size_t)S)) {
    msg = "non-finite coordinate";
    return 1;
  }
  pl.n_sup = S;
  pl.tracks.resize((size_t)T);
  pl.sup_cam.resize((size_t)S);
  pl.l2d.resize(4 * (size_t)S);
  pl.l3d.assign(l3d6, l3d6 + 6 * (size_t)S);
  pl.line6.assign(line6, line6 + 6 * (size_t)T);
  std::vector<int> order, ids;
  for (int64_t n = 0; n < T; ++n) {
    const double *l = line6 + 6 * n;
    const double dx = l[0] - l[3], dy = l[1] - l[4], dz = l[2] - l[5];
    if (!(std::sqrt((dx * dx + dy * dy) + dz * dz) > 0.0)) {  // CHECK_GT(line.length(), 0.0) (infinite_line.cc:68)
      msg = "track " + std::to_string(n) + ": the line has zero length";
      return 1;
    }
    const long long a = off[n];
    const int K = (int)(off[n + 1] - a);
    // values[num_outliers] and values[2 K - 1 - num_outliers] (infinite_line.cc:284-285)
    if (cfg.num_outliers_aggregator < 0 || cfg.num_outliers_aggregator > 2 * K - 1) {
      msg = "num_outliers " + std::to_string(cfg.num_outliers_aggregator) + " leaves the " + std::to_string(2 * K) +
            " values of track " + std::to_string(n);
      return 1;
    }
    order.resize((size_t)K);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return img[a + x] < img[a + y]; });
    ids.assign(img + a, img + a + K);
    std::sort(ids.begin(), ids.end());
    const int n_images = (int)(std::unique(ids.begin(), ids.end()) - ids.begin());  // count_images()
    for (int k = 0; k < K; ++k) {
      const long long src = a + order[(size_t)k];
      auto it = id2idx.find(img[src]);
      if (it == id2idx.end()) {  // imagecols_.camview(img_id): std::map::at
        msg = "track " + std::to_string(n) + ": image id " + std::to_string(img[src]) + " is not in the collection";
        return 1;
      }
      pl.sup_cam[(size_t)(a + k)] = it->second;
      for (int c = 0; c < 4; ++c) pl.l2d[4 * (size_t)(a + k) + c] = l2d4[4 * src + c];
    }
    pl.tracks[(size_t)n] = RfTrack{a, K, (cfg.constant_line != 0 || n_images < cfg.min_num_images) ? 1 : 0};
  }
  return 0;
}

// ---- the host twin of a group of kRfWidth lanes ----
struct HostGroup {
  const double *tab;
  long long stride;
  const RfTrack &t;
  double alpha;
  double cost(const double p[6]) const {
    double dm[6];
    rf_plucker<double>(p, p + 4, dm);
    double part[kRfWidth][kRfSums];
    for (int l = 0; l < kRfWidth; ++l) {
      double s = 0.0;
      for (int k = l; k < t.n; k += kRfWidth) s = s + rf_cost_term(rf_load(tab, stride, t.s0 + k), dm, alpha);
      part[l][0] = s;
    }
    double out[kRfSums];
    rf_tree_host(part, 1, out);
    return 0.5 * out[0];
  }
  void linearise(const double p[6], double acc[kRfSums]) const {
    Rf4 u[4], w[2], dm[6];
    rf_seed(p, u, w);
    rf_plucker<Rf4>(u, w, dm);
    double part[kRfWidth][kRfSums];
    for (int l = 0; l < kRfWidth; ++l) {
      for (int c = 0; c < kRfSums; ++c) part[l][c] = 0.0;
      for (int k = l; k < t.n; k += kRfWidth) rf_accumulate(rf_load(tab, stride, t.s0 + k), dm, alpha, part[l]);
    }
    rf_tree_host(part, kRfSums, acc);
  }
};

// k_refine_cut on the host: the same rank rule
void cut_host(const RfTrack &t, const double *l3d, int num_outliers, RfOut &o) {
  d3 dir, m;
  rf_infinite(o.p, &dir, &m);
  const double *l3 = l3d + 6 * t.s0;
  const d3 pref = rf_pref(dir, m, mk3(l3[0], l3[1], l3[2]));
  const long long n = 2 * (long long)t.n, lo = num_outliers, hi = n - 1 - num_outliers;
  const double nan = std::nan("");
  for (int c = 0; c < 6; ++c) o.seg[c] = nan;
  for (long long i = 0; i < n; ++i) {
    double v;
    bool is_lo, is_hi;
    rf_rank_test(l3, n, i, pref, dir, lo, hi, &v, &is_lo, &is_hi);
    if (is_lo) { o.seg[0] = pref.x + dir.x * v; o.seg[1] = pref.y + dir.y * v; o.seg[2] = pref.z + dir.z * v; }
    if (is_hi) { o.seg[3] = pref.x + dir.x * v; o.seg[4] = pref.y + dir.y * v; o.seg[5] = pref.z + dir.z * v; }
  }
}

void run_host(const Plan &pl, const double *k, const double *q, const double *t, const lt_refine_config &cfg, int n_threads,
              std::vector<RfOut> &out) {
  const long long S = pl.n_sup, T = (long long)pl.tracks.size();
  const long long stride = std::max<long long>(S, 1);
  std::vector<double> tab((size_t)kRfFields * (size_t)stride);
  const int nt = n_threads > 0 ? n_threads : omp_get_max_threads();
#pragma omp parallel for num_threads(nt) schedule(static)
  for (long long i = 0; i < S; ++i) {
    const int cam = pl.sup_cam[(size_t)i];
    rf_view_matrix(k + 4 * (size_t)cam, q + 4 * (size_t)cam, t + 3 * (size_t)cam, tab.data() + i, stride);
    const double *l = pl.l2d.data() + 4 * i;
    tab[18 * stride + i] = l[0]; tab[19 * stride + i] = l[1];
    tab[20 * stride + i] = l[2]; tab[21 * stride + i] = l[3];
    const double dx = l[2] - l[0], dy = l[3] - l[1];
    tab[22 * stride + i] = std::sqrt(dx * dx + dy * dy) / 30.0;
  }
  out.resize((size_t)T);
#pragma omp parallel for num_threads(nt) schedule(dynamic, 16)
  for (long long n = 0; n < T; ++n) {
    RfOut &o = out[(size_t)n];
    const RfTrack &tr = pl.tracks[(size_t)n];
    rf_minimal(pl.line6.data() + 6 * n, o.p);
    HostGroup grp{tab.data(), stride, tr, cfg.geometric_alpha};
    rf_lm(grp, tr.constant != 0, cfg.max_num_iterations, o.p, &o.cost0, &o.cost1, &o.iters, &o.code);
    cut_host(tr, pl.l3d.data(), cfg.num_outliers_aggregator, o);
  }
}

void copy_out(const RfOut *o, long long T, double *params6, double *seg6, double *cost2, int32_t *iters, int32_t *codes) {
  for (long long n = 0; n < T; ++n) {
    if (params6) std::copy(o[n].p, o[n].p + 6, params6 + 6 * n);
    if (seg6) std::copy(o[n].seg, o[n].seg + 6, seg6 + 6 * n);
    if (cost2) { cost2[2 * n] = o[n].cost0; cost2[2 * n + 1] = o[n].cost1; }
    if (iters) iters[n] = o[n].iters;
    if (codes) codes[n] = o[n].code;
  }
}

// upload of the plan, the three kernels, download into ctx->rf.out; d_k / d_q / d_t: the cameras on the device
int run_device(lt_ctx *ctx, const Plan &pl, const double *d_k, const double *d_q, const double *d_t,
               const lt_refine_config &cfg, double t0) {
  const long long S = pl.n_sup, T = (long long)pl.tracks.size();
  static_assert(sizeof(RfOut) == 15 * sizeof(double), "RfOut is 15 doubles");
  ctx->rf.out.assign(15 * (size_t)T, 0.0);
  for (int k = 0; k < 4; ++k) ctx->rf.timers[k] = 0.0;
  if (T == 0) return LT_OK;
  if (T * kRfWidth / kRfBlock + 1 > (long long)INT_MAX / kRfBlock || S > ((long long)1 << 31))
    return fail(ctx, LT_ERR_ARGUMENT, "lt_refine: too many tracks for one call (split them)");
  hipStream_t st = ctx->stream;
  const long long stride = S;
  if (int rc = upload_vec(ctx, ctx->rf.d_cam, pl.sup_cam)) return rc;
  if (int rc = upload_vec(ctx, ctx->rf.d_l2d, pl.l2d)) return rc;
  if (int rc = upload_vec(ctx, ctx->rf.d_l3d, pl.l3d)) return rc;
  if (int rc = upload_vec(ctx, ctx->rf.d_line, pl.line6)) return rc;
  if (int rc = upload_vec(ctx, ctx->rf.d_tracks, pl.tracks)) return rc;
  ENSURE(ctx, ctx->rf.d_tab, 8 * (size_t)kRfFields * (size_t)stride);
  ENSURE(ctx, ctx->rf.d_out, sizeof(RfOut) * (size_t)T);
  if (int rc = stream_sync(ctx)) return rc;
  const double t1 = now_ms();
  ctx->rf.timers[0] = t1 - t0;

  RfDev dev;
  dev.tracks = ctx->rf.d_tracks.as<RfTrack>();
  dev.n_tracks = T;
  dev.sup = ctx->rf.d_tab.as<double>();
  dev.stride = stride;
  dev.l3d = ctx->rf.d_l3d.as<double>();
  dev.alpha = cfg.geometric_alpha;
  dev.max_iter = cfg.max_num_iterations;
  dev.num_outliers = cfg.num_outliers_aggregator;
  RfOut *d_out = ctx->rf.d_out.as<RfOut>();
  Events<2> ev;  // around k_refine_lm
  if (int rc = ev.create(ctx)) return rc;
  launch_refine_prep(st, d_k, d_q, d_t, ctx->rf.d_cam.as<int>(), ctx->rf.d_l2d.as<double>(), S, ctx->rf.d_tab.as<double>(),
                     stride, ctx->rf.d_line.as<double>(), T, d_out);
  if (int rc = ev.record(ctx, 0)) return rc;
  launch_refine_lm(st, dev, d_out);
  if (int rc = ev.record(ctx, 1)) return rc;
  launch_refine_cut(st, dev, d_out);
  if (int rc = stream_sync(ctx)) return rc;
  const double t2 = now_ms();
  ctx->rf.timers[1] = t2 - t1;
  ctx->rf.timers[3] = ev.ms(0, 1);
  HIPCHK(ctx, hipMemcpyAsync(ctx->rf.out.data(), d_out, sizeof(RfOut) * (size_t)T, hipMemcpyDeviceToHost, st));
  if (int rc = stream_sync(ctx)) return rc;
  ctx->rf.timers[2] = now_ms() - t2;
  return LT_OK;
}

}  // namespace

namespace lt_impl {

// lt_refine_tracks (lt_tracks.cpp): the cameras of the context, resident since lt_init
int refine_with_ctx_cams(lt_ctx *ctx, int64_t T, const double *line6, const int64_t *off, const int32_t *img,
                         const double *l2d4, const double *l3d6, const lt_refine_config *cfg) {
  const std::string who = "lt_refine_tracks";
  const double t0 = now_ms();
  if (!ctx->inited || !ctx->d_kvec.p || !ctx->d_qvec.p || !ctx->d_tvec.p)
    return fail(ctx, LT_ERR_STATE, who + ": the context holds no cameras (lt_init first)");
  std::string msg;
  Plan pl;
  if (check_config(cfg, msg) || make_plan(ctx->id2idx, T, line6, off, img, l2d4, l3d6, *cfg, pl, msg))
    return fail(ctx, LT_ERR_ARGUMENT, who + ": " + msg);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return run_device(ctx, pl, ctx->d_kvec.as<double>(), ctx->d_qvec.as<double>(), ctx->d_tvec.as<double>(), *cfg, t0);
}

}  // namespace lt_impl

extern "C" {

void lt_refine_config_default(lt_refine_config *cfg) {
  if (!cfg) return;
  cfg->geometric_alpha = 10.0;       // refinement_config.h:58-69
  cfg->min_num_images = 4;
  cfg->num_outliers_aggregator = 2;  // cfgs/triangulation/default.yaml:143
  cfg->num_outliers_aggregate = 2;
  cfg->max_num_iterations = 100;
  cfg->constant_line = 0;            // hybrid_bundle_adjustment_config.h:33
  cfg->pad_ = 0;
}

int lt_refine_arrays(lt_ctx *ctx, int n_img, const int32_t *img_ids, const double *kvec4, const double *qvec4,
                     const double *tvec3, int64_t n_tracks, const double *line6, const int64_t *off, const int32_t *img,
                     const double *line2d4, const double *line3d6, const lt_refine_config *cfg) {
  if (!ctx) return LT_ERR_ARGUMENT;
  const std::string who = "lt_refine_arrays";
  const double t0 = now_ms();
  std::string msg;
  std::unordered_map<int, int> id2idx;
  Plan pl;
  if (check_config(cfg, msg) || check_cams(n_img, img_ids, kvec4, qvec4, tvec3, id2idx, msg) ||
      make_plan(id2idx, n_tracks, line6, off, img, line2d4, line3d6, *cfg, pl, msg))
    return fail(ctx, LT_ERR_ARGUMENT, who + ": " + msg);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t nI = (size_t)std::max(n_img, 1);
  ENSURE(ctx, ctx->rf.d_k, 32 * nI);
  ENSURE(ctx, ctx->rf.d_q, 32 * nI);
  ENSURE(ctx, ctx->rf.d_t, 24 * nI);
  if (n_img > 0) {
    HIPCHK(ctx, hipMemcpyAsync(ctx->rf.d_k.p, kvec4, 32 * (size_t)n_img, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->rf.d_q.p, qvec4, 32 * (size_t)n_img, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->rf.d_t.p, tvec3, 24 * (size_t)n_img, hipMemcpyHostToDevice, ctx->stream));
  }
  return run_device(ctx, pl, ctx->rf.d_k.as<double>(), ctx->rf.d_q.as<double>(), ctx->rf.d_t.as<double>(), *cfg, t0);
}

int64_t lt_refine_num(lt_ctx *ctx) { return ctx ? (int64_t)(ctx->rf.out.size() / 15) : 0; }

int lt_refine_get(lt_ctx *ctx, double *params6, double *seg6, double *cost2, int32_t *iters, int32_t *codes) {
  if (!ctx) return LT_ERR_ARGUMENT;
  copy_out(reinterpret_cast<const RfOut *>(ctx->rf.out.data()), (long long)(ctx->rf.out.size() / 15), params6, seg6, cost2,
           iters, codes);
  return LT_OK;
}

int lt_refine_get_timers(lt_ctx *ctx, double out[4]) {
  if (!ctx || !out) return LT_ERR_ARGUMENT;
  for (int k = 0; k < 4; ++k) out[k] = ctx->rf.timers[k];
  return LT_OK;
}

static thread_local std::string g_host_error;
const char *lt_fn_refine_host_error(void) { return g_host_error.c_str(); }

int lt_fn_refine_host(int n_img, const int32_t *img_ids, const double *kvec4, const double *qvec4, const double *tvec3,
                      int64_t n_tracks, const double *line6, const int64_t *off, const int32_t *img,
                      const double *line2d4, const double *line3d6, const lt_refine_config *cfg, int n_threads,
                      double *params6, double *seg6, double *cost2, int32_t *iters, int32_t *codes) {
  std::string msg;
  std::unordered_map<int, int> id2idx;
  Plan pl;
  if (check_config(cfg, msg) || check_cams(n_img, img_ids, kvec4, qvec4, tvec3, id2idx, msg) ||
      make_plan(id2idx, n_tracks, line6, off, img, line2d4, line3d6, *cfg, pl, msg)) {
    g_host_error = "lt_fn_refine_host: " + msg;
    return LT_ERR_ARGUMENT;
  }
  g_host_error.clear();
  std::vector<RfOut> out;
  run_host(pl, kvec4, qvec4, tvec3, *cfg, n_threads, out);
  copy_out(out.data(), (long long)out.size(), params6, seg6, cost2, iters, codes);
  return LT_OK;
}

int lt_fn_refine_eval(int64_t K, const double *cam11, const double *line2d4, const double params6[6], double alpha,
                      double *residuals, double *cost, double g[4], double H[16]) {
  if (K < 1 || !cam11 || !line2d4 || !params6 || !(alpha >= 0.0) || !(alpha <= 700.0)) return LT_ERR_ARGUMENT;
  std::vector<double> tab((size_t)kRfFields * (size_t)K);
  for (int64_t i = 0; i < K; ++i) {
    const double *c = cam11 + 11 * i, *l = line2d4 + 4 * i;
    rf_view_matrix(c, c + 4, c + 8, tab.data() + i, (long long)K);
    tab[18 * K + i] = l[0]; tab[19 * K + i] = l[1]; tab[20 * K + i] = l[2]; tab[21 * K + i] = l[3];
    const double dx = l[2] - l[0], dy = l[3] - l[1];
    tab[22 * K + i] = std::sqrt(dx * dx + dy * dy) / 30.0;
  }
  const RfTrack tr{0, (int)K, 0};
  HostGroup grp{tab.data(), (long long)K, tr, alpha};
  if (cost) *cost = grp.cost(params6);
  double acc[kRfSums];
  grp.linearise(params6, acc);
  if (H) {
    int o = 0;
    for (int i = 0; i < 4; ++i)
      for (int j = i; j < 4; ++j, ++o) H[4 * i + j] = H[4 * j + i] = acc[o];
  }
  if (g) std::copy(acc + 10, acc + 14, g);
  if (residuals) {
    Rf4 u[4], w[2], dm[6];
    rf_seed(params6, u, w);
    rf_plucker<Rf4>(u, w, dm);
    double scratch[kRfSums] = {0};
    for (int64_t i = 0; i < K; ++i) rf_accumulate(rf_load(tab.data(), K, i), dm, alpha, scratch, residuals + 2 * i);
  }
  return LT_OK;
}

int lt_fn_refine_cut(int64_t K, const double *line3d6, const double params6[6], int num_outliers, double seg6[6]) {
  if (K < 1 || K > (1 << 28) || !line3d6 || !params6 || !seg6 || num_outliers < 0 || num_outliers > 2 * K - 1 ||
      !all_finite(line3d6, 6 * (size_t)K))
    return LT_ERR_ARGUMENT;
  RfOut o;
  std::copy(params6, params6 + 6, o.p);
  cut_host(RfTrack{0, (int)K, 0}, line3d6, num_outliers, o);
  std::copy(o.seg, o.seg + 6, seg6);
  return LT_OK;
}

int lt_fn_refine_explog(int which, int64_t n, const double *x, double *out) {
  if (n < 0 || (n > 0 && (!x || !out)) || (which != 0 && which != 1)) return LT_ERR_ARGUMENT;
  for (int64_t k = 0; k < n; ++k) {
    if (which == 0 ? !(x[k] >= 0.0 && x[k] <= 700.0) : !(x[k] >= 1.0 && x[k] < kMaxDist)) return LT_ERR_ARGUMENT;
    out[k] = which == 0 ? lt_exp(x[k]) : lt_log(x[k]);
  }
  return LT_OK;
}

int lt_fn_refine_minimal(const double line6[6], double params6[6]) {
  if (!line6 || !params6 || !all_finite(line6, 6)) return LT_ERR_ARGUMENT;
  const double dx = line6[0] - line6[3], dy = line6[1] - line6[4], dz = line6[2] - line6[5];
  if (!(std::sqrt((dx * dx + dy * dy) + dz * dz) > 0.0)) return LT_ERR_ARGUMENT;
  rf_minimal(line6, params6);
  return LT_OK;
}

int lt_fn_refine_infinite(const double params6[6], double dm6[6]) {
  if (!params6 || !dm6) return LT_ERR_ARGUMENT;
  d3 d, m;
  rf_infinite(params6, &d, &m);
  dm6[0] = d.x; dm6[1] = d.y; dm6[2] = d.z;
  dm6[3] = m.x; dm6[4] = m.y; dm6[5] = m.z;
  return LT_OK;
}

}  // extern "C"
