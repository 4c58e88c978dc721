// lt_loc.cpp -- the point-line pose refinement of limap.optimize.hybrid_localization (LineLocEngine, JointLocEngine,
// solve_jointloc; optimize/hybrid_localization/hybrid_localization.cc:26-134) for a batch of independent problems.
// Validation, the residual blocks in JointLocEngine::AddResiduals' order with their ScaledLoss weights, upload, the launch
// of lt_kernels_loc.hip and the download; lt_fn_loc_host is the whole step in plain C++ from the same inline functions
// (lt_loc.h) with the reductions in the device's order, so both agree bit for bit.

#include "lt_host.h"
#include "lt_loc.h"
#include "lt_twin.h"

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

struct Plan {
  std::vector<LcProb> probs;
  std::vector<double> tab;   // kLcFields x stride
  std::vector<double> kvec;  // 4 per problem
  std::vector<LcOut> init;   // the initial poses, q normalised once
  long long stride = 1;
  LcCfg cfg;
};

// the checks and the block table.  Blocks of a problem: its 3D lines in order, each with its 2D segments in order
// (ScaledLoss weight weight_line * length / sum_lengths), then its points (weight_point)
int make_plan(int64_t P, const double *kvec4, const double *qvec4, const double *tvec3, const int64_t *line_off,
              const double *line3d6, const int64_t *seg_off, const double *seg4, const int64_t *pt_off, const double *p3d3,
              const double *p2d2, const lt_loc_config *c, Plan &pl, std::string &msg) {
  if (lc_check_config(c, pl.cfg, msg)) return 1;
  if (P < 0 || (P > 0 && (!kvec4 || !qvec4 || !tvec3))) { msg = "bad problem arrays"; return 1; }
  msg = offsets_msg("line", P, line_off);
  if (!msg.empty()) return 1;
  msg = offsets_msg("point", P, pt_off);
  if (!msg.empty()) return 1;
  const long long NL = line_off[P], NP = pt_off[P];
  msg = offsets_msg("segment", NL, seg_off);
  if (!msg.empty()) return 1;
  const long long NS = seg_off[NL];
  if ((NL > 0 && !line3d6) || (NS > 0 && !seg4) || (NP > 0 && (!p3d3 || !p2d2))) { msg = "null correspondence arrays"; return 1; }
  if (!all_finite(kvec4, 4 * P) || !all_finite(qvec4, 4 * P) || !all_finite(tvec3, 3 * P)) { msg = "non-finite camera or pose"; return 1; }
  if (!all_finite(line3d6, 6 * NL) || !all_finite(seg4, 4 * NS) || !all_finite(p3d3, 3 * NP) || !all_finite(p2d2, 2 * NP)) {
    msg = "non-finite coordinate";
    return 1;
  }
  const long long NB = NS + NP;
  if (NB > ((long long)1 << 31) || P > (long long)INT_MAX) { msg = "too many blocks for one call (split the problems)"; return 1; }
  pl.stride = std::max<long long>(NB, 1);
  pl.tab.assign((size_t)kLcFields * (size_t)pl.stride, 0.0);
  pl.probs.resize((size_t)P);
  pl.kvec.assign(kvec4, kvec4 + 4 * (size_t)P);
  pl.init.resize((size_t)P);
  const long long st = pl.stride;
  double *tab = pl.tab.data();
  const int nres_line = lc_num_res(pl.cfg.cost);
  // problem n owns blocks [seg_off[line_off[n]] + pt_off[n], ...): the problems fill the table independently
  auto fill = [&](int64_t n, std::string &msg) -> int {
    long long b = seg_off[line_off[n]] + pt_off[n];
    const double *k = kvec4 + 4 * n;
    if (k[0] == 0.0 || k[1] == 0.0) { msg = "problem " + std::to_string(n) + ": a focal length is 0"; return 1; }
    const double *q = qvec4 + 4 * n;
    if (q[0] == 0.0 && q[1] == 0.0 && q[2] == 0.0 && q[3] == 0.0) { msg = "problem " + std::to_string(n) + ": zero quaternion"; return 1; }
    LcOut &o = pl.init[(size_t)n];
    lm_normalise_q(q, o.q);
    for (int c2 = 0; c2 < 3; ++c2) o.t[c2] = tvec3[3 * n + c2];
    o.cost0 = o.cost1 = 0.0;
    o.iters = 0;
    o.code = 0;
    const long long b0 = b;
    long long n_res = 0;
    for (long long l = line_off[n]; l < line_off[n + 1]; ++l) {
      const double *l3 = line3d6 + 6 * l;
      const double dx = l3[3] - l3[0], dy = l3[4] - l3[1], dz = l3[5] - l3[2];
      // upstream divides the direction by sqrt(0 + 1e-8) and optimises against a zero direction: no constraint a caller
      // can mean, so it is an argument error here
      if (!(std::sqrt((dx * dx + dy * dy) + dz * dz) > 0.0)) { msg = "3D line " + std::to_string(l) + " has zero length"; return 1; }
      double sum_lengths = 0.0;  // hybrid_localization.cc:105-108
      for (long long s = seg_off[l]; s < seg_off[l + 1]; ++s) {
        const double *g = seg4 + 4 * s;
        const double ex = g[2] - g[0], ey = g[3] - g[1];
        sum_lengths += std::sqrt(ex * ex + ey * ey);
      }
      if (seg_off[l + 1] > seg_off[l] && !(sum_lengths > 0.0)) {  // length / sum_lengths is 0 / 0 upstream
        msg = "the 2D segments of 3D line " + std::to_string(l) + " have sum_lengths == 0";
        return 1;
      }
      for (long long s = seg_off[l]; s < seg_off[l + 1]; ++s, ++b) {
        const double *g = seg4 + 4 * s;
        const double ex = g[2] - g[0], ey = g[3] - g[1];
        const double length = std::sqrt(ex * ex + ey * ey);
        for (int c2 = 0; c2 < 6; ++c2) tab[(long long)c2 * st + b] = l3[c2];
        tab[6 * st + b] = g[0]; tab[7 * st + b] = g[1];
        tab[8 * st + b] = g[2]; tab[9 * st + b] = g[3];
        tab[10 * st + b] = c->weight_line * length / sum_lengths;  // :112
        tab[11 * st + b] = 0.0;
        n_res += nres_line;
      }
    }
    for (long long i = pt_off[n]; i < pt_off[n + 1]; ++i, ++b) {
      for (int c2 = 0; c2 < 3; ++c2) tab[(long long)c2 * st + b] = p3d3[3 * i + c2];
      tab[6 * st + b] = p2d2[2 * i];
      tab[7 * st + b] = p2d2[2 * i + 1];
      tab[10 * st + b] = c->weight_point;
      tab[11 * st + b] = 1.0;
      n_res += 2;
    }
    if (b - b0 > (1 << 28)) { msg = "too many blocks in a problem"; return 1; }
    pl.probs[(size_t)n] = LcProb{b0, (int)(b - b0), (int)n_res};
    return 0;
  };
  long long bad = -1;  // the first problem with an error speaks, whatever the thread count
  std::string bad_msg;
#pragma omp parallel for schedule(static)
  for (int64_t n = 0; n < P; ++n) {
    std::string m;
    if (fill(n, m)) {
#pragma omp critical(lt_loc_plan)
      if (bad < 0 || n < bad) { bad = n; bad_msg = m; }
    }
  }
  if (bad >= 0) { msg = bad_msg; return 1; }
  return 0;
}

// the host twin of the wave of k_loc_lm
typedef LcGroup<LmHostLanes<kLcWidth>> HostGroup;

void run_host(const Plan &pl, int n_threads, std::vector<LcOut> &out) {
  const long long P = (long long)pl.probs.size();
  out = pl.init;
  const int nt = n_threads > 0 ? n_threads : omp_get_max_threads();
#pragma omp parallel for num_threads(nt) schedule(dynamic, 4)
  for (long long n = 0; n < P; ++n) {
    LcOut &o = out[(size_t)n];
    const LcProb &pr = pl.probs[(size_t)n];
    HostGroup grp{{}, pl.cfg, pl.tab.data(), pl.stride, pr.b0, pr.n, pl.kvec.data() + 4 * n};
    double p[7] = {o.q[0], o.q[1], o.q[2], o.q[3], o.t[0], o.t[1], o.t[2]};
    lc_lm(grp, pr.n, pl.cfg.max_iter, p, &o.cost0, &o.cost1, &o.iters, &o.code);
    for (int c = 0; c < 4; ++c) o.q[c] = p[c];
    for (int c = 0; c < 3; ++c) o.t[c] = p[4 + c];
  }
}

void copy_out(const LcOut *o, const int *n_res, long long P, double *qvec4, double *tvec3, double *cost2, int32_t *num_res,
              int32_t *iters, int32_t *codes) {
  for (long long n = 0; n < P; ++n) {
    if (qvec4) std::copy(o[n].q, o[n].q + 4, qvec4 + 4 * n);
    if (tvec3) std::copy(o[n].t, o[n].t + 3, tvec3 + 3 * n);
    if (cost2) { cost2[2 * n] = o[n].cost0; cost2[2 * n + 1] = o[n].cost1; }
    if (num_res) num_res[n] = n_res[n];
    if (iters) iters[n] = o[n].iters;
    if (codes) codes[n] = o[n].code;
  }
}

std::vector<int> residual_counts(const Plan &pl) {
  std::vector<int> r(pl.probs.size());
  for (size_t n = 0; n < r.size(); ++n) r[n] = pl.probs[n].n_res;
  return r;
}

static thread_local HostError g_host_error;

// ---- pose scoring ----
struct ScorePlan {
  std::vector<double> tab;  // kLcScoreFields x stride; points first
  std::vector<double> q, t;
  long long stride = 1, H = 0, N = 0;
  LcScoreDev dev;
};

int make_score_plan(const double *kvec4, int64_t n_l3d, const double *line3d6, int64_t n_seg, const int32_t *l3d_ids,
                    const double *seg4, int64_t n_pts, const double *p3d3, const double *p2d2, int64_t n_poses,
                    const double *qvec4, const double *tvec3, const lt_loc_score_config *c, ScorePlan &pl, std::string &msg) {
  if (!c) { msg = "null configuration"; return 1; }
  if (c->cost_function == kLcMidpointAngle3) { msg = "E2DMidpointAngleDist3 is not compatible with scoring (upstream throws)"; return 1; }
  if (c->cost_function < kLcMidpoint2 || c->cost_function > kLcPlaneLine2) { msg = "unknown line cost function"; return 1; }
  if (n_l3d < 0 || n_seg < 0 || n_pts < 0 || n_poses < 0 || !kvec4) { msg = "bad counts"; return 1; }
  if ((n_l3d > 0 && !line3d6) || (n_seg > 0 && (!l3d_ids || !seg4)) || (n_pts > 0 && (!p3d3 || !p2d2)) ||
      (n_poses > 0 && (!qvec4 || !tvec3))) {
    msg = "null arrays";
    return 1;
  }
  if (!all_finite(kvec4, 4) || !all_finite(line3d6, 6 * n_l3d) || !all_finite(seg4, 4 * n_seg) ||
      !all_finite(p3d3, 3 * n_pts) || !all_finite(p2d2, 2 * n_pts)) {
    msg = "non-finite input";  // the poses may be: a NaN pose fails its cheirality tests
    return 1;
  }
  if (kvec4[0] == 0.0 || kvec4[1] == 0.0) { msg = "a focal length is 0"; return 1; }
  if (std::isnan(c->cheirality_min_depth) || std::isnan(c->cheirality_overlap_pixels)) { msg = "non-finite cheirality bound"; return 1; }
  if (c->want_msac)
    for (int i = 0; i < 2; ++i)
      if (std::isnan(c->squared_thresholds[i]) || !std::isfinite(c->weights[i])) { msg = "non-finite threshold or weight"; return 1; }
  const long long N = n_pts + n_seg;
  if (N > (long long)INT_MAX / 2 || n_poses > (long long)INT_MAX) { msg = "too many correspondences or poses for one call"; return 1; }
  pl.H = n_poses;
  pl.N = N;
  pl.stride = std::max<long long>(N, 1);
  pl.tab.assign((size_t)kLcScoreFields * (size_t)pl.stride, 0.0);
  const long long st = pl.stride;
  double *tab = pl.tab.data();
  for (long long i = 0; i < n_pts; ++i) lc_score_fill_point(tab, st, i, p3d3 + 3 * i, p2d2 + 2 * i);
  std::vector<double> dm(6 * (size_t)std::max<int64_t>(n_l3d, 1));  // the pose-independent part of a 3D line, once
  std::vector<char> have((size_t)std::max<int64_t>(n_l3d, 1), 0);
  for (long long s2 = 0; s2 < n_seg; ++s2)
    if (lc_score_fill_line(tab, st, n_pts + s2, n_l3d, line3d6, l3d_ids[s2], seg4 + 4 * s2, dm.data(), have.data(), msg)) return 1;
  pl.q.assign(qvec4, qvec4 + 4 * (size_t)n_poses);
  pl.t.assign(tvec3, tvec3 + 3 * (size_t)n_poses);
  LcScoreDev &d = pl.dev;
  d.tab = tab;
  d.stride = st;
  d.qvec = pl.q.data();
  d.tvec = pl.t.data();
  d.n_poses = n_poses;
  for (int k = 0; k < 4; ++k) d.k[k] = kvec4[k];
  d.sc.cfg = lc_cfg_of(c->cost_function, kLcNone, kLcTrivial, 1.0, 0);
  d.sc.min_depth = c->cheirality_min_depth;
  d.sc.overlap = c->cheirality_overlap_pixels;
  for (int i = 0; i < 2; ++i) { d.sc.thr2[i] = c->squared_thresholds[i]; d.sc.w[i] = c->weights[i]; }
  d.sc.n_points = (int)n_pts;
  d.sc.n_lines = (int)n_seg;
  d.sc.want_msac = c->want_msac ? 1 : 0;
  d.sc.pad_ = 0;
  return 0;
}

// k_loc_score on the host: the same cells, the score summed in the wave's order
void score_host(const ScorePlan &pl, int n_threads, double *table, double *scores, int32_t *inliers) {
  const LcScoreDev &d = pl.dev;
  const int nt = n_threads > 0 ? n_threads : omp_get_max_threads();
  const long long N = pl.N;
#pragma omp parallel for num_threads(nt) schedule(dynamic, 8)
  for (long long h = 0; h < pl.H; ++h) {
    int in[2] = {0, 0};
    const double sum = lc_msac_sum(LmHostLanes<kLcWidth>{}, d.sc, d.k, d.qvec + 4 * h, d.tvec + 3 * h, d.tab, d.stride, 0,
                                   d.sc.n_points, d.sc.n_lines, [&](int i, bool is_point, double r2) {
      if (table) table[h * N + i] = r2;
      if (d.sc.want_msac && r2 < d.sc.thr2[is_point ? 0 : 1]) in[is_point ? 0 : 1] += 1;
    });
    if (d.sc.want_msac) {
      if (scores) scores[h] = sum;
      if (inliers) { inliers[2 * h] = in[0]; inliers[2 * h + 1] = in[1]; }
    }
  }
}

}  // namespace

extern "C" {

void lt_loc_config_default(lt_loc_config *cfg) {
  if (!cfg) return;
  cfg->cost_function = kLcPerp2;  // hybrid_localization_config.h:37-56,66-67
  cfg->weight_function = kLcNone;
  cfg->loss = kLcTrivial;
  cfg->max_num_iterations = 100;
  cfg->loss_a = 1.0;
  cfg->weight_line = 1.0;
  cfg->weight_point = 1.0;
}

int lt_loc_solve(lt_ctx *ctx, int64_t n_prob, const double *kvec4, const double *qvec4, const double *tvec3,
                 const int64_t *line_off, const double *line3d6, const int64_t *seg_off, const double *seg4,
                 const int64_t *pt_off, const double *p3d3, const double *p2d2, const lt_loc_config *cfg) {
  if (!ctx) return LT_ERR_ARGUMENT;
  const double t0 = now_ms();
  std::string msg;
  Plan pl;
  if (make_plan(n_prob, kvec4, qvec4, tvec3, line_off, line3d6, seg_off, seg4, pt_off, p3d3, p2d2, cfg, pl, msg))
    return fail(ctx, LT_ERR_ARGUMENT, "lt_loc_solve: " + msg);
  const long long P = n_prob;
  static_assert(sizeof(LcOut) == 10 * sizeof(double), "LcOut is 10 doubles");
  ctx->lc.out.assign(10 * (size_t)P, 0.0);
  ctx->lc.n_res = residual_counts(pl);
  for (int k = 0; k < 4; ++k) ctx->lc.timers[k] = 0.0;
  if (P == 0) return LT_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (int rc = upload_vec(ctx, ctx->lc.d_tab, pl.tab)) return rc;
  if (int rc = upload_vec(ctx, ctx->lc.d_probs, pl.probs)) return rc;
  if (int rc = upload_vec(ctx, ctx->lc.d_k, pl.kvec)) return rc;
  if (int rc = upload_vec(ctx, ctx->lc.d_out, pl.init)) return rc;
  if (int rc = stream_sync(ctx)) return rc;
  const double t1 = now_ms();
  ctx->lc.timers[0] = t1 - t0;
  LcDev dev;
  dev.probs = ctx->lc.d_probs.as<LcProb>();
  dev.n_probs = P;
  dev.tab = ctx->lc.d_tab.as<double>();
  dev.stride = pl.stride;
  dev.kvec = ctx->lc.d_k.as<double>();
  dev.cfg = pl.cfg;
  LcOut *d_out = ctx->lc.d_out.as<LcOut>();
  Events<2> ev;  // around k_loc_lm
  if (int rc = ev.create(ctx)) return rc;
  if (int rc = ev.record(ctx, 0)) return rc;
  launch_loc_lm(st, dev, d_out);
  if (int rc = ev.record(ctx, 1)) return rc;
  if (int rc = stream_sync(ctx)) return rc;
  const double t2 = now_ms();
  ctx->lc.timers[1] = t2 - t1;
  ctx->lc.timers[3] = ev.ms(0, 1);
  HIPCHK(ctx, hipMemcpyAsync(ctx->lc.out.data(), d_out, sizeof(LcOut) * (size_t)P, hipMemcpyDeviceToHost, st));
  if (int rc = stream_sync(ctx)) return rc;
  ctx->lc.timers[2] = now_ms() - t2;
  return LT_OK;
}

int64_t lt_loc_num(lt_ctx *ctx) { return ctx ? (int64_t)(ctx->lc.out.size() / 10) : 0; }

int lt_loc_get(lt_ctx *ctx, double *qvec4, double *tvec3, double *cost2, int32_t *num_res, int32_t *iters, int32_t *codes) {
  if (!ctx) return LT_ERR_ARGUMENT;
  copy_out(reinterpret_cast<const LcOut *>(ctx->lc.out.data()), ctx->lc.n_res.data(), (long long)(ctx->lc.out.size() / 10),
           qvec4, tvec3, cost2, num_res, iters, codes);
  return LT_OK;
}

int lt_loc_get_timers(lt_ctx *ctx, double out[4]) {
  if (!ctx || !out) return LT_ERR_ARGUMENT;
  for (int k = 0; k < 4; ++k) out[k] = ctx->lc.timers[k];
  return LT_OK;
}

const char *lt_fn_loc_host_error(void) { return g_host_error.c_str(); }

int lt_fn_loc_host(int64_t n_prob, const double *kvec4, const double *qvec4, const double *tvec3, const int64_t *line_off,
                   const double *line3d6, const int64_t *seg_off, const double *seg4, const int64_t *pt_off,
                   const double *p3d3, const double *p2d2, const lt_loc_config *cfg, int n_threads, double *qvec4_out,
                   double *tvec3_out, double *cost2, int32_t *num_res, int32_t *iters, int32_t *codes) {
  std::string msg;
  Plan pl;
  const bool bad = make_plan(n_prob, kvec4, qvec4, tvec3, line_off, line3d6, seg_off, seg4, pt_off, p3d3, p2d2, cfg, pl, msg);
  if (int rc = g_host_error.check("lt_fn_loc_host", bad, msg)) return rc;
  std::vector<LcOut> out;
  run_host(pl, n_threads, out);
  const std::vector<int> nr = residual_counts(pl);
  copy_out(out.data(), nr.data(), (long long)out.size(), qvec4_out, tvec3_out, cost2, num_res, iters, codes);
  return LT_OK;
}

// as_given: the pose as the caller holds it (an iterate of the solve), not normalised once more
static int loc_eval(const char *who, bool as_given, const double kvec4[4], const double qvec4[4], const double tvec3[3],
                    int64_t n_lines, const double *line3d6, const int64_t *seg_off, const double *seg4, int64_t n_points,
                    const double *p3d3, const double *p2d2, const lt_loc_config *cfg, double *residuals, double *cost,
                    double g[6], double H[36]) {
  std::string msg;
  Plan pl;
  const int64_t line_off[2] = {0, n_lines}, pt_off[2] = {0, n_points};
  const bool bad = n_lines < 0 || n_points < 0 ||
                   make_plan(1, kvec4, qvec4, tvec3, line_off, line3d6, seg_off, seg4, pt_off, p3d3, p2d2, cfg, pl, msg);
  if (int rc = g_host_error.check(who, bad, msg)) return rc;
  const LcProb &pr = pl.probs[0];
  const LcOut &o = pl.init[0];
  double p[7] = {o.q[0], o.q[1], o.q[2], o.q[3], o.t[0], o.t[1], o.t[2]};
  if (as_given)
    for (int i = 0; i < 4; ++i) p[i] = qvec4[i];
  HostGroup grp{{}, pl.cfg, pl.tab.data(), pl.stride, pr.b0, pr.n, pl.kvec.data()};
  if (residuals) std::fill(residuals, residuals + 4 * (size_t)pr.n, std::nan(""));
  if (cost) *cost = grp.cost(p);
  double acc[kLcSums];
  grp.linearise_res(p, acc, residuals);
  sums_to_gH<6>(acc, g, H);
  return LT_OK;
}

int lt_fn_loc_eval(const double kvec4[4], const double qvec4[4], const double tvec3[3], int64_t n_lines,
                   const double *line3d6, const int64_t *seg_off, const double *seg4, int64_t n_points, const double *p3d3,
                   const double *p2d2, const lt_loc_config *cfg, double *residuals, double *cost, double g[6], double H[36]) {
  return loc_eval("lt_fn_loc_eval", false, kvec4, qvec4, tvec3, n_lines, line3d6, seg_off, seg4, n_points, p3d3, p2d2, cfg,
                  residuals, cost, g, H);
}

int lt_fn_loc_eval_at(const double kvec4[4], const double qvec4[4], const double tvec3[3], int64_t n_lines,
                      const double *line3d6, const int64_t *seg_off, const double *seg4, int64_t n_points,
                      const double *p3d3, const double *p2d2, const lt_loc_config *cfg, double *residuals, double *cost,
                      double g[6], double H[36]) {
  return loc_eval("lt_fn_loc_eval_at", true, kvec4, qvec4, tvec3, n_lines, line3d6, seg_off, seg4, n_points, p3d3, p2d2,
                  cfg, residuals, cost, g, H);
}

int lt_loc_score(lt_ctx *ctx, const double kvec4[4], int64_t n_l3d, const double *line3d6, int64_t n_seg,
                 const int32_t *l3d_ids, const double *seg4, int64_t n_pts, const double *p3d3, const double *p2d2,
                 int64_t n_poses, const double *qvec4, const double *tvec3, const lt_loc_score_config *cfg) {
  if (!ctx) return LT_ERR_ARGUMENT;
  const double t0 = now_ms();
  std::string msg;
  ScorePlan pl;
  if (make_score_plan(kvec4, n_l3d, line3d6, n_seg, l3d_ids, seg4, n_pts, p3d3, p2d2, n_poses, qvec4, tvec3, cfg, pl, msg))
    return fail(ctx, LT_ERR_ARGUMENT, "lt_loc_score: " + msg);
  lt_host::LocState &lc = ctx->lc;
  lc.score_h = pl.H;
  lc.score_n = pl.N;
  lc.score_msac = pl.dev.sc.want_msac != 0;
  lc.table.assign((size_t)pl.H * (size_t)pl.N, 0.0);
  lc.scores.assign((size_t)pl.H, 0.0);
  lc.inliers.assign(2 * (size_t)pl.H, 0);
  for (int k = 0; k < 4; ++k) lc.score_timers[k] = 0.0;
  if (pl.H == 0) return LT_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (int rc = upload_vec(ctx, lc.d_stab, pl.tab)) return rc;
  if (int rc = upload_vec(ctx, lc.d_sq, pl.q)) return rc;
  if (int rc = upload_vec(ctx, lc.d_st, pl.t)) return rc;
  ENSURE(ctx, lc.d_table, 8 * std::max<size_t>((size_t)pl.H * (size_t)pl.N, 1));
  ENSURE(ctx, lc.d_scores, 8 * (size_t)pl.H);
  ENSURE(ctx, lc.d_inl, 8 * (size_t)pl.H);
  if (int rc = stream_sync(ctx)) return rc;
  const double t1 = now_ms();
  lc.score_timers[0] = t1 - t0;
  LcScoreDev dev = pl.dev;
  dev.tab = lc.d_stab.as<double>();
  dev.qvec = lc.d_sq.as<double>();
  dev.tvec = lc.d_st.as<double>();
  Events<2> ev;  // around k_loc_score
  if (int rc = ev.create(ctx)) return rc;
  if (int rc = ev.record(ctx, 0)) return rc;
  launch_loc_score(st, dev, lc.d_table.as<double>(), lc.d_scores.as<double>(), lc.d_inl.as<int>());
  if (int rc = ev.record(ctx, 1)) return rc;
  if (int rc = stream_sync(ctx)) return rc;
  const double t2 = now_ms();
  lc.score_timers[1] = t2 - t1;
  lc.score_timers[3] = ev.ms(0, 1);
  if (pl.N > 0)
    HIPCHK(ctx, hipMemcpyAsync(lc.table.data(), lc.d_table.p, 8 * (size_t)pl.H * (size_t)pl.N, hipMemcpyDeviceToHost, st));
  if (lc.score_msac) {
    HIPCHK(ctx, hipMemcpyAsync(lc.scores.data(), lc.d_scores.p, 8 * (size_t)pl.H, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(lc.inliers.data(), lc.d_inl.p, 8 * (size_t)pl.H, hipMemcpyDeviceToHost, st));
  }
  if (int rc = stream_sync(ctx)) return rc;
  lc.score_timers[2] = now_ms() - t2;
  return LT_OK;
}

int lt_loc_score_size(lt_ctx *ctx, int64_t *n_poses, int64_t *n_corr) {
  if (!ctx) return LT_ERR_ARGUMENT;
  if (n_poses) *n_poses = ctx->lc.score_h;
  if (n_corr) *n_corr = ctx->lc.score_n;
  return LT_OK;
}

int lt_loc_score_get(lt_ctx *ctx, double *table, double *scores, int32_t *inliers2) {
  if (!ctx) return LT_ERR_ARGUMENT;
  const lt_host::LocState &lc = ctx->lc;
  if ((scores || inliers2) && !lc.score_msac) return fail(ctx, LT_ERR_STATE, "lt_loc_score_get: the last call did not ask for the MSAC score");
  if (table) std::copy(lc.table.begin(), lc.table.end(), table);
  if (scores) std::copy(lc.scores.begin(), lc.scores.end(), scores);
  if (inliers2) std::copy(lc.inliers.begin(), lc.inliers.end(), inliers2);
  return LT_OK;
}

int lt_loc_score_get_timers(lt_ctx *ctx, double out[4]) {
  if (!ctx || !out) return LT_ERR_ARGUMENT;
  for (int k = 0; k < 4; ++k) out[k] = ctx->lc.score_timers[k];
  return LT_OK;
}

int lt_fn_loc_score_host(const double kvec4[4], int64_t n_l3d, const double *line3d6, int64_t n_seg, const int32_t *l3d_ids,
                         const double *seg4, int64_t n_pts, const double *p3d3, const double *p2d2, int64_t n_poses,
                         const double *qvec4, const double *tvec3, const lt_loc_score_config *cfg, int n_threads,
                         double *table, double *scores, int32_t *inliers2) {
  std::string msg;
  ScorePlan pl;
  const bool bad = make_score_plan(kvec4, n_l3d, line3d6, n_seg, l3d_ids, seg4, n_pts, p3d3, p2d2, n_poses, qvec4, tvec3, cfg, pl, msg);
  if (int rc = g_host_error.check("lt_fn_loc_score_host", bad, msg)) return rc;
  score_host(pl, n_threads, table, scores, inliers2);
  return LT_OK;
}

int lt_fn_loc_qvec_from_R(const double R9[9], double qvec4[4]) {
  if (!R9 || !qvec4 || !all_finite(R9, 9)) return LT_ERR_ARGUMENT;
  const double m[3][3] = {{R9[0], R9[1], R9[2]}, {R9[3], R9[4], R9[5]}, {R9[6], R9[7], R9[8]}};
  rf_quat_from_matrix(m, qvec4);
  return LT_OK;
}

}  // extern "C"
