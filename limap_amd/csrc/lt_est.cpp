// lt_est.cpp -- the minimal absolute-pose solvers of limap_amd.estimators for a batch of samples of one
// kind: validation, the field-major sample table, upload, the launch of lt_kernels_est.hip and the download;
// lt_fn_est_minimal_host is the same step in plain C++ from the same inline functions (lt_est.h), so both agree bit
// for bit.

#include "lt_host.h"
#include "lt_est_loop.h"
#include "lt_twin.h"

#include <algorithm>
#include <climits>
#include <cstdint>
#include <string>
#include <vector>

#include <omp.h>

using namespace lt;
using namespace lt_impl;

namespace {

struct Plan {
  std::vector<double> tab;  // kEsFields x stride
  long long stride = 1, n = 0;
  int kind = 0;
};

int make_plan(int kind, int64_t n, const double *xs, const double *Xs, const double *ls, const double *Cs, const double *Vs,
              Plan &pl, std::string &msg) {
  if (kind < kEsP3P || kind > kEsP3LL) { msg = "unknown solver kind " + std::to_string(kind); return 1; }
  if (n < 0 || n > (int64_t)INT_MAX / (kEsMaxSol * kEsPoseDoubles)) { msg = "bad sample count"; return 1; }
  const int np = es_num_points(kind), nl = 3 - np;
  if (n > 0 && ((np > 0 && (!xs || !Xs)) || (nl > 0 && (!ls || !Cs || !Vs)))) { msg = "null sample arrays"; return 1; }
  if (!all_finite(xs, np ? 3 * np * n : 0) || !all_finite(Xs, np ? 3 * np * n : 0) || !all_finite(ls, nl ? 3 * nl * n : 0) ||
      !all_finite(Cs, nl ? 3 * nl * n : 0) || !all_finite(Vs, nl ? 3 * nl * n : 0)) {
    msg = "non-finite sample";
    return 1;
  }
  pl.kind = kind;
  pl.n = n;
  pl.stride = std::max<long long>(n, 1);
  pl.tab.assign((size_t)kEsFields * (size_t)pl.stride, 0.0);
  const long long st = pl.stride;
  double *tab = pl.tab.data();
  for (long long i = 0; i < n; ++i) {
    for (int a = 0; a < np; ++a)
      for (int c = 0; c < 3; ++c) {
        tab[(long long)(3 * a + c) * st + i] = xs[(i * np + a) * 3 + c];
        tab[(long long)(9 + 3 * a + c) * st + i] = Xs[(i * np + a) * 3 + c];
      }
    for (int a = 0; a < nl; ++a)
      for (int c = 0; c < 3; ++c) {
        tab[(long long)(18 + 3 * a + c) * st + i] = ls[(i * nl + a) * 3 + c];
        tab[(long long)(27 + 3 * a + c) * st + i] = Cs[(i * nl + a) * 3 + c];
        tab[(long long)(36 + 3 * a + c) * st + i] = Vs[(i * nl + a) * 3 + c];
      }
  }
  return 0;
}

// k_est_minimal on the host
void run_host(const Plan &pl, int n_threads, double *poses, int32_t *counts) {
  EsDev d{pl.tab.data(), pl.stride, pl.n, pl.kind, 0};
  const int nt = n_threads > 0 ? n_threads : omp_get_max_threads();
  constexpr int W = kEsMaxSol * kEsPoseDoubles;
#pragma omp parallel for num_threads(nt) schedule(dynamic, 16)
  for (long long i = 0; i < pl.n; ++i) {
    double x[3][3], X[3][3], l[3][3], C[3][3], V[3][3], out[kEsMaxSol][kEsPoseDoubles];
    es_load(d, i, x, X, l, C, V);
    const int n = es_solve(es_num_points(d.kind), x, X, l, C, V, out);
    if (poses)
      for (int s = 0; s < kEsMaxSol; ++s)
        for (int c = 0; c < kEsPoseDoubles; ++c) poses[i * W + s * kEsPoseDoubles + c] = s < n ? out[s][c] : 0.0;
    if (counts) counts[i] = n;
  }
}

thread_local HostError g_host_error;

// ---- the hybrid loop ----
struct LoopPlan {
  EhOpt opt;
  std::vector<EhQuery> qs;
  std::vector<EhState> st;
  std::vector<double> tab;  // kLcScoreFields x stride
  std::vector<int> ids;     // per correspondence
  std::vector<long long> out_off;  // Q + 1: the queries' places in the caller's inlier array (= c0)
  long long stride = 1, Q = 0, N = 0;
  int running = 0, poll = 4;
};

int make_loop_plan(int64_t Q, const double *kvec4, const double *qvec4, const double *tvec3, const int64_t *pt_off,
                   const double *p3d3, const double *p2d2, const int64_t *l3d_off, const double *line3d6, const int64_t *seg_off,
                   const int32_t *l3d_ids, const double *seg4, const lt_est_config *c, int64_t trace_cap, LoopPlan &pl,
                   std::string &msg) {
  if (!c) { msg = "null configuration"; return 1; }
  if (Q < 0 || Q > 1000000 || (Q > 0 && (!kvec4 || !qvec4 || !tvec3))) { msg = "bad query arrays"; return 1; }
  for (const auto &pr : {std::make_pair("point", pt_off), std::make_pair("3D line", l3d_off), std::make_pair("segment", seg_off)}) {
    msg = offsets_msg(pr.first, Q, pr.second);
    if (!msg.empty()) return 1;
  }
  const long long NP = pt_off[Q], NL = l3d_off[Q], NS = seg_off[Q];
  if ((NP > 0 && (!p3d3 || !p2d2)) || (NL > 0 && !line3d6) || (NS > 0 && (!l3d_ids || !seg4))) { msg = "null correspondence arrays"; return 1; }
  if (!all_finite(kvec4, 4 * Q) || !all_finite(qvec4, 4 * Q) || !all_finite(tvec3, 3 * Q) || !all_finite(p3d3, 3 * NP) ||
      !all_finite(p2d2, 2 * NP) || !all_finite(line3d6, 6 * NL) || !all_finite(seg4, 4 * NS)) {
    msg = "non-finite input";
    return 1;
  }
  const lt_loc_config &lc = c->loc;
  if (lc.cost_function == kLcMidpointAngle3) { msg = "E2DMidpointAngleDist3 is not compatible with scoring (upstream throws)"; return 1; }
  if (lc_check_config(&lc, pl.opt.lsq, msg)) return 1;
  for (int i = 0; i < 2; ++i)
    if (!(c->squared_inlier_thresholds[i] >= 0.0) || !std::isfinite(c->squared_inlier_thresholds[i]) || !std::isfinite(c->data_type_weights[i])) {
      msg = "non-finite or negative threshold or weight";
      return 1;
    }
  if (!(c->success_probability > 0.0 && c->success_probability < 1.0)) { msg = "success_probability must be inside (0, 1)"; return 1; }
  if (!(c->threshold_multiplier >= 1.0) || !std::isfinite(c->threshold_multiplier)) { msg = "threshold_multiplier must be >= 1"; return 1; }
  if (std::isnan(c->cheirality_min_depth) || std::isnan(c->cheirality_overlap_pixels)) { msg = "non-finite cheirality bound"; return 1; }
  if (c->round_size < 1 || c->round_size > 4096) { msg = "round_size must be within 1 .. 4096"; return 1; }
  if (c->num_lo_steps < 0 || c->num_lsq_iterations < 2 || c->min_sample_multiplicator < 1 || c->non_min_sample_multiplier < 1 ||
      c->num_lo_steps > 1000 || c->num_lsq_iterations > 1000) {
    msg = "bad local-optimisation counts (num_lsq_iterations >= 2: upstream divides by num_lsq_iterations - 1)";
    return 1;
  }
  if (c->max_num_iterations > 100000000u || c->max_num_iterations_per_solver > 100000000u || c->min_num_iterations > 100000000u) {
    msg = "iteration bounds above 1e8";
    return 1;
  }
  if (trace_cap < 0 || trace_cap > (1 << 24)) { msg = "bad trace capacity"; return 1; }
  const long long N = NP + NS;
  if (N > (long long)INT_MAX / 2) { msg = "too many correspondences for one call"; return 1; }
  EhOpt &o = pl.opt;
  for (int i = 0; i < 2; ++i) { o.thr2[i] = c->squared_inlier_thresholds[i]; o.w[i] = c->data_type_weights[i]; }
  o.success_probability = c->success_probability;
  o.threshold_multiplier = c->threshold_multiplier;
  o.min_depth = c->cheirality_min_depth;
  o.overlap = c->cheirality_overlap_pixels;
  o.weight_line = lc.weight_line;
  o.weight_point = lc.weight_point;
  o.seed = c->random_seed;
  o.min_it = c->min_num_iterations; o.max_it = c->max_num_iterations;
  o.max_it_solver = c->max_num_iterations_per_solver; o.lo_start = c->lo_starting_iterations;
  o.num_lo_steps = c->num_lo_steps; o.num_lsq = c->num_lsq_iterations;
  o.min_sample_mult = c->min_sample_multiplicator; o.non_min_mult = c->non_min_sample_multiplier;
  o.final_lsq = c->final_least_squares ? 1 : 0;
  o.round_size = c->round_size;
  o.solver_flags = 0;
  for (int i = 0; i < 4; ++i) o.solver_flags |= (c->solver_flags[i] ? 1 : 0) << i;
  o.trace_cap = (int)trace_cap;
  pl.poll = c->poll_interval > 0 ? c->poll_interval : 4;
  pl.Q = Q;
  pl.N = N;
  pl.stride = std::max<long long>(N, 1);
  pl.tab.assign((size_t)kLcScoreFields * (size_t)pl.stride, 0.0);
  pl.ids.assign((size_t)pl.stride, 0);
  pl.qs.resize((size_t)Q);
  pl.st.resize((size_t)Q);
  const long long st = pl.stride;
  double *tab = pl.tab.data();
  pl.running = 0;
  for (long long q = 0; q < Q; ++q) {
    EhQuery &qr = pl.qs[(size_t)q];
    const double *k = kvec4 + 4 * q;
    if (k[0] == 0.0 || k[1] == 0.0) { msg = "query " + std::to_string(q) + ": a focal length is 0"; return 1; }
    const double *qq = qvec4 + 4 * q;
    if (qq[0] == 0.0 && qq[1] == 0.0 && qq[2] == 0.0 && qq[3] == 0.0) { msg = "query " + std::to_string(q) + ": zero quaternion"; return 1; }
    for (int i = 0; i < 4; ++i) { qr.k[i] = k[i]; qr.q0[i] = qq[i]; }
    for (int i = 0; i < 3; ++i) qr.t0[i] = tvec3[3 * q + i];
    qr.c0 = pt_off[q] + seg_off[q];
    qr.n_pts = (int)(pt_off[q + 1] - pt_off[q]);
    qr.n_lines = (int)(seg_off[q + 1] - seg_off[q]);
    const long long n_l3d = l3d_off[q + 1] - l3d_off[q];
    for (long long a = 0; a < qr.n_pts; ++a) {
      const long long i = qr.c0 + a, src = pt_off[q] + a;
      lc_score_fill_point(tab, st, i, p3d3 + 3 * src, p2d2 + 2 * src);
      pl.ids[(size_t)i] = -1;
    }
    for (long long a = 0; a < qr.n_lines; ++a) {
      const long long i = qr.c0 + qr.n_pts + a, src = seg_off[q] + a, id = l3d_ids[src];
      if (lc_score_fill_line(tab, st, i, n_l3d, line3d6 + 6 * l3d_off[q], id, seg4 + 4 * src, nullptr, nullptr, msg)) {
        msg = "query " + std::to_string(q) + ": " + msg;
        return 1;
      }
      pl.ids[(size_t)i] = (int)id;
    }
    eh_init(o, qr, pl.st[(size_t)q]);
    if (!pl.st[(size_t)q].done) pl.running += 1;
  }
  return 0;
}

// the host twin's wave
typedef EhWave<LmHostLanes<kLcWidth>> HostWave;

struct LoopResult {
  std::vector<EhState> st;
  std::vector<int> inl;
  std::vector<double> trace;
};

// the rounds on the host: every query runs its rounds to the end (no query reads another's state)
void run_loop_host(const LoopPlan &pl, int n_threads, LoopResult &res) {
  const long long Q = pl.Q, st = pl.stride, R = pl.opt.round_size;
  res.st = pl.st;
  res.inl.assign((size_t)st, 0);
  res.trace.assign((size_t)Q * (size_t)pl.opt.trace_cap * kEhTrace, 0.0);
  std::vector<double> r2((size_t)st), blk((size_t)kLcFields * (size_t)st);
  std::vector<int> lists(4 * (size_t)st), ints((size_t)std::max<long long>(Q, 1) * kEhInts);
  std::vector<double> rposes((size_t)std::max<long long>(Q, 1) * R * kEsMaxSol * kEsPoseDoubles), rscores((size_t)std::max<long long>(Q, 1) * R * kEsMaxSol);
  std::vector<int> rints(2 * (size_t)std::max<long long>(Q, 1) * R);
  int n_done = 0;
  EhDev d;
  d.opt = pl.opt; d.n_queries = Q; d.stride = st;
  d.qs = pl.qs.data(); d.st = res.st.data(); d.tab = pl.tab.data(); d.l3d_id = pl.ids.data();
  d.r2 = r2.data();
  d.inl = lists.data(); d.base = d.inl + st; d.samp = d.base + st; d.mark = d.samp + st; d.out_inl = res.inl.data();
  d.blk = blk.data(); d.ints = ints.data();
  d.r_poses = rposes.data(); d.r_scores = rscores.data(); d.r_counts = rints.data(); d.r_solver = rints.data() + Q * R;
  d.trace = res.trace.data(); d.n_done = &n_done;
  const int nt = n_threads > 0 ? n_threads : omp_get_max_threads();
#pragma omp parallel for num_threads(nt) schedule(dynamic, 1)
  for (long long q = 0; q < Q; ++q) {
    const EhQuery &qr = d.qs[q];
    HostWave g{{}, d, qr, eh_score_cfg(d.opt, qr)};
    while (!d.st[q].done) {
      for (int slot = 0; slot < R; ++slot) eh_draw_solve(d, q, slot);
      for (int slot = 0; slot < R; ++slot) {
        const long long ri = q * R + slot;
        for (int m = 0; m < d.r_counts[ri]; ++m)
          d.r_scores[ri * kEsMaxSol + m] = g.score_impl(d.r_poses + (ri * kEsMaxSol + m) * kEsPoseDoubles, false);
      }
      EhState s = d.st[q];
      eh_replay(g, d, q, s);
      d.st[q] = s;
    }
  }
}

void copy_loop_out(const LoopPlan &pl, const EhState *st, const int *inl, const double *tr, double *pose7, double *dstats3,
                   int32_t *istats12, int32_t *inliers, double *trace) {
  for (long long q = 0; q < pl.Q; ++q) {
    const EhState &s = st[q];
    if (pose7) std::copy(s.best, s.best + 7, pose7 + 7 * q);
    if (dstats3) { dstats3[3 * q] = s.best_score; dstats3[3 * q + 1] = s.ratios[0]; dstats3[3 * q + 2] = s.ratios[1]; }
    if (istats12) {
      int32_t *o = istats12 + 12 * q;
      o[0] = (int32_t)s.it_total;
      for (int i = 0; i < 4; ++i) o[1 + i] = (int32_t)s.it_solver[i];
      o[5] = s.best_num_inliers; o[6] = s.best_solver; o[7] = s.n_lo; o[8] = s.n_inl[0]; o[9] = s.n_inl[1];
      o[10] = (s.prior[0] > 0.0 || s.prior[1] > 0.0 || s.prior[2] > 0.0 || s.prior[3] > 0.0) ? 1 : 0;
      o[11] = s.n_trace;
    }
  }
  if (inliers) std::copy(inl, inl + pl.N, inliers);
  if (trace) std::copy(tr, tr + (size_t)pl.Q * (size_t)pl.opt.trace_cap * kEhTrace, trace);
}

}  // namespace

extern "C" {

#ifndef LT_HOST_ONLY
int lt_est_minimal(lt_ctx *ctx, int kind, int64_t n, const double *xs, const double *Xs, const double *ls, const double *Cs,
                   const double *Vs) {
  if (!ctx) return LT_ERR_ARGUMENT;
  const double t0 = now_ms();
  std::string msg;
  Plan pl;
  if (make_plan(kind, n, xs, Xs, ls, Cs, Vs, pl, msg)) return fail(ctx, LT_ERR_ARGUMENT, "lt_est_minimal: " + msg);
  lt_host::EsState &es = ctx->es;
  constexpr size_t W = (size_t)kEsMaxSol * kEsPoseDoubles;
  es.poses.assign(W * (size_t)n, 0.0);
  es.counts.assign((size_t)n, 0);
  for (int k = 0; k < 4; ++k) es.timers[k] = 0.0;
  if (n == 0) return LT_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (int rc = upload_vec(ctx, es.d_tab, pl.tab)) return rc;
  ENSURE(ctx, es.d_poses, 8 * W * (size_t)n);
  ENSURE(ctx, es.d_counts, 4 * (size_t)n);
  if (int rc = stream_sync(ctx)) return rc;
  const double t1 = now_ms();
  es.timers[0] = t1 - t0;
  EsDev dev{es.d_tab.as<double>(), pl.stride, pl.n, pl.kind, 0};
  Events<2> ev;  // around k_est_minimal
  if (int rc = ev.create(ctx)) return rc;
  if (int rc = ev.record(ctx, 0)) return rc;
  launch_est_minimal(st, dev, es.d_poses.as<double>(), es.d_counts.as<int>());
  if (int rc = ev.record(ctx, 1)) return rc;
  if (int rc = stream_sync(ctx)) return rc;
  const double t2 = now_ms();
  es.timers[1] = t2 - t1;
  es.timers[3] = ev.ms(0, 1);
  HIPCHK(ctx, hipMemcpyAsync(es.poses.data(), es.d_poses.p, 8 * W * (size_t)n, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(es.counts.data(), es.d_counts.p, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
  if (int rc = stream_sync(ctx)) return rc;
  es.timers[2] = now_ms() - t2;
  return LT_OK;
}

int64_t lt_est_minimal_num(lt_ctx *ctx) { return ctx ? (int64_t)ctx->es.counts.size() : 0; }

int lt_est_minimal_get(lt_ctx *ctx, double *poses56, int32_t *counts) {
  if (!ctx) return LT_ERR_ARGUMENT;
  if (poses56) std::copy(ctx->es.poses.begin(), ctx->es.poses.end(), poses56);
  if (counts) std::copy(ctx->es.counts.begin(), ctx->es.counts.end(), counts);
  return LT_OK;
}

int lt_est_minimal_get_timers(lt_ctx *ctx, double out[4]) {
  if (!ctx || !out) return LT_ERR_ARGUMENT;
  for (int k = 0; k < 4; ++k) out[k] = ctx->es.timers[k];
  return LT_OK;
}
#endif  // LT_HOST_ONLY

const char *lt_fn_est_host_error(void) { return g_host_error.c_str(); }

void lt_est_config_default(lt_est_config *c) {
  if (!c) return;
  c->squared_inlier_thresholds[0] = c->squared_inlier_thresholds[1] = 1.0;  // hybrid_pose_estimator.h:33-34
  c->data_type_weights[0] = c->data_type_weights[1] = 1.0;
  c->success_probability = 0.9999;
  c->threshold_multiplier = 1.4142135623730951;
  c->cheirality_min_depth = 0.0;
  c->cheirality_overlap_pixels = 10.0;
  c->random_seed = 0;
  c->min_num_iterations = 100;
  c->max_num_iterations = 10000;
  c->max_num_iterations_per_solver = 10000;
  c->lo_starting_iterations = 50;
  c->num_lo_steps = 10;
  c->num_lsq_iterations = 4;
  c->min_sample_multiplicator = 7;
  c->non_min_sample_multiplier = 3;
  c->final_least_squares = 0;
  c->round_size = 64;
  for (int i = 0; i < 4; ++i) c->solver_flags[i] = 1;
  c->poll_interval = 4;
  c->loc.cost_function = kLcPerp2;
  c->loc.weight_function = kLcNone;
  c->loc.loss = kLcTrivial;
  c->loc.max_num_iterations = 100;
  c->loc.loss_a = 1.0;
  c->loc.weight_line = 1.0;
  c->loc.weight_point = 1.0;
}

#ifndef LT_HOST_ONLY
int lt_est_solve(lt_ctx *ctx, int64_t n_query, const double *kvec4, const double *qvec4, const double *tvec3,
                 const int64_t *pt_off, const double *p3d3, const double *p2d2, const int64_t *l3d_off, const double *line3d6,
                 const int64_t *seg_off, const int32_t *l3d_ids, const double *seg4, const lt_est_config *cfg,
                 int64_t trace_cap) {
  if (!ctx) return LT_ERR_ARGUMENT;
  const double t0 = now_ms();
  std::string msg;
  LoopPlan pl;
  if (make_loop_plan(n_query, kvec4, qvec4, tvec3, pt_off, p3d3, p2d2, l3d_off, line3d6, seg_off, l3d_ids, seg4, cfg, trace_cap,
                     pl, msg))
    return fail(ctx, LT_ERR_ARGUMENT, "lt_est_solve: " + msg);
  lt_host::EsState &es = ctx->es;
  const long long Q = pl.Q, st = pl.stride, R = pl.opt.round_size;
  es.n_query = Q; es.n_corr = pl.N; es.trace_cap = trace_cap;
  es.pose.assign(7 * (size_t)Q, 0.0);
  es.dstats.assign(3 * (size_t)Q, 0.0);
  es.istats.assign(12 * (size_t)Q, 0);
  es.inliers.assign((size_t)pl.N, 0);
  es.trace.assign((size_t)Q * (size_t)trace_cap * kEhTrace, 0.0);
  for (int k = 0; k < 8; ++k) es.loop_timers[k] = 0.0;
  if (Q == 0) return LT_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t stream = ctx->stream;
  if (int rc = upload_vec(ctx, es.d_qs, pl.qs)) return rc;
  if (int rc = upload_vec(ctx, es.d_st, pl.st)) return rc;
  if (int rc = upload_vec(ctx, es.d_ltab, pl.tab)) return rc;
  if (int rc = upload_vec(ctx, es.d_ids, pl.ids)) return rc;
  const size_t slots = (size_t)Q * (size_t)R;
  ENSURE(ctx, es.d_r2, 8 * (size_t)st);
  ENSURE(ctx, es.d_lists, 4 * 5 * (size_t)st);
  ENSURE(ctx, es.d_blk, 8 * (size_t)kLcFields * (size_t)st);
  ENSURE(ctx, es.d_ints, 4 * (size_t)kEhInts * (size_t)Q);
  ENSURE(ctx, es.d_rposes, 8 * slots * kEsMaxSol * kEsPoseDoubles);
  ENSURE(ctx, es.d_rscores, 8 * slots * kEsMaxSol);
  ENSURE(ctx, es.d_rints, 4 * 2 * slots);
  ENSURE(ctx, es.d_trace, 8 * std::max<size_t>((size_t)Q * (size_t)trace_cap * kEhTrace, 1));
  ENSURE(ctx, es.d_done, 8);
  HIPCHK(ctx, hipMemsetAsync(es.d_done.p, 0, 8, stream));
  HIPCHK(ctx, hipMemsetAsync(es.d_lists.p, 0, 4 * 5 * (size_t)st, stream));
  HIPCHK(ctx, hipMemsetAsync(es.d_trace.p, 0, 8 * std::max<size_t>((size_t)Q * (size_t)trace_cap * kEhTrace, 1), stream));
  if (int rc = stream_sync(ctx)) return rc;
  const double t1 = now_ms();
  es.loop_timers[0] = t1 - t0;
  EhDev d;
  d.opt = pl.opt; d.n_queries = Q; d.stride = st;
  d.qs = es.d_qs.as<EhQuery>(); d.st = es.d_st.as<EhState>(); d.tab = es.d_ltab.as<double>(); d.l3d_id = es.d_ids.as<int>();
  d.r2 = es.d_r2.as<double>();
  d.inl = es.d_lists.as<int>(); d.base = d.inl + st; d.samp = d.base + st; d.mark = d.samp + st; d.out_inl = d.mark + st;
  d.blk = es.d_blk.as<double>(); d.ints = es.d_ints.as<int>();
  d.r_poses = es.d_rposes.as<double>(); d.r_scores = es.d_rscores.as<double>();
  d.r_counts = es.d_rints.as<int>(); d.r_solver = d.r_counts + slots;
  d.trace = es.d_trace.as<double>(); d.n_done = es.d_done.as<int>();
  if (pl.running > 0) {
    Events<2> ev;  // around the rounds of a poll
    if (int rc = ev.create(ctx)) return rc;
    int done = 0;
    long long launched = 0;
    double dev_ms = 0.0;
    const int rc = run_polled(
        ctx, 1, es.d_done.p, done,
        [&] {
          (void)ev.record(ctx, 0);
          for (int k = 0; k < pl.poll; ++k) launch_est_round(stream, d);
          (void)ev.record(ctx, 1);
        },
        [&](int n) { return n >= pl.running; }, [&] { dev_ms += ev.ms(0, 1); }, &launched);
    if (rc) return rc;
    es.loop_timers[3] = (double)(launched * pl.poll);
    es.loop_timers[4] = dev_ms;
  }
  const double t2 = now_ms();
  es.loop_timers[1] = t2 - t1;
  std::vector<EhState> sts((size_t)Q);
  HIPCHK(ctx, hipMemcpyAsync(sts.data(), d.st, sizeof(EhState) * (size_t)Q, hipMemcpyDeviceToHost, stream));
  std::vector<int> inl((size_t)st);
  HIPCHK(ctx, hipMemcpyAsync(inl.data(), d.out_inl, 4 * (size_t)st, hipMemcpyDeviceToHost, stream));
  if (!es.trace.empty()) HIPCHK(ctx, hipMemcpyAsync(es.trace.data(), d.trace, 8 * es.trace.size(), hipMemcpyDeviceToHost, stream));
  if (int rc = stream_sync(ctx)) return rc;
  copy_loop_out(pl, sts.data(), inl.data(), nullptr, es.pose.data(), es.dstats.data(), es.istats.data(), es.inliers.data(), nullptr);
  es.loop_timers[2] = now_ms() - t2;
  return LT_OK;
}

int lt_est_get(lt_ctx *ctx, double *pose7, double *dstats3, int32_t *istats12, int32_t *inliers, double *trace) {
  if (!ctx) return LT_ERR_ARGUMENT;
  const lt_host::EsState &es = ctx->es;
  if (pose7) std::copy(es.pose.begin(), es.pose.end(), pose7);
  if (dstats3) std::copy(es.dstats.begin(), es.dstats.end(), dstats3);
  if (istats12) std::copy(es.istats.begin(), es.istats.end(), istats12);
  if (inliers) std::copy(es.inliers.begin(), es.inliers.end(), inliers);
  if (trace) std::copy(es.trace.begin(), es.trace.end(), trace);
  return LT_OK;
}

int lt_est_get_timers(lt_ctx *ctx, double out[8]) {
  if (!ctx || !out) return LT_ERR_ARGUMENT;
  for (int k = 0; k < 8; ++k) out[k] = ctx->es.loop_timers[k];
  return LT_OK;
}
#endif  // LT_HOST_ONLY

int lt_fn_est_host(int64_t n_query, const double *kvec4, const double *qvec4, const double *tvec3, const int64_t *pt_off,
                   const double *p3d3, const double *p2d2, const int64_t *l3d_off, const double *line3d6,
                   const int64_t *seg_off, const int32_t *l3d_ids, const double *seg4, const lt_est_config *cfg,
                   int64_t trace_cap, int host_threads, double *pose7, double *dstats3, int32_t *istats12, int32_t *inliers,
                   double *trace) {
  std::string msg;
  LoopPlan pl;
  const bool bad = make_loop_plan(n_query, kvec4, qvec4, tvec3, pt_off, p3d3, p2d2, l3d_off, line3d6, seg_off, l3d_ids, seg4, cfg,
                                  trace_cap, pl, msg);
  if (int rc = g_host_error.check("lt_fn_est_host", bad, msg)) return rc;
  LoopResult res;
  run_loop_host(pl, host_threads, res);
  copy_loop_out(pl, res.st.data(), res.inl.data(), res.trace.data(), pose7, dstats3, istats12, inliers, trace);
  return LT_OK;
}

uint32_t lt_fn_est_num_required(const double ratios2[2], double success_probability, int solver, uint32_t min_it, uint32_t max_it) {
  if (!ratios2 || solver < 0 || solver > 3) return 0;
  return eh_num_required(ratios2, 1.0 - success_probability, solver, min_it, max_it);
}

double lt_fn_est_log(double x) { return eh_log(x); }

int lt_fn_est_probabilities(const double ratios2[2], const uint32_t its4[4], const int32_t flags4[4], int32_t n_pts,
                            int32_t n_lines, uint32_t min_it, double prior4[4], double prob4[4]) {
  if (!ratios2 || !its4 || !flags4 || !prior4 || !prob4 || n_pts < 0 || n_lines < 0) return LT_ERR_ARGUMENT;
  EhState s;
  EhOpt o;
  o.min_it = min_it;
  int flags = 0;
  for (int i = 0; i < 4; ++i) { flags |= (flags4[i] ? 1 : 0) << i; s.it_solver[i] = its4[i]; }
  s.ratios[0] = ratios2[0]; s.ratios[1] = ratios2[1];
  const bool any = eh_priors(flags, n_pts, n_lines, s.prior);
  eh_freeze(o, s);
  for (int i = 0; i < 4; ++i) { prior4[i] = s.prior[i]; prob4[i] = s.prob[i]; }
  return any ? 1 : 0;
}

int lt_fn_est_minimal_host(int kind, int64_t n, const double *xs, const double *Xs, const double *ls, const double *Cs,
                           const double *Vs, int n_threads, double *poses56, int32_t *counts) {
  std::string msg;
  Plan pl;
  if (int rc = g_host_error.check("lt_fn_est_minimal_host", make_plan(kind, n, xs, Xs, ls, Cs, Vs, pl, msg), msg)) return rc;
  run_host(pl, n_threads, poses56, counts);
  return LT_OK;
}

}  // extern "C"
