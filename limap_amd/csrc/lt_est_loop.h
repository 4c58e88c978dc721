// lt_est_loop.h -- the hybrid LO-MSAC of limap.estimators.absolute_pose (PointLineAbsolutePoseHybridRansac::EstimateModel,
// pl_absolute_pose_hybrid_ransac.h:63-249) by rounds: shared text of the device (lt_kernels_est.hip) and
// the host twin (lt_est.cpp).  limap's own control flow is restated in its order; RansacLib's parts (the sampler, the
// shuffles, NumRequiredIterations) and the powers and the logarithm they need are this project's definition below.
//
// A round is three steps for every running query:
//   eh_draw_solve  per iteration slot: the solver type under the probabilities frozen at the round's start, the minimal
//                  sample, its inputs as JointPoseEstimator::MinimalSolver builds them, es_solve
//   eh_score_slot  per pose: ScoreModel against every correspondence of the query
//   eh_replay      per query, in iteration order: new best, local optimisation when due, termination update, the
//                  per-solver cap; iterations past the break do not count.  With round_size 1 this is upstream's loop.
// The group G supplies what a wave does together: score() (every correspondence's squared error into r2[], the MSAC sum
// in lane order), lm() (lc_lm over the gathered block table), lead() and sync().  Everything else is scalar and runs on
// every lane alike; lists and tables in memory are written by the lead lane between two sync().
#pragma once

#include "lt_est.h"
#include "lt_loc.h"

namespace lt {

constexpr int kEhTrace = 12;          // doubles per trace record
constexpr int kEhInts = 8;            // scratch integers per query
constexpr unsigned kEhLoKey = 0x80000000u;  // the iteration field of a local optimisation's draw key: kEhLoKey | lo id
constexpr double kEhLn2 = 0.6931471805599453;

struct EhOpt {
  double thr2[2], w[2];  // squared_inlier_thresholds_, data_type_weights_: points, lines
  double success_probability, threshold_multiplier;
  double min_depth, overlap;  // cheirality_min_depth, cheirality_overlap_pixels
  double weight_line, weight_point;  // LeastSquares' block weights
  unsigned long long seed;
  unsigned min_it, max_it, max_it_solver, lo_start;
  int num_lo_steps, num_lsq, min_sample_mult, non_min_mult;
  int final_lsq, round_size, solver_flags, trace_cap;
  LcCfg lsq;  // LeastSquares: the caller's cost function, weight, loss, iteration cap
};

struct EhQuery {
  double k[4], q0[4], t0[3];
  long long c0;  // its correspondences [c0, c0 + n_pts + n_lines) of the table, the points first
  int n_pts, n_lines;
};

struct EhState {
  double best[7], best_score;  // best_model, stats.best_model_score
  double minm[7], min_score;   // best_minimal_model, best_min_model_score
  double ratios[2], prob[4], prior[4];
  unsigned it_total, it_solver[4], max_it_solver[4];
  int best_solver, n_lo, best_num_inliers, n_inl[2], done, n_trace, pad_;
};

struct EhDev {
  EhOpt opt;
  long long n_queries, stride;
  const EhQuery *qs;
  EhState *st;
  const double *tab;  // kLcScoreFields x stride
  const int *l3d_id;  // per correspondence (lines: the id of its 3D line within the query)
  double *r2;         // stride
  int *inl, *base, *samp, *mark, *out_inl;  // stride each
  double *blk;        // kLcFields x stride
  int *ints;          // kEhInts per query
  double *r_poses, *r_scores;  // per query round_size x 8 x 7, round_size x 8
  int *r_counts, *r_solver;    // per query round_size
  double *trace;      // per query trace_cap x kEhTrace
  int *n_done;
};

// ---- this project's definition of the third parties' parts ----
LT_HD unsigned long long eh_fmix(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// lt_kernels_fit.hip's generator keyed by (seed, query, iteration, stream)
struct EhRng {
  unsigned long long k, c;
  LT_HD void init(unsigned long long seed, long long query, unsigned iter, unsigned stream) {
    const unsigned long long g = 0x9E3779B97F4A7C15ull;
    k = eh_fmix(seed + g);
    k = eh_fmix(k ^ ((unsigned long long)query + g));
    k = eh_fmix(k ^ ((unsigned long long)iter + g));
    k = eh_fmix(k ^ ((unsigned long long)stream + g));
    c = 0;
  }
  LT_HD unsigned draw() {
    ++c;
    return (unsigned)(eh_fmix(k + c * 0x9E3779B97F4A7C15ull) >> 32);
  }
  LT_HD int uniform(int n) {  // n >= 1
    const unsigned un = (unsigned)n, thr = (0u - un) % un;
    for (;;) {
      const unsigned u = draw();
      if (u >= thr) return (int)(u % un);
    }
  }
  LT_HD double unit() { return ((double)draw() + 0.5) / 4294967296.0; }  // in (0, 1)
};

// x^n by squaring, n >= 0
LT_HD double eh_powi(double x, unsigned n) {
  double r = 1.0;
  while (n) {
    if (n & 1u) r = r * x;
    x = x * x;
    n >>= 1;
  }
  return r;
}
// the natural logarithm of a positive finite x: x = m 2^e with m in [1/sqrt 2, sqrt 2), log m = 2 atanh((m - 1) / (m + 1))
// by 14 terms of its series
LT_HD double eh_log(double x) {
  int e = 0;
  for (int i = 0; i < 1100 && x >= 1.4142135623730951; ++i) { x = x * 0.5; ++e; }
  for (int i = 0; i < 1100 && x < 0.7071067811865476; ++i) { x = x * 2.0; --e; }
  const double s = (x - 1.0) / (x + 1.0), s2 = s * s;
  double acc = 0.0;
  for (int k = 13; k >= 0; --k) acc = acc * s2 + 1.0 / (double)(2 * k + 1);
  return (double)e * kEhLn2 + 2.0 * s * acc;
}
LT_HD int eh_min_size(int solver, int type) { return type == 0 ? 3 - solver : solver; }  // min_sample_sizes
// NumRequiredIterations: p = prod ratio_j^size_j; ceil(log(1 - success) / log(1 - p) + 0.5) within [min, max];
// p <= 0 gives max, p >= 1 gives min
LT_HD unsigned eh_num_required(const double ratios[2], double prob_missing, int solver, unsigned min_it, unsigned max_it) {
  const double p = eh_powi(ratios[0], (unsigned)eh_min_size(solver, 0)) * eh_powi(ratios[1], (unsigned)eh_min_size(solver, 1));
  if (!(p > 0.0)) return max_it;
  if (p >= 1.0) return min_it;
  const double den = eh_log(1.0 - p);
  if (!(den < 0.0)) return max_it;  // 1 - p rounds to 1
  const double v = eh_log(prob_missing) / den + 0.5;
  unsigned n;
  if (!(v < (double)max_it)) n = max_it;
  else if (v <= 0.0) n = 0;
  else {
    n = (unsigned)v;
    if ((double)n < v) ++n;  // ceil
    if (n > max_it) n = max_it;
  }
  return n < min_it ? min_it : n;
}
// combination() of hybrid_pose_estimator.h:118-126
LT_HD double eh_comb(unsigned n, unsigned m) {
  unsigned long long num = 1, den = 1;
  for (unsigned i = 0; i < m; ++i) num *= (unsigned long long)(n - i);
  for (unsigned i = 0; i < m; ++i) den *= (unsigned long long)(i + 1);
  return (double)(num / den);
}
// solver_probabilities (hybrid_pose_estimator.h:76-90) and VerifyData (:588-616); false: no solver can run
LT_HD bool eh_priors(int flags, int n_pts, int n_lines, double prior[4]) {
  bool any = false;
  for (int s = 0; s < 4; ++s) {
    const int a = eh_min_size(s, 0), b = eh_min_size(s, 1);
    prior[s] = 0.0;
    if (((flags >> s) & 1) && a <= n_pts && b <= n_lines) prior[s] = eh_comb((unsigned)n_pts, (unsigned)a) * eh_comb((unsigned)n_lines, (unsigned)b);
    any = any || prior[s] > 0.0;
  }
  return any;
}
// SelectMinimalSolver's probabilities (:258-300, Eq. 1), frozen for a round
LT_HD void eh_freeze(const EhOpt &o, EhState &s) {
  const double sum_ratios = s.ratios[0] + s.ratios[1];
  for (int i = 0; i < 4; ++i) {
    if (sum_ratios == 0.0) { s.prob[i] = s.prior[i]; continue; }
    double num_iters = (double)s.it_solver[i];
    if (num_iters > 0.0) num_iters -= 1.0;
    double all = 1.0;
    for (int j = 0; j < 2; ++j) all *= eh_powi(s.ratios[j], (unsigned)eh_min_size(i, j));
    if (num_iters < (double)o.min_it) s.prob[i] = all * s.prior[i];
    else s.prob[i] = all * eh_powi(1.0 - all, (unsigned)num_iters) * s.prior[i];
  }
}
// :302-314 with kProb = u sum; where rounding leaves no solver, the last one with a prior
LT_HD int eh_select(const EhState &s, double u) {
  double sum = 0.0;
  for (int i = 0; i < 4; ++i) sum += s.prob[i];
  const double kprob = u * sum;
  double cur = 0.0;
  int last = -1;
  for (int i = 0; i < 4; ++i) {
    if (s.prior[i] == 0.0) continue;
    last = i;
    cur += s.prob[i];
    if (kprob <= cur) return i;
  }
  return last;
}

LT_HD LcScoreCfg eh_score_cfg(const EhOpt &o, const EhQuery &qr) {
  LcScoreCfg sc;
  sc.cfg = o.lsq;
  sc.cfg.weight = kLcNone;
  sc.cfg.loss = kLcTrivial;
  sc.cfg.loss_a = 1.0;
  sc.min_depth = o.min_depth;
  sc.overlap = o.overlap;
  for (int i = 0; i < 2; ++i) { sc.thr2[i] = o.thr2[i]; sc.w[i] = o.w[i]; }
  sc.n_points = qr.n_pts;
  sc.n_lines = qr.n_lines;
  sc.want_msac = 1;
  sc.pad_ = 0;
  return sc;
}

// the group G of the replay: what a wave does together, over the lanes (LmWaveLanes in the kernels, LmHostLanes in the
// host twin)
template <class Lanes>
struct EhWave {
  Lanes lanes;
  const EhDev &d;
  const EhQuery &qr;
  LcScoreCfg sc;
  LT_HD bool lead() const { return lanes.lead(); }
  LT_HD void sync() const { lanes.sync(); }
  LT_HD double score_impl(const double m[7], bool store) const {
    const double sum = lc_msac_sum(lanes, sc, qr.k, m, m + 4, d.tab, d.stride, qr.c0, qr.n_pts, qr.n_lines,
                                   [&](int i, bool, double r2) { if (store) d.r2[qr.c0 + i] = r2; });
    if (store) lanes.sync();
    return sum;
  }
  LT_HD double score(const double m[7]) const { return score_impl(m, true); }
  LT_HD void lm(const LcCfg &cfg, int n_blocks, double p[7], int *code) const {
    LcGroup<Lanes> grp{lanes, cfg, d.blk, d.stride, qr.c0, n_blocks, qr.k};
    double F0, F1;
    int it;
    lc_lm(grp, n_blocks, cfg.max_iter, p, &F0, &F1, &it, code);
  }
};

// ---- step 1: one iteration slot of a round ----
ES_HD void eh_draw_solve(const EhDev &d, long long q, int slot) {
  const EhState &s = d.st[q];
  const EhQuery &qr = d.qs[q];
  const long long ri = q * d.opt.round_size + slot;
  d.r_counts[ri] = 0;
  d.r_solver[ri] = -1;
  if (s.done) return;
  const unsigned max_it = d.opt.max_it > d.opt.min_it ? d.opt.max_it : d.opt.min_it;
  if ((unsigned long long)s.it_total + (unsigned)slot >= max_it) return;
  EhRng rng;
  rng.init(d.opt.seed, q, s.it_total + (unsigned)slot, 0);
  const int solver = eh_select(s, rng.unit());
  d.r_solver[ri] = solver;
  if (solver < 0) return;
  const int np = 3 - solver, nl = solver;
  int pick[3];
  double x[3][3], X[3][3], l[3][3], C[3][3], V[3][3];
  for (int a = 0; a < 3; ++a)
    for (int c = 0; c < 3; ++c) x[a][c] = X[a][c] = l[a][c] = C[a][c] = V[a][c] = 0.0;
  // without replacement within a data type: the j-th draw is uniform over the n - j left, in ascending index order
  for (int type = 0; type < 2; ++type) {
    const int cnt = type == 0 ? np : nl, n = type == 0 ? qr.n_pts : qr.n_lines;
    for (int j = 0; j < cnt; ++j) {
      int v = rng.uniform(n - j);
      int sorted[3], ns = 0;
      for (int a = 0; a < j; ++a) {  // insertion into the ascending list of what is taken
        int p = ns++;
        while (p > 0 && sorted[p - 1] > pick[a]) { sorted[p] = sorted[p - 1]; --p; }
        sorted[p] = pick[a];
      }
      for (int a = 0; a < ns; ++a)
        if (v >= sorted[a]) ++v;
      pick[j] = v;
      const long long i = qr.c0 + (type == 0 ? 0 : qr.n_pts) + v;
      double f[10];
      for (int c = 0; c < 10; ++c) f[c] = d.tab[(long long)c * d.stride + i];
      if (type == 0) {  // joint_pose_estimator.cc:92-95
        const double b0 = (f[6] - qr.k[2]) / qr.k[0], b1 = (f[7] - qr.k[3]) / qr.k[1];
        const double n0 = sqrt((b0 * b0 + b1 * b1) + 1.0);
        x[j][0] = b0 / n0; x[j][1] = b1 / n0; x[j][2] = 1.0 / n0;
        for (int c = 0; c < 3; ++c) X[j][c] = f[c];
      } else {  // :99-107
        double e[2][3];
        for (int a = 0; a < 2; ++a) {
          const double b0 = (f[6 + 2 * a] - qr.k[2]) / qr.k[0], b1 = (f[7 + 2 * a] - qr.k[3]) / qr.k[1];
          const double n0 = sqrt((b0 * b0 + b1 * b1) + 1.0);
          e[a][0] = b0 / n0; e[a][1] = b1 / n0; e[a][2] = 1.0 / n0;
        }
        const double c0 = e[0][1] * e[1][2] - e[0][2] * e[1][1], c1 = e[0][2] * e[1][0] - e[0][0] * e[1][2],
                     c2 = e[0][0] * e[1][1] - e[0][1] * e[1][0];
        const double n0 = sqrt((c0 * c0 + c1 * c1) + c2 * c2);
        l[j][0] = c0 / n0; l[j][1] = c1 / n0; l[j][2] = c2 / n0;
        for (int c = 0; c < 3; ++c) {
          C[j][c] = f[c];
          V[j][c] = d.tab[(long long)(10 + c) * d.stride + i];  // the unit direction (lc_item_prep)
        }
        if (!(n0 > 0.0)) { for (int c = 0; c < 3; ++c) l[j][c] = 0.0; }  // a segment of zero length: no pose
      }
    }
  }
  double out[kEsMaxSol][kEsPoseDoubles];
  const int n = es_solve(np, x, X, l, C, V, out);
  double *dst = d.r_poses + ri * (kEsMaxSol * kEsPoseDoubles);
  for (int m = 0; m < n; ++m)
    for (int c = 0; c < kEsPoseDoubles; ++c) dst[m * kEsPoseDoubles + c] = out[m][c];
  d.r_counts[ri] = n;
}

// ---- step 3: the replay ----
struct EhCtx {
  const EhDev &d;
  long long q;
  const EhQuery &qr;
  int *ints;
};

template <class G>
LT_HD void eh_trace(G &g, const EhCtx &c, EhState &s, const double rec[kEhTrace]) {
  if (s.n_trace < c.d.opt.trace_cap && g.lead()) {
    double *t = c.d.trace + (c.q * c.d.opt.trace_cap + s.n_trace) * kEhTrace;
    for (int i = 0; i < kEhTrace; ++i) t[i] = rec[i];
  }
  if (c.d.opt.trace_cap > 0) s.n_trace += 1;  // counts what a larger buffer would hold
}

// GetInliers (:360-393) of the model whose errors stand in r2: list[0 .. n0) the points, then the lines, as indices
// within their type; counts through ints[0], ints[1]
template <class G>
LT_HD void eh_inliers(G &g, const EhCtx &c, const double thr[2], int *list, int cnt[2]) {
  if (g.lead()) {
    int n = 0;
    for (int i = 0; i < c.qr.n_pts; ++i)
      if (c.d.r2[c.qr.c0 + i] < thr[0]) list[c.qr.c0 + n++] = i;
    c.ints[0] = n;
    for (int i = 0; i < c.qr.n_lines; ++i)
      if (c.d.r2[c.qr.c0 + c.qr.n_pts + i] < thr[1]) list[c.qr.c0 + n++] = i;
    c.ints[1] = n - c.ints[0];
  }
  g.sync();
  cnt[0] = c.ints[0];
  cnt[1] = c.ints[1];
  g.sync();
}

// RandomShuffleAndResize: a partial Fisher-Yates shuffle of list[0 .. n), the first k kept (lead lane)
LT_HD void eh_shuffle(EhRng &rng, int *list, int n, int k) {
  for (int j = 0; j < k && j < n; ++j) {
    const int r = j + rng.uniform(n - j);
    const int t = list[j];
    list[j] = list[r];
    list[r] = t;
  }
}

// The block table of JointLocEngine for a sample (joint_pose_estimator.cc:137-158, hybrid_localization.cc:98-128):
// samp[0 .. np) points, samp[np .. np + nl) lines, indices within their type.  Lines are grouped by their 3D line in
// the order its id first appears, each group's segments in sample order with weight wl length / sum_lengths; then the
// points with weight wp.  Lead lane.
LT_HD void eh_gather(const EhCtx &c, const int *samp, int np, int nl, double wl, double wp) {
  const EhDev &d = c.d;
  const long long c0 = c.qr.c0, st = d.stride;
  const int *sl = samp + np;
  long long b = c0;
  for (int a = 0; a < nl; ++a) d.mark[c0 + a] = 0;
  for (int a = 0; a < nl; ++a) {
    if (d.mark[c0 + a]) continue;
    const int id = d.l3d_id[c0 + c.qr.n_pts + sl[a]];
    double sum = 0.0;
    for (int e = a; e < nl; ++e) {
      const long long i = c0 + c.qr.n_pts + sl[e];
      if (d.l3d_id[i] != id) continue;
      const double ex = d.tab[8 * st + i] - d.tab[6 * st + i], ey = d.tab[9 * st + i] - d.tab[7 * st + i];
      sum += sqrt(ex * ex + ey * ey);
    }
    for (int e = a; e < nl; ++e) {
      const long long i = c0 + c.qr.n_pts + sl[e];
      if (d.l3d_id[i] != id) continue;
      d.mark[c0 + e] = 1;
      const double ex = d.tab[8 * st + i] - d.tab[6 * st + i], ey = d.tab[9 * st + i] - d.tab[7 * st + i];
      for (int f = 0; f < 10; ++f) d.blk[(long long)f * st + b] = d.tab[(long long)f * st + i];
      d.blk[10 * st + b] = wl * sqrt(ex * ex + ey * ey) / sum;
      d.blk[11 * st + b] = 0.0;
      ++b;
    }
  }
  for (int a = 0; a < np; ++a, ++b) {
    const long long i = c0 + samp[a];
    for (int f = 0; f < 10; ++f) d.blk[(long long)f * st + b] = d.tab[(long long)f * st + i];
    d.blk[10 * st + b] = wp;
    d.blk[11 * st + b] = 1.0;
  }
}

// JointLocEngine::Solve on the gathered blocks and IsSolutionUsable; the pose becomes CameraPose(GetFinalR(), GetFinalT())
template <class G>
LT_HD bool eh_refine(G &g, const EhCtx &c, const LcCfg &cfg, int n_blocks, double p[7]) {
  double w[7];
  lm_normalise_q(p, w);
  for (int i = 0; i < 3; ++i) w[4 + i] = p[4 + i];
  int code = 0;
  g.lm(cfg, n_blocks, w, &code);
  g.sync();
  if (code > 2) return false;
  double nq[4], R[3][3];
  lm_normalise_q(w, nq);
  es_rotation(nq, R);
  rf_quat_from_matrix(R, p);
  for (int i = 0; i < 3; ++i) p[4 + i] = w[4 + i];
  return true;
}

LT_HD void eh_update_best(double score, const double m[7], int solver, double *best_score, double best[7], int *best_solver) {
  if (score < *best_score) {
    *best_score = score;
    for (int i = 0; i < 7; ++i) best[i] = m[i];
    *best_solver = solver;
  }
}

// LeastSquaresFit (:547-573)
template <class G>
LT_HD void eh_lsq_fit(G &g, const EhCtx &c, const double thr[2], int solver_type, unsigned lo_id, unsigned stream, double m[7]) {
  const EhOpt &o = c.d.opt;
  g.score(m);
  int cnt[2];
  eh_inliers(g, c, thr, c.d.inl, cnt);
  int size[2];
  for (int i = 0; i < 2; ++i) {
    size[i] = eh_min_size(solver_type, i);
    if (cnt[i] < size[i]) return;
    size[i] *= o.min_sample_mult;
    if (size[i] > cnt[i]) size[i] = cnt[i];
  }
  if (g.lead()) {
    EhRng rng;
    rng.init(o.seed, c.q, kEhLoKey | lo_id, stream);
    int *pts = c.d.inl + c.qr.c0, *lns = pts + cnt[0];
    eh_shuffle(rng, pts, cnt[0], size[0]);
    eh_shuffle(rng, lns, cnt[1], size[1]);
    int *sm = c.d.samp + c.qr.c0;
    for (int a = 0; a < size[0]; ++a) sm[a] = pts[a];
    for (int a = 0; a < size[1]; ++a) sm[size[0] + a] = lns[a];
    eh_gather(c, sm, size[0], size[1], o.weight_line, o.weight_point);
  }
  g.sync();
  eh_refine(g, c, o.lsq, size[0] + size[1], m);
}

// UpdateRANSACTerminationCriteria (:395-426): the inliers of the model into out_inl, the ratios, the caps
template <class G>
LT_HD void eh_update_term(G &g, const EhCtx &c, EhState &s, const double m[7]) {
  const EhOpt &o = c.d.opt;
  g.score(m);
  eh_inliers(g, c, o.thr2, c.d.out_inl, s.n_inl);
  s.best_num_inliers = s.n_inl[0] + s.n_inl[1];
  s.ratios[0] = c.qr.n_pts > 0 ? (double)s.n_inl[0] / (double)c.qr.n_pts : 0.0;
  s.ratios[1] = c.qr.n_lines > 0 ? (double)s.n_inl[1] / (double)c.qr.n_lines : 0.0;
  for (int k = 0; k < 4; ++k) s.max_it_solver[k] = eh_num_required(s.ratios, 1.0 - o.success_probability, k, o.min_it, o.max_it_solver);
}

// LocalOptimization (:431-545)
template <class G>
LT_HD void eh_lo(G &g, const EhCtx &c, EhState &s, int solver_type, double model[7], double *score_best, int *best_solver) {
  const EhOpt &o = c.d.opt;
  const unsigned lo_id = (unsigned)s.n_lo;
  double rel[2], upd[2];
  for (int i = 0; i < 2; ++i) {
    upd[i] = (o.threshold_multiplier - 1.0) * o.thr2[i] / (double)(o.num_lsq - 1);
    rel[i] = o.thr2[i] * o.threshold_multiplier;
  }
  const double score_in = *score_best;
  double m_init[7];
  for (int i = 0; i < 7; ++i) m_init[i] = model[i];
  eh_lsq_fit(g, c, rel, solver_type, lo_id, 0, m_init);
  double score = g.score(m_init);
  eh_update_best(score, m_init, solver_type, score_best, model, best_solver);
  int nb[2];
  eh_inliers(g, c, o.thr2, c.d.base, nb);
  const int n_base = nb[0] + nb[1];
  int non_min = 3 * o.non_min_mult < n_base / 2 ? 3 * o.non_min_mult : n_base / 2;
  if (non_min < 6) non_min = 6;
  const int n_samp = non_min < n_base ? non_min : n_base;
  int skipped = 0;
  for (int r = 0; r < o.num_lo_steps; ++r) {
    const unsigned st0 = 1u + (unsigned)r * (unsigned)(o.num_lsq + 2);
    if (n_samp < 6) { ++skipped; continue; }  // NonMinimalSolver: fewer than non_minimal_sample_size()
    if (g.lead()) {
      // inliers_base_all_type: the points, then the lines offset by the number of points
      int *all = c.d.inl + c.qr.c0;
      const int *bs = c.d.base + c.qr.c0;
      for (int a = 0; a < nb[0]; ++a) all[a] = bs[a];
      for (int a = nb[0]; a < n_base; ++a) all[a] = bs[a] + c.qr.n_pts;
      EhRng rng;
      rng.init(o.seed, c.q, kEhLoKey | lo_id, st0);
      eh_shuffle(rng, all, n_base, n_samp);
      // NonMinimalSolver's split (:143-158): the points of the sample in order, then its lines
      int *sm = c.d.samp + c.qr.c0;
      int np = 0, nl = 0;
      for (int a = 0; a < n_samp; ++a)
        if (all[a] < c.qr.n_pts) sm[np++] = all[a];
      for (int a = 0; a < n_samp; ++a)
        if (all[a] >= c.qr.n_pts) sm[np + nl++] = all[a] - c.qr.n_pts;
      c.ints[2] = np;
      eh_gather(c, sm, np, nl, 1.0, 1.0);
    }
    g.sync();
    double m[7] = {1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // a default-constructed pose
    LcCfg nm = o.lsq;  // weights 1, TrivialLoss
    nm.loss = kLcTrivial;
    nm.loss_a = 1.0;
    if (!eh_refine(g, c, nm, n_samp, m)) { ++skipped; continue; }
    score = g.score(m);
    eh_update_best(score, m, solver_type, score_best, model, best_solver);
    eh_lsq_fit(g, c, o.thr2, solver_type, lo_id, st0 + 1, m);
    double cur[2] = {rel[0], rel[1]};
    for (int i = 0; i < o.num_lsq; ++i) {
      eh_lsq_fit(g, c, cur, solver_type, lo_id, st0 + 2 + (unsigned)i, m);
      score = g.score(m);
      eh_update_best(score, m, solver_type, score_best, model, best_solver);
      for (int j = 0; j < 2; ++j) cur[j] -= upd[j];
    }
  }
  const double rec[kEhTrace] = {1.0, (double)lo_id, (double)solver_type, (double)nb[0], (double)nb[1], (double)n_samp,
                                rel[0], upd[0], score_in, *score_best, (double)s.it_total, (double)skipped};
  eh_trace(g, c, s, rec);
}

// the end of EstimateModel (:214-248)
template <class G>
LT_HD void eh_finish(G &g, const EhCtx &c, EhState &s) {
  const EhOpt &o = c.d.opt;
  if (s.it_total <= o.lo_start && s.best_score < kMaxDist) {
    s.n_lo += 1;
    eh_lo(g, c, s, s.best_solver, s.best, &s.best_score, &s.best_solver);
    eh_update_term(g, c, s, s.best);
  }
  double applied = 0.0, score = kMaxDist;
  if (o.final_lsq) {
    double m[7];
    for (int i = 0; i < 7; ++i) m[i] = s.best[i];
    if (g.lead()) {  // LeastSquares(stats.inlier_indices)
      int *sm = c.d.samp + c.qr.c0;
      for (int a = 0; a < s.best_num_inliers; ++a) sm[a] = c.d.out_inl[c.qr.c0 + a];
      eh_gather(c, sm, s.n_inl[0], s.n_inl[1], o.weight_line, o.weight_point);
    }
    g.sync();
    eh_refine(g, c, o.lsq, s.best_num_inliers, m);
    score = g.score(m);
    if (score < s.best_score) {
      s.best_score = score;
      for (int i = 0; i < 7; ++i) s.best[i] = m[i];
      eh_update_term(g, c, s, s.best);
      applied = 1.0;
    }
  }
  const double rec[kEhTrace] = {2.0, (double)s.it_total, (double)o.final_lsq, applied, score, s.best_score,
                                (double)s.best_num_inliers, (double)s.n_lo, (double)s.best_solver, 0.0, 0.0, 0.0};
  eh_trace(g, c, s, rec);
  s.done = 1;
}

// one round of a query (:113-212).  Returns with s.done set when the run has ended.
template <class G>
LT_HD void eh_replay(G &g, const EhDev &d, long long q, EhState &s) {
  const EhOpt &o = d.opt;
  const EhCtx c{d, q, d.qs[q], d.ints + q * kEhInts};
  const unsigned max_it = o.max_it > o.min_it ? o.max_it : o.min_it;
  bool ended = false;
  for (int slot = 0; slot < o.round_size && !ended; ++slot) {
    if (s.it_total >= max_it) { ended = true; break; }
    double flags = 0.0;
    if (s.it_total == o.lo_start && s.min_score < kMaxDist) {
      s.n_lo += 1;
      eh_lo(g, c, s, s.best_solver, s.best, &s.best_score, &s.best_solver);
      eh_update_term(g, c, s, s.best);
      flags += 4.0;
    }
    const long long ri = q * o.round_size + slot;
    const int solver = d.r_solver[ri], n_models = d.r_counts[ri];
    if (solver < 0) { ended = true; break; }
    s.it_solver[solver] += 1;
    double best_local = kMaxDist;
    int best_id = 0;
    bool skip_cap = false;
    if (n_models > 0) {
      for (int m = 0; m < n_models; ++m) {  // GetBestEstimatedModelId
        const double sc = d.r_scores[ri * kEsMaxSol + m];
        if (sc < best_local) { best_local = sc; best_id = m; }
      }
      if (best_local < s.min_score || s.it_total == o.lo_start) {
        const bool k_best = best_local < s.min_score;
        if (k_best) {
          s.min_score = best_local;
          for (int i = 0; i < 7; ++i) s.minm[i] = d.r_poses[(ri * kEsMaxSol + best_id) * kEsPoseDoubles + i];
          eh_update_best(s.min_score, s.minm, solver, &s.best_score, s.best, &s.best_solver);
          flags += 1.0;
        }
        const bool run_lo = s.it_total >= o.lo_start && s.min_score < kMaxDist;
        if (!k_best && !run_lo) {
          skip_cap = true;  // upstream's `continue`
        } else {
          if (run_lo) {
            s.n_lo += 1;
            double score = s.min_score;
            eh_lo(g, c, s, s.best_solver, s.minm, &score, &s.best_solver);
            eh_update_best(score, s.minm, solver, &s.best_score, s.best, &s.best_solver);
            flags += 2.0;
          }
          eh_update_term(g, c, s, s.best);
        }
      }
    }
    const bool cap = !skip_cap && s.it_solver[solver] >= s.max_it_solver[solver];
    if (cap) flags += 8.0;
    const double rec[kEhTrace] = {0.0, (double)s.it_total, (double)solver, (double)n_models, best_local, flags, s.best_score,
                                  s.ratios[0], s.ratios[1], (double)s.max_it_solver[solver], (double)s.it_solver[solver],
                                  (double)s.best_num_inliers};
    eh_trace(g, c, s, rec);
    if (cap) { ended = true; break; }
    s.it_total += 1;
  }
  if (!ended && s.it_total >= max_it) ended = true;
  if (ended) eh_finish(g, c, s);
  else eh_freeze(o, s);
}

// the state of a query before its first round
LT_HD void eh_init(const EhOpt &o, const EhQuery &qr, EhState &s) {
  lm_normalise_q(qr.q0, s.best);
  for (int i = 0; i < 3; ++i) s.best[4 + i] = qr.t0[i];
  for (int i = 0; i < 7; ++i) s.minm[i] = s.best[i];
  s.best_score = s.min_score = kMaxDist;
  s.ratios[0] = s.ratios[1] = 0.0;
  const unsigned cap = o.max_it_solver > o.min_it ? o.max_it_solver : o.min_it;
  for (int i = 0; i < 4; ++i) { s.it_solver[i] = 0; s.max_it_solver[i] = cap; }
  s.it_total = 0;
  s.best_solver = -1;
  s.n_lo = s.best_num_inliers = s.n_inl[0] = s.n_inl[1] = s.n_trace = s.pad_ = 0;
  s.done = eh_priors(o.solver_flags, qr.n_pts, qr.n_lines, s.prior) ? 0 : 1;
  eh_freeze(o, s);
}

void launch_est_round(hipStream_t st, const EhDev &dev);

}  // namespace lt
