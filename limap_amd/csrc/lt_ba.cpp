// lt_ba.cpp -- the bundle adjustment with free poses, points and lines of limap.optimize.hybrid_bundle_adjustment
// (HybridBAEngine: hybrid_bundle_adjustment.cc:18-310) with constant intrinsics.  Validation, the residual blocks in
// SetUp()'s order with their ScaledLoss weights, the index tables of the Schur complement, upload, the launch loop of
// lt_kernels_ba.hip and the download; lt_fn_ba_host is the whole solve in plain C++ from the same inline functions
// (lt_ba.h) with every reduction in the device's order, so both agree bit for bit.

#include "lt_host.h"
#include "lt_ba.h"
#include "lt_ingest.h"
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

// what a call passes in (the arguments of lt_ba_arrays)
struct Input {
  int n_img;
  const int32_t *img_ids;
  const double *k, *q, *t;
  int64_t n_pt;
  const double *pt3;
  const int64_t *pt_off;
  const int32_t *pt_img;
  const double *pt_xy;
  int64_t n_ln;
  const double *line6;
  const int64_t *ln_off;
  const int32_t *ln_img;
  const double *l2d4, *l3d6;
  const lt_ba_config *cfg;
};

struct Plan {
  int C = 0, NS = 0, NB = 0, NPair = 0, NP = 0;  // NP: point structures (they come first)
  double alpha = 10.0;
  int max_iter = 0, num_outliers = 0, poll = kBaPollDefault, kernel_timers = 0;
  bool constant_pose = false;     // the tracks separate: point tracks only, every one its own problem
  std::vector<int> cam_row;       // per active image its row of the input
  std::vector<double> kvec, pose0, sp0;
  std::vector<BaStruct> st;
  std::vector<BaBlk> blk;
  std::vector<int> pair_cam, pair_s, pair_blk_off, pair_blk, cam_blk_off, cam_blk, sch_off, sch;
  std::vector<double> l3d;        // 6 per line support, input order
  std::vector<long long> ln_off;
};

int check_config(const lt_ba_config *c, std::string &msg) {
  if (!c) { msg = "null configuration"; return 1; }
  if (!c->constant_intrinsics) { msg = "constant_intrinsics=0 is not built (intrinsics are constant)"; return 1; }
  if (!(c->geometric_alpha >= 0.0) || !(c->geometric_alpha <= 700.0)) { msg = "geometric_alpha outside [0, 700]"; return 1; }
  if (c->max_num_iterations < 0) { msg = "max_num_iterations is negative"; return 1; }
  if (!std::isfinite(c->lw_point)) { msg = "lw_point is not finite"; return 1; }
  if (c->poll_interval < 0) { msg = "poll_interval is negative"; return 1; }
  return 0;
}

int make_plan(const Input &in, Plan &pl, std::string &msg) {
  if (check_config(in.cfg, msg)) return 1;
  const lt_ba_config &cfg = *in.cfg;
  IdRows id2row;
  if (ingest_cams(in.n_img, in.img_ids, in.k, in.q, in.t, id2row, msg)) return 1;
  if (in.n_pt < 0 || in.n_ln < 0) { msg = "bad track counts"; return 1; }
  pl.constant_pose = cfg.constant_pose != 0;
  if (pl.constant_pose && in.n_ln > 0) {
    msg = "constant_pose=1 takes point tracks only: with constant cameras every line track is its own problem, which lt_refine_arrays solves";
    return 1;
  }
  if (in.n_pt > 0) {
    msg = offsets_msg("point track", in.n_pt, in.pt_off);
    if (!msg.empty()) return 1;
  }
  if (in.n_ln > 0) {
    msg = offsets_msg("line track", in.n_ln, in.ln_off);
    if (!msg.empty()) return 1;
  }
  const long long MP = in.n_pt > 0 ? in.pt_off[in.n_pt] : 0, ML = in.n_ln > 0 ? in.ln_off[in.n_ln] : 0;
  if ((in.n_pt > 0 && !in.pt3) || (MP > 0 && (!in.pt_img || !in.pt_xy)) || (in.n_ln > 0 && !in.line6) ||
      (ML > 0 && (!in.ln_img || !in.l2d4 || !in.l3d6))) {
    msg = "null track arrays";
    return 1;
  }
  if (!all_finite(in.pt3, 3 * in.n_pt) || !all_finite(in.pt_xy, 2 * MP) || !all_finite(in.line6, 6 * in.n_ln) ||
      !all_finite(in.l2d4, 4 * ML) || !all_finite(in.l3d6, 6 * ML)) {
    msg = "non-finite coordinate";
    return 1;
  }
  if (in.n_pt + in.n_ln > (long long)(1 << 28) || MP + ML > (long long)(1 << 28)) { msg = "too many tracks or observations for one call"; return 1; }
  pl.alpha = cfg.geometric_alpha;
  pl.max_iter = cfg.max_num_iterations;
  pl.num_outliers = cfg.num_outliers_aggregator;
  pl.poll = cfg.poll_interval > 0 ? cfg.poll_interval : kBaPollDefault;
  pl.kernel_timers = cfg.kernel_timers;
  pl.NP = (int)in.n_pt;
  pl.NS = (int)(in.n_pt + in.n_ln);
  pl.st.resize((size_t)pl.NS);
  pl.sp0.assign(6 * (size_t)pl.NS, 0.0);
  pl.l3d.assign(in.l3d6, in.l3d6 + 6 * (size_t)ML);
  pl.ln_off.assign(in.ln_off ? in.ln_off : nullptr, in.ln_off ? in.ln_off + in.n_ln + 1 : nullptr);
  // blocks with the input row of their image; the rows of the active images follow below
  // AddPointGeometricResiduals returns at once without a weight; R1.1 is skipped when point, intrinsics and pose are all constant
  const bool add_points = cfg.lw_point > 0.0 && !(pl.constant_pose && cfg.constant_point != 0);
  for (int64_t n = 0; n < in.n_pt; ++n) {
    BaStruct &s = pl.st[(size_t)n];
    s = BaStruct{(int)pl.blk.size(), 0, 0, 0, 0, 0, {0, 0}};
    for (int c = 0; c < 3; ++c) pl.sp0[6 * (size_t)n + c] = in.pt3[3 * n + c];
    if (add_points && ingest_point_track(n, (int)n, in.pt_off, in.pt_img, in.pt_xy, cfg.lw_point, id2row, pl.blk, msg)) return 1;
    s.nb = (int)pl.blk.size() - s.b0;
    s.constant = (cfg.constant_point != 0 || s.nb == 0) ? 1 : 0;  // without a block the point is no parameter of the problem
  }
  SupportOrder so;
  for (int64_t n = 0; n < in.n_ln; ++n) {
    const int si = pl.NP + (int)n;
    BaStruct &s = pl.st[(size_t)si];
    s = BaStruct{(int)pl.blk.size(), 0, 0, 0, 1, 0, {0, 0}};
    if (ingest_line_length("line track", n, in.line6 + 6 * n, msg)) return 1;
    rf_minimal(in.line6 + 6 * n, pl.sp0.data() + 6 * (size_t)si);
    const long long a = in.ln_off[n];
    const int K = (int)(in.ln_off[n + 1] - a);
    if (K <= 0) { msg = "line track " + std::to_string(n) + " has no supports"; return 1; }  // THROW_CHECK_GT(line3ds.size(), 0)
    int n_images;
    if (ingest_outliers("line track", n, cfg.num_outliers_aggregator, K, msg) ||
        ingest_supports("line track", n, in.ln_img + a, K, id2row, so, &n_images, msg,
                        [&](int, int x, int row) { pl.blk.push_back(line_blk(in.l2d4 + 4 * (a + x), row, si)); }))
      return 1;
    s.nb = K;
    s.constant = (cfg.constant_line != 0 || n_images < cfg.min_num_images) ? 1 : 0;
  }
  pl.NB = (int)pl.blk.size();
  // the images that carry a residual block, in ascending id: only they are parameters of the problem
  std::vector<char> used((size_t)std::max(in.n_img, 1), 0);
  for (const BaBlk &b : pl.blk) used[(size_t)b.cam] = 1;
  std::vector<int> rows;
  for (int n = 0; n < in.n_img; ++n)
    if (used[(size_t)n]) rows.push_back(n);
  std::sort(rows.begin(), rows.end(), [&](int x, int y) { return in.img_ids[x] < in.img_ids[y]; });
  if (!pl.constant_pose && (int)rows.size() > kBaMaxImages) {
    msg = std::to_string(rows.size()) + " images carry residuals, more than LT_BA_MAX_IMAGES = " + std::to_string(kBaMaxImages) +
          " (a preconditioned-CG path for larger collections is not built)";
    return 1;
  }
  pl.C = (int)rows.size();
  pl.cam_row = rows;
  std::vector<int> row2cam((size_t)std::max(in.n_img, 1), -1);
  pl.kvec.resize(4 * (size_t)pl.C);
  pl.pose0.resize(7 * (size_t)pl.C);
  for (int c = 0; c < pl.C; ++c) {
    const int r = rows[(size_t)c];
    row2cam[(size_t)r] = c;
    if (ingest_cam_row(in.img_ids, in.k, in.q, in.t, r, true, pl.kvec.data() + 4 * (size_t)c, pl.pose0.data() + 7 * (size_t)c, msg))
      return 1;
  }
  for (BaBlk &b : pl.blk) b.cam = row2cam[(size_t)b.cam];
  // the (track, image) pairs of every structure in ascending image order, and the blocks of each pair in residual order
  pl.pair_blk_off.push_back(0);
  std::vector<int> cams;
  for (int s = 0; s < pl.NS; ++s) {
    BaStruct &st = pl.st[(size_t)s];
    cams.clear();
    for (int i = 0; i < st.nb; ++i) cams.push_back(pl.blk[(size_t)(st.b0 + i)].cam);
    std::sort(cams.begin(), cams.end());
    cams.erase(std::unique(cams.begin(), cams.end()), cams.end());
    st.p0 = (int)pl.pair_cam.size();
    st.np = (int)cams.size();
    for (int c : cams) {
      const int p = (int)pl.pair_cam.size();
      pl.pair_cam.push_back(c);
      pl.pair_s.push_back(s);
      for (int i = 0; i < st.nb; ++i)
        if (pl.blk[(size_t)(st.b0 + i)].cam == c) {
          pl.blk[(size_t)(st.b0 + i)].pair = p;
          pl.pair_blk.push_back(st.b0 + i);
        }
      pl.pair_blk_off.push_back((int)pl.pair_blk.size());
    }
  }
  pl.NPair = (int)pl.pair_cam.size();
  // per image its blocks in ascending order
  pl.cam_blk_off.assign((size_t)pl.C + 1, 0);
  for (const BaBlk &b : pl.blk) pl.cam_blk_off[(size_t)b.cam + 1] += 1;
  for (int c = 0; c < pl.C; ++c) pl.cam_blk_off[(size_t)c + 1] += pl.cam_blk_off[(size_t)c];
  pl.cam_blk.resize((size_t)pl.NB);
  std::vector<int> fb(pl.cam_blk_off.begin(), pl.cam_blk_off.end() - 1);
  for (int b = 0; b < pl.NB; ++b) pl.cam_blk[(size_t)fb[(size_t)pl.blk[(size_t)b].cam]++] = b;
  // per image pair (i, j <= i) the couples (p, q) of pairs of the free structures that see both, in ascending structure
  // order: the terms of S_ij
  if (pl.constant_pose) return 0;  // no Schur complement: the poses are no unknowns
  const size_t n_ij = (size_t)pl.C * ((size_t)pl.C + 1) / 2;
  std::vector<long long> cnt(n_ij + 1, 0);
  for (int pass = 0; pass < 2; ++pass) {
    for (int s = 0; s < pl.NS; ++s) {
      const BaStruct &st = pl.st[(size_t)s];
      if (st.constant) continue;
      for (int p = st.p0; p < st.p0 + st.np; ++p)
        for (int q = st.p0; q <= p; ++q) {  // the pairs of a structure ascend in image order
          const size_t ij = (size_t)pl.pair_cam[(size_t)p] * ((size_t)pl.pair_cam[(size_t)p] + 1) / 2 + (size_t)pl.pair_cam[(size_t)q];
          if (pass == 0) {
            cnt[ij + 1] += 1;
          } else {
            const long long at = cnt[ij]++;
            pl.sch[2 * (size_t)at] = p;
            pl.sch[2 * (size_t)at + 1] = q;
          }
        }
    }
    if (pass == 0) {
      for (size_t x = 0; x < n_ij; ++x) cnt[x + 1] += cnt[x];
      if (cnt[n_ij] > (long long)(1 << 29)) { msg = "too many (track, image, image) terms for one call"; return 1; }
      pl.sch_off.assign(cnt.begin(), cnt.end());
      pl.sch.assign(2 * (size_t)cnt[n_ij], 0);
    }
  }
  return 0;
}

// what a solve leaves
struct Result {
  std::vector<double> pose, sp;  // the current set: 7 C, 6 NS
  BaStatus status;
};

// the work tables of a solve on the host
struct HostTables {
  std::vector<double> pose, sp, lin, V, bs, W, U, g, Vinv, Y, S, LT, rhs, dc, ds, chunk;
  BaStatus status;
  BaDev dev;
};

void bind_plan(const Plan &pl, BaDev &d) {
  d.C = pl.C; d.NS = pl.NS; d.NB = pl.NB; d.NPair = pl.NPair;
  d.n = 6 * pl.C;
  d.n_chunks = lm_chunks_of(pl.NB);
  d.alpha = pl.alpha;
}

void host_tables(const Plan &pl, HostTables &h) {
  BaDev &d = h.dev;
  bind_plan(pl, d);
  const size_t n = (size_t)d.n;
  h.pose.assign(2 * 7 * (size_t)pl.C, 0.0);
  std::copy(pl.pose0.begin(), pl.pose0.end(), h.pose.begin());
  h.sp.assign(2 * 6 * (size_t)pl.NS, 0.0);
  std::copy(pl.sp0.begin(), pl.sp0.end(), h.sp.begin());
  h.lin.assign((size_t)kBaLinFields * std::max(pl.NB, 1), 0.0);
  h.V.assign(10 * (size_t)std::max(pl.NS, 1), 0.0);
  h.bs.assign(4 * (size_t)std::max(pl.NS, 1), 0.0);
  h.W.assign(24 * (size_t)std::max(pl.NPair, 1), 0.0);
  h.U.assign(21 * (size_t)std::max(pl.C, 1), 0.0);
  h.g.assign(6 * (size_t)std::max(pl.C, 1), 0.0);
  h.Vinv.assign(16 * (size_t)std::max(pl.NS, 1), 0.0);
  h.Y.assign(24 * (size_t)std::max(pl.NPair, 1), 0.0);
  h.S.assign(std::max<size_t>(n * n, 1), 0.0);
  h.LT.assign(std::max<size_t>(n * n, 1), 0.0);
  h.rhs.assign(std::max<size_t>(n, 1), 0.0);
  h.dc.assign(std::max<size_t>(n, 1), 0.0);
  h.ds.assign(4 * (size_t)std::max(pl.NS, 1), 0.0);
  h.chunk.assign(2 * (size_t)d.n_chunks, 0.0);
  d.kvec = pl.kvec.data(); d.pose = h.pose.data(); d.sp = h.sp.data();
  d.st = pl.st.data(); d.blk = pl.blk.data();
  d.pair_cam = pl.pair_cam.data(); d.pair_s = pl.pair_s.data();
  d.pair_blk_off = pl.pair_blk_off.data(); d.pair_blk = pl.pair_blk.data();
  d.cam_blk_off = pl.cam_blk_off.data(); d.cam_blk = pl.cam_blk.data();
  d.sch_off = pl.sch_off.data(); d.sch = pl.sch.data();
  d.lin = h.lin.data(); d.V = h.V.data(); d.bs = h.bs.data(); d.W = h.W.data(); d.U = h.U.data(); d.g = h.g.data();
  d.Vinv = h.Vinv.data(); d.Y = h.Y.data(); d.S = h.S.data(); d.LT = h.LT.data(); d.rhs = h.rhs.data(); d.dc = h.dc.data();
  d.ds = h.ds.data(); d.chunk = h.chunk.data();
  d.status = &h.status;
  h.status = BaStatus{};
  h.status.max_iter = pl.max_iter;
}

// ---- the host twins of the kernels ----
// k_ba_cost; k_ba_decide's reduction of the chunks
void host_cost(const BaDev &d, int set, bool with_md, int nt) {
  lm_chunks_host(d.chunk, d.NB, d.n_chunks, d.n_chunks, nt, [&](int i, double *a, double *b) {
    double c, m;
    ba_item_cost(d, set, i, with_md, &c, &m);
    *a = *a + c;
    *b = *b + m;
  });
}
void host_totals(const BaDev &d, double *cost, double *md) { lm_totals_host(d.chunk, d.n_chunks, d.n_chunks, cost, md); }
// k_ba_linearize, k_ba_blocks, k_ba_images
void host_linearise(const BaDev &d, int cur, int nt) {
#pragma omp parallel for num_threads(nt) schedule(static)
  for (int b = 0; b < d.NB; ++b) ba_item_linearise(d, cur, b);
#pragma omp parallel for num_threads(nt) schedule(static)
  for (int s = 0; s < d.NS; ++s) {
    const BaStruct st = d.st[s];
    if (st.constant) continue;
    double part[kBaWidth][kRfSums], out[kRfSums];
    for (int l = 0; l < kBaWidth; ++l) ba_struct_part(d, st, l, part[l]);
    lm_tree_host(part, kRfSums, out);
    for (int c = 0; c < 10; ++c) d.V[(size_t)10 * s + c] = out[c];
    for (int c = 0; c < 4; ++c) d.bs[(size_t)4 * s + c] = out[10 + c];
    for (int q = st.p0; q < st.p0 + st.np; ++q) ba_pair_W(d, q);
  }
#pragma omp parallel for num_threads(nt) schedule(static)
  for (int c = 0; c < d.C; ++c) {
    double part[kLcWidth][kLcSums], out[kLcSums];
    for (int l = 0; l < kBaWave; ++l) ba_cam_part(d, c, l, part[l]);
    lm_tree_host(part, kLcSums, out);
    for (int x = 0; x < 21; ++x) d.U[(size_t)21 * c + x] = out[x];
    for (int x = 0; x < 6; ++x) d.g[(size_t)6 * c + x] = out[21 + x];
  }
}
// k_ba_schur: the image pairs of row i
void host_schur_row(const BaDev &d, int i, double mu) {
  for (int j = 0; j <= i; ++j)
    for (int e = 0; e < 42; ++e) ba_item_schur(d, i, j, e, mu);
}

void host_init(const BaDev &d, int nt, double *total0 = nullptr) {
  host_cost(d, 0, false, nt);
  double cost, md;
  host_totals(d, &cost, &md);
  if (total0) *total0 = cost;
  ba_decide_init(*d.status, cost);
}

// one attempt: launch_ba_attempt on the host.  rec (tests): what the attempt hands to ba_decide_step -- the radius and
// the fresh flag it ran with, whether a factorisation failed, the two totals; rec[1] = -1: it ended by the zero gradient
void host_attempt(const BaDev &d, int nt, double *rec = nullptr) {
  BaStatus &st = *d.status;
  if (st.done) return;
  if (rec) { rec[0] = st.mu; rec[1] = 0.0; rec[2] = st.fresh; rec[3] = rec[4] = 0.0; }
  if (st.fresh) host_linearise(d, st.cur, nt);
  {
    int bad = 0;
#pragma omp parallel for num_threads(nt) schedule(static) reduction(| : bad)
    for (int s = 0; s < d.NS; ++s) bad |= ba_item_vinv(d, s, st.mu) ? 0 : 1;
    if (bad) st.bad = 1;
  }
  if (!st.bad) {
#pragma omp parallel for num_threads(nt) schedule(dynamic, 1)
    for (int i = 0; i < d.C; ++i) host_schur_row(d, i, st.mu);
    if (st.fresh) {  // k_ba_chol's first step
      bool nz = false;
      for (int i = 0; i < d.n; ++i) nz = nz || d.g[i] != 0.0;
      for (int s = 0; s < d.NS; ++s) {
        if (d.st[s].constant) continue;
        for (int l = 0; l < (d.st[s].kind ? 4 : 3); ++l) nz = nz || d.bs[(size_t)4 * s + l] != 0.0;
      }
      if (!nz) {
        st.code = kRfZeroGrad; st.done = 1;
        if (rec) rec[1] = -1.0;
        return;
      }
    }
    if (!ba_cholesky_host(d.n, d.S, d.rhs, d.LT, d.dc)) st.bad = 1;
  }
  if (!st.bad) {
#pragma omp parallel for num_threads(nt) schedule(static)
    for (int e = 0; e < d.NS + d.C; ++e) {
      if (e < d.NS) ba_item_backsub_struct(d, st.cur, e);
      else ba_item_backsub_cam(d, st.cur, e - d.NS);
    }
    host_cost(d, 1 - st.cur, true, nt);
  }
  double cost, md;
  host_totals(d, &cost, &md);
  if (rec) { rec[1] = st.bad; rec[3] = cost; rec[4] = md; }
  ba_decide_step(st, cost, md);
}

void run_host(const Plan &pl, int n_threads, Result &res) {
  const int nt = n_threads > 0 ? n_threads : omp_get_max_threads();
  HostTables h;
  host_tables(pl, h);
  host_init(h.dev, nt);
  while (!h.status.done) host_attempt(h.dev, nt);
  const int cur = h.status.cur;
  res.pose.assign(h.pose.begin() + (size_t)cur * 7 * pl.C, h.pose.begin() + (size_t)(cur + 1) * 7 * pl.C);
  res.sp.assign(h.sp.begin() + (size_t)cur * 6 * pl.NS, h.sp.begin() + (size_t)(cur + 1) * 6 * pl.NS);
  res.status = h.status;
}

// ---- constant poses: every point track its own problem (k_ba_point_lm) ----
void bind_points(const Plan &pl, BaDev &d) {
  d = BaDev{};
  bind_plan(pl, d);
}

void run_points_host(const Plan &pl, int n_threads, std::vector<BaPtOut> &out) {
  const int nt = n_threads > 0 ? n_threads : omp_get_max_threads();
  BaDev d;
  bind_points(pl, d);
  std::vector<double> pose = pl.pose0, sp = pl.sp0;
  d.kvec = pl.kvec.data(); d.pose = pose.data(); d.sp = sp.data();
  d.st = pl.st.data(); d.blk = pl.blk.data();
  out.assign((size_t)pl.NS, BaPtOut{});
#pragma omp parallel for num_threads(nt) schedule(dynamic, 16)
  for (int s = 0; s < pl.NS; ++s) {
    BaPtOut &o = out[(size_t)s];
    for (int c = 0; c < 3; ++c) o.p[c] = pl.sp0[6 * (size_t)s + c];
    BaPointGroup<LmHostLanes<kBaWidth>> grp{{}, d, pl.st[(size_t)s]};
    ba_point_lm(grp, pl.st[(size_t)s].constant != 0, pl.max_iter, o.p, &o.cost0, &o.cost1, &o.iters, &o.code);
  }
}

// the separated solve as one result: the points; the costs summed over the tracks in ascending order, the largest
// iteration count, and the largest termination code of the free tracks (5 where every track is constant)
void points_result(const Plan &pl, const std::vector<BaPtOut> &out, Result &res) {
  res.pose = pl.pose0;
  res.sp = pl.sp0;
  res.status = BaStatus{};
  res.status.done = 1;
  int code = -1;
  for (int s = 0; s < pl.NS; ++s) {
    const BaPtOut &o = out[(size_t)s];
    for (int c = 0; c < 3; ++c) res.sp[6 * (size_t)s + c] = o.p[c];
    res.status.F0 = res.status.F0 + o.cost0;
    res.status.F = res.status.F + o.cost1;
    res.status.iters = std::max(res.status.iters, o.iters);
    if (o.code != kRfConstant) code = std::max(code, o.code);
  }
  res.status.code = code < 0 ? (int)kRfConstant : code;
}

// a problem without residual blocks: Solve() returns false upstream, nothing changes
void no_residuals(const Plan &pl, Result &res) {
  res.pose = pl.pose0;
  res.sp = pl.sp0;
  res.status = BaStatus{};
  res.status.done = 1;
  res.status.code = kLcNoResiduals;
}

// GetLineSegmentFromInfiniteLine3d on the solved parameters: §19's cut (the rank rule of k_refine_cut), on the host in
// both paths
void cut_line(const double p[6], const double *l3, long long K, int num_outliers, double seg[6]) {
  d3 dir, m;
  rf_infinite(p, &dir, &m);
  const d3 pref = rf_pref(dir, m, mk3(l3[0], l3[1], l3[2]));
  const long long n = 2 * K, lo = num_outliers, hi = n - 1 - num_outliers;
  for (int c = 0; c < 6; ++c) seg[c] = std::nan("");
  for (long long i = 0; i < n; ++i) {
    double v;
    bool is_lo, is_hi;
    rf_rank_test(l3, n, i, pref, dir, lo, hi, &v, &is_lo, &is_hi);
    if (is_lo) { seg[0] = pref.x + dir.x * v; seg[1] = pref.y + dir.y * v; seg[2] = pref.z + dir.z * v; }
    if (is_hi) { seg[3] = pref.x + dir.x * v; seg[4] = pref.y + dir.y * v; seg[5] = pref.z + dir.z * v; }
  }
}

// the outputs of lt_ba_get.  An image without a residual block keeps its input pose bit for bit
struct Outputs {
  std::vector<double> q, t, pts, params, segs;
  double cost[2];
  int iters, code;
};
void gather(const Input &in, const Plan &pl, const Result &res, Outputs &o) {
  o.q.assign(in.q, in.q + 4 * (size_t)in.n_img);
  o.t.assign(in.t, in.t + 3 * (size_t)in.n_img);
  for (int c = 0; c < (pl.constant_pose ? 0 : pl.C); ++c) {  // constant poses keep their input bit for bit
    const int r = pl.cam_row[(size_t)c];
    for (int x = 0; x < 4; ++x) o.q[4 * (size_t)r + x] = res.pose[7 * (size_t)c + x];
    for (int x = 0; x < 3; ++x) o.t[3 * (size_t)r + x] = res.pose[7 * (size_t)c + 4 + x];
  }
  o.pts.resize(3 * (size_t)pl.NP);
  for (int n = 0; n < pl.NP; ++n)
    for (int x = 0; x < 3; ++x) o.pts[3 * (size_t)n + x] = res.sp[6 * (size_t)n + x];
  const int NL = pl.NS - pl.NP;
  o.params.resize(6 * (size_t)NL);
  o.segs.resize(6 * (size_t)NL);
  for (int n = 0; n < NL; ++n) {
    const double *p = res.sp.data() + 6 * (size_t)(pl.NP + n);
    std::copy(p, p + 6, o.params.begin() + 6 * (size_t)n);
    const long long a = pl.ln_off[(size_t)n], K = pl.ln_off[(size_t)n + 1] - a;
    cut_line(p, pl.l3d.data() + 6 * a, K, pl.num_outliers, o.segs.data() + 6 * (size_t)n);
  }
  o.cost[0] = res.status.F0;
  o.cost[1] = res.status.F;
  o.iters = res.status.iters;
  o.code = res.status.code;
}
void copy_out(const Outputs &o, double *qvec4, double *tvec3, double *pt3, double *params6, double *seg6, double *cost2,
              int32_t *iters, int32_t *code) {
  if (qvec4) std::copy(o.q.begin(), o.q.end(), qvec4);
  if (tvec3) std::copy(o.t.begin(), o.t.end(), tvec3);
  if (pt3) std::copy(o.pts.begin(), o.pts.end(), pt3);
  if (params6) std::copy(o.params.begin(), o.params.end(), params6);
  if (seg6) std::copy(o.segs.begin(), o.segs.end(), seg6);
  if (cost2) { cost2[0] = o.cost[0]; cost2[1] = o.cost[1]; }
  if (iters) *iters = o.iters;
  if (code) *code = o.code;
}

static thread_local HostError g_host_error;

#ifndef LT_HOST_ONLY  // (tools/ba_host_asan.cpp compiles the host twin alone: no context, no HIP runtime)
int run_device(lt_ctx *ctx, const Plan &pl, Result &res, double timers[16]) {
  lt_host::BaState &ba = ctx->ba;
  const double t0 = now_ms();
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  BaDev d;
  bind_plan(pl, d);
  const size_t n = (size_t)d.n, C = (size_t)pl.C, NS = (size_t)pl.NS, NB = (size_t)std::max(pl.NB, 1), NPair = (size_t)std::max(pl.NPair, 1);
  // the two parameter sets: set 0 holds the initial point
  std::vector<double> pose(2 * 7 * C, 0.0), sp(2 * 6 * NS, 0.0);
  std::copy(pl.pose0.begin(), pl.pose0.end(), pose.begin());
  std::copy(pl.sp0.begin(), pl.sp0.end(), sp.begin());
  // one index buffer: pair_cam, pair_s, pair_blk_off, pair_blk, cam_blk_off, cam_blk, sch_off, sch
  std::vector<int> idx;
  size_t o_idx[8];
  const std::vector<int> *parts[8] = {&pl.pair_cam, &pl.pair_s, &pl.pair_blk_off, &pl.pair_blk, &pl.cam_blk_off, &pl.cam_blk,
                                      &pl.sch_off, &pl.sch};
  for (int k = 0; k < 8; ++k) {
    o_idx[k] = idx.size();
    idx.insert(idx.end(), parts[k]->begin(), parts[k]->end());
  }
  if (int rc = upload_vec(ctx, ba.d_k, pl.kvec)) return rc;
  if (int rc = upload_vec(ctx, ba.d_pose, pose)) return rc;
  if (int rc = upload_vec(ctx, ba.d_sp, sp)) return rc;
  if (int rc = upload_vec(ctx, ba.d_st, pl.st)) return rc;
  if (int rc = upload_vec(ctx, ba.d_blk, pl.blk)) return rc;
  if (int rc = upload_vec(ctx, ba.d_idx, idx)) return rc;
  // V 10 NS | bs 4 NS | W 24 NPair | U 21 C | g 6 C | Vinv 16 NS | Y 24 NPair
  const size_t o_V = 0, o_bs = o_V + 10 * NS, o_W = o_bs + 4 * NS, o_U = o_W + 24 * NPair, o_g = o_U + 21 * C,
               o_Vinv = o_g + 6 * C, o_Y = o_Vinv + 16 * NS, n_sums = o_Y + 24 * NPair;
  ENSURE(ctx, ba.d_lin, 8 * (size_t)kBaLinFields * NB);
  ENSURE(ctx, ba.d_sums, 8 * std::max<size_t>(n_sums, 1));
  ENSURE(ctx, ba.d_S, 8 * std::max<size_t>(n * n, 1));
  ENSURE(ctx, ba.d_LT, 8 * std::max<size_t>(n * n, 1));
  ENSURE(ctx, ba.d_vec, 8 * std::max<size_t>(2 * n + 4 * NS, 1));  // rhs n | dc n | ds 4 NS
  ENSURE(ctx, ba.d_chunk, 8 * 2 * (size_t)d.n_chunks);
  ENSURE(ctx, ba.d_status, sizeof(BaStatus));
  BaStatus init = BaStatus{};
  init.max_iter = pl.max_iter;
  HIPCHK(ctx, hipMemcpyAsync(ba.d_status.p, &init, sizeof(BaStatus), hipMemcpyHostToDevice, st));
  d.kvec = ba.d_k.as<double>(); d.pose = ba.d_pose.as<double>(); d.sp = ba.d_sp.as<double>();
  d.st = ba.d_st.as<BaStruct>(); d.blk = ba.d_blk.as<BaBlk>();
  const int *ib = ba.d_idx.as<int>();
  d.pair_cam = ib + o_idx[0]; d.pair_s = ib + o_idx[1]; d.pair_blk_off = ib + o_idx[2]; d.pair_blk = ib + o_idx[3];
  d.cam_blk_off = ib + o_idx[4]; d.cam_blk = ib + o_idx[5]; d.sch_off = ib + o_idx[6]; d.sch = ib + o_idx[7];
  d.lin = ba.d_lin.as<double>();
  double *sums = ba.d_sums.as<double>();
  d.V = sums + o_V; d.bs = sums + o_bs; d.W = sums + o_W; d.U = sums + o_U; d.g = sums + o_g; d.Vinv = sums + o_Vinv; d.Y = sums + o_Y;
  d.S = ba.d_S.as<double>(); d.LT = ba.d_LT.as<double>();
  d.rhs = ba.d_vec.as<double>(); d.dc = d.rhs + n; d.ds = d.dc + n;
  d.chunk = ba.d_chunk.as<double>();
  d.status = ba.d_status.as<BaStatus>();
  if (int rc = stream_sync(ctx)) return rc;
  const double t1 = now_ms();
  timers[0] = t1 - t0;
  // the loop: its decisions are made on the device; `poll` attempts are enqueued back to back, then the status record
  // (64 bytes) comes back.  Attempts enqueued past the end of the solve return at once, so the result does not depend
  // on the interval
  Events<10> ev;
  if (pl.kernel_timers)
    if (int rc = ev.create(ctx)) return rc;
  launch_ba_init(st, d);
  BaStatus status = BaStatus{};
  long long launched = 0;
  if (int rc = run_polled(
          ctx, pl.kernel_timers ? 1 : pl.poll, ba.d_status.p, status,
          [&]() {
            launch_ba_attempt(st, d, pl.kernel_timers ? ev.data() : nullptr);
            if (pl.kernel_timers) ev.mark_all();
          },
          [](const BaStatus &s) { return s.done != 0; },
          [&]() {
            if (pl.kernel_timers)
              for (int x = 0; x < 9; ++x) timers[4 + x] += ev.ms(x, x + 1);
          },
          &launched))
    return rc;
  const double t2 = now_ms();
  timers[1] = t2 - t1;
  timers[3] = (double)launched;
  const int cur = status.cur;
  if (int rc = download(ctx, res.pose, ba.d_pose.as<double>() + (size_t)cur * 7 * C, 7 * C)) return rc;
  if (int rc = download(ctx, res.sp, ba.d_sp.as<double>() + (size_t)cur * 6 * NS, 6 * NS)) return rc;
  if (int rc = stream_sync(ctx)) return rc;
  res.status = status;
  timers[2] = now_ms() - t2;
  return LT_OK;
}

int run_points_device(lt_ctx *ctx, const Plan &pl, std::vector<BaPtOut> &out, double timers[16]) {
  lt_host::BaState &ba = ctx->ba;
  const double t0 = now_ms();
  HIPCHK(ctx, hipSetDevice(ctx->device));
  BaDev d;
  bind_points(pl, d);
  if (int rc = upload_vec(ctx, ba.d_k, pl.kvec)) return rc;
  if (int rc = upload_vec(ctx, ba.d_pose, pl.pose0)) return rc;
  if (int rc = upload_vec(ctx, ba.d_sp, pl.sp0)) return rc;
  if (int rc = upload_vec(ctx, ba.d_st, pl.st)) return rc;
  if (int rc = upload_vec(ctx, ba.d_blk, pl.blk)) return rc;
  ENSURE(ctx, ba.d_vec, sizeof(BaPtOut) * (size_t)std::max(pl.NS, 1));
  d.kvec = ba.d_k.as<double>(); d.pose = ba.d_pose.as<double>(); d.sp = ba.d_sp.as<double>();
  d.st = ba.d_st.as<BaStruct>(); d.blk = ba.d_blk.as<BaBlk>();
  if (int rc = stream_sync(ctx)) return rc;
  const double t1 = now_ms();
  timers[0] = t1 - t0;
  launch_ba_points(ctx->stream, d, pl.max_iter, ba.d_vec.as<BaPtOut>());
  if (int rc = stream_sync(ctx)) return rc;
  const double t2 = now_ms();
  timers[1] = t2 - t1;
  if (int rc = download(ctx, out, ba.d_vec.p, (size_t)pl.NS)) return rc;
  if (int rc = stream_sync(ctx)) return rc;
  timers[2] = now_ms() - t2;
  return LT_OK;
}
#endif  // LT_HOST_ONLY

Input make_input(int n_img, const int32_t *img_ids, const double *kvec4, const double *qvec4, const double *tvec3,
                 int64_t n_pt, const double *pt3, const int64_t *pt_off, const int32_t *pt_img, const double *pt_xy2,
                 int64_t n_ln, const double *line6, const int64_t *ln_off, const int32_t *ln_img, const double *l2d4,
                 const double *l3d6, const lt_ba_config *cfg) {
  return Input{n_img, img_ids, kvec4, qvec4, tvec3, n_pt, pt3, pt_off, pt_img, pt_xy2, n_ln, line6, ln_off, ln_img, l2d4, l3d6, cfg};
}

}  // namespace

extern "C" {

void lt_ba_config_default(lt_ba_config *cfg) {
  if (!cfg) return;
  cfg->geometric_alpha = 10.0;  // hybrid_bundle_adjustment_config.h:17-49 except constant_intrinsics, which is 0 there
  cfg->lw_point = 0.1;
  cfg->min_num_images = 4;
  cfg->num_outliers_aggregator = 2;
  cfg->max_num_iterations = 100;
  cfg->constant_intrinsics = 1;
  cfg->constant_principal_point = 1;
  cfg->constant_pose = 0;
  cfg->constant_point = 0;
  cfg->constant_line = 0;
  cfg->poll_interval = 0;
  cfg->kernel_timers = 0;
}

int lt_ba_max_images(void) { return kBaMaxImages; }
int lt_ba_poll_default(void) { return kBaPollDefault; }

#ifndef LT_HOST_ONLY
int lt_ba_arrays(lt_ctx *ctx, int n_img, const int32_t *img_ids, const double *kvec4, const double *qvec4,
                 const double *tvec3, int64_t n_pt, const double *pt3, const int64_t *pt_off, const int32_t *pt_img,
                 const double *pt_xy2, int64_t n_ln, const double *line6, const int64_t *ln_off, const int32_t *ln_img,
                 const double *l2d4, const double *l3d6, const lt_ba_config *cfg) {
  if (!ctx) return LT_ERR_ARGUMENT;
  const Input in = make_input(n_img, img_ids, kvec4, qvec4, tvec3, n_pt, pt3, pt_off, pt_img, pt_xy2, n_ln, line6, ln_off,
                              ln_img, l2d4, l3d6, cfg);
  std::string msg;
  Plan pl;
  if (make_plan(in, pl, msg)) return fail(ctx, LT_ERR_ARGUMENT, "lt_ba_arrays: " + msg);
  lt_host::BaState &ba = ctx->ba;
  for (double &x : ba.timers) x = 0.0;
  Result res;
  if (pl.NB == 0) {
    no_residuals(pl, res);
  } else if (pl.constant_pose) {
    std::vector<BaPtOut> out;
    if (int rc = run_points_device(ctx, pl, out, ba.timers)) return rc;
    points_result(pl, out, res);
  } else if (int rc = run_device(ctx, pl, res, ba.timers)) {
    return rc;
  }
  Outputs o;
  gather(in, pl, res, o);
  ba.q = o.q; ba.t = o.t; ba.pts = o.pts; ba.params = o.params; ba.segs = o.segs;
  ba.cost[0] = o.cost[0]; ba.cost[1] = o.cost[1];
  ba.iters = o.iters; ba.code = o.code;
  return LT_OK;
}

int lt_ba_get(lt_ctx *ctx, double *qvec4, double *tvec3, double *pt3, double *params6, double *seg6, double *cost2,
              int32_t *iters, int32_t *code) {
  if (!ctx) return LT_ERR_ARGUMENT;
  const lt_host::BaState &ba = ctx->ba;
  Outputs o{ba.q, ba.t, ba.pts, ba.params, ba.segs, {ba.cost[0], ba.cost[1]}, ba.iters, ba.code};
  copy_out(o, qvec4, tvec3, pt3, params6, seg6, cost2, iters, code);
  return LT_OK;
}

int lt_ba_get_timers(lt_ctx *ctx, double out[16]) {
  if (!ctx || !out) return LT_ERR_ARGUMENT;
  for (int k = 0; k < 16; ++k) out[k] = ctx->ba.timers[k];
  return LT_OK;
}
#endif  // LT_HOST_ONLY

const char *lt_fn_ba_host_error(void) { return g_host_error.c_str(); }

int lt_fn_ba_host(int n_img, const int32_t *img_ids, const double *kvec4, const double *qvec4, const double *tvec3,
                  int64_t n_pt, const double *pt3, const int64_t *pt_off, const int32_t *pt_img, const double *pt_xy2,
                  int64_t n_ln, const double *line6, const int64_t *ln_off, const int32_t *ln_img, const double *l2d4,
                  const double *l3d6, const lt_ba_config *cfg, int n_threads, double *qvec4_out, double *tvec3_out,
                  double *pt3_out, double *params6, double *seg6, double *cost2, int32_t *iters, int32_t *code) {
  const Input in = make_input(n_img, img_ids, kvec4, qvec4, tvec3, n_pt, pt3, pt_off, pt_img, pt_xy2, n_ln, line6, ln_off,
                              ln_img, l2d4, l3d6, cfg);
  std::string msg;
  Plan pl;
  if (int rc = g_host_error.check("lt_fn_ba_host", make_plan(in, pl, msg), msg)) return rc;
  Result res;
  if (pl.NB == 0) {
    no_residuals(pl, res);
  } else if (pl.constant_pose) {
    std::vector<BaPtOut> out;
    run_points_host(pl, n_threads, out);
    points_result(pl, out, res);
  } else {
    run_host(pl, n_threads, res);
  }
  Outputs o;
  gather(in, pl, res, o);
  copy_out(o, qvec4_out, tvec3_out, pt3_out, params6, seg6, cost2, iters, code);
  return LT_OK;
}

int lt_fn_ba_eval(int n_img, const int32_t *img_ids, const double *kvec4, const double *qvec4, const double *tvec3,
                  int64_t n_pt, const double *pt3, const int64_t *pt_off, const int32_t *pt_img, const double *pt_xy2,
                  int64_t n_ln, const double *line6, const int64_t *ln_off, const int32_t *ln_img, const double *l2d4,
                  const double *l3d6, const lt_ba_config *cfg, const double *params6_in, int64_t *dims4, int32_t *blk_info3,
                  double *residuals, double *cost, double *g, double *H, double mu, double *step) {
  const Input in = make_input(n_img, img_ids, kvec4, qvec4, tvec3, n_pt, pt3, pt_off, pt_img, pt_xy2, n_ln, line6, ln_off,
                              ln_img, l2d4, l3d6, cfg);
  std::string msg;
  Plan pl;
  if (int rc = g_host_error.check("lt_fn_ba_eval", make_plan(in, pl, msg), msg)) return rc;
  if (pl.constant_pose) return g_host_error.refuse("lt_fn_ba_eval", "constant_pose=1 has no joint system");
  const int NL = pl.NS - pl.NP;
  if (params6_in)  // the lines' minimal parameters as given (the edge fixtures), not those of their segments
    std::copy(params6_in, params6_in + 6 * (size_t)NL, pl.sp0.begin() + 6 * (size_t)pl.NP);
  // the unknowns: images (6 each), then the free structures in order (3 / 4 each)
  std::vector<int> so((size_t)pl.NS, -1);
  int nu = 6 * pl.C;
  for (int s = 0; s < pl.NS; ++s)
    if (!pl.st[(size_t)s].constant) { so[(size_t)s] = nu; nu += pl.st[(size_t)s].kind ? 4 : 3; }
  if (dims4) { dims4[0] = pl.C; dims4[1] = pl.NB; dims4[2] = nu; dims4[3] = pl.NS; }
  if (!residuals && !cost && !g && !H && !step && !blk_info3) return LT_OK;
  if (pl.NB == 0) return g_host_error.refuse("lt_fn_ba_eval", "no residual blocks");
  HostTables h;
  host_tables(pl, h);
  const BaDev &d = h.dev;
  host_init(d, 1);
  if (cost) *cost = h.status.F;
  host_linearise(d, 0, 1);
  if (blk_info3)
    for (int b = 0; b < pl.NB; ++b) {
      blk_info3[3 * b] = pl.blk[(size_t)b].cam;
      blk_info3[3 * b + 1] = pl.blk[(size_t)b].s;
      blk_info3[3 * b + 2] = so[(size_t)pl.blk[(size_t)b].s];
    }
  if (residuals)
    for (int b = 0; b < pl.NB; ++b) { residuals[2 * b] = ba_lin(d, 0, b); residuals[2 * b + 1] = ba_lin(d, 1, b); }
  if (g) std::fill(g, g + nu, 0.0);
  if (H) std::fill(H, H + (size_t)nu * nu, 0.0);
  if (g || H)
    for (int b = 0; b < pl.NB; ++b) {
      const BaBlk &bk = pl.blk[(size_t)b];
      int col[10];
      double J[2][10];
      int nc = 6;
      for (int a = 0; a < 6; ++a) { col[a] = 6 * bk.cam + a; J[0][a] = ba_lin(d, 3 + a, b); J[1][a] = ba_lin(d, 9 + a, b); }
      if (so[(size_t)bk.s] >= 0)
        for (int l = 0; l < (bk.kind ? 4 : 3); ++l, ++nc) {
          col[nc] = so[(size_t)bk.s] + l;
          J[0][nc] = ba_lin(d, 15 + l, b);
          J[1][nc] = ba_lin(d, 19 + l, b);
        }
      const double r0 = ba_lin(d, 0, b), r1 = ba_lin(d, 1, b), rho1 = ba_lin(d, 2, b);
      for (int x = 0; x < nc; ++x) {
        if (g) g[col[x]] += rho1 * (J[0][x] * r0 + J[1][x] * r1);
        if (H)
          for (int y = 0; y < nc; ++y) H[(size_t)col[x] * nu + col[y]] += rho1 * (J[0][x] * J[0][y] + J[1][x] * J[1][y]);
      }
    }
  if (step) {  // the Schur route's step at radius mu
    std::fill(step, step + nu, std::nan(""));
    bool ok = true;
    for (int s = 0; s < pl.NS; ++s) ok = ba_item_vinv(d, s, mu) && ok;
    if (ok) {
      for (int i = 0; i < d.C; ++i) host_schur_row(d, i, mu);
      ok = ba_cholesky_host(d.n, d.S, d.rhs, d.LT, d.dc);
    }
    if (ok) {
      for (int s = 0; s < pl.NS; ++s) ba_item_backsub_struct(d, 0, s);
      for (int i = 0; i < d.n; ++i) step[i] = d.dc[i];
      for (int s = 0; s < pl.NS; ++s)
        if (so[(size_t)s] >= 0)
          for (int l = 0; l < (pl.st[(size_t)s].kind ? 4 : 3); ++l) step[so[(size_t)s] + l] = d.ds[(size_t)4 * s + l];
    }
  }
  return LT_OK;
}

int lt_fn_ba_point_eval(int n_img, const int32_t *img_ids, const double *kvec4, const double *qvec4, const double *tvec3,
                        int64_t n_pt, const double *pt3, const int64_t *pt_off, const int32_t *pt_img, const double *pt_xy2,
                        int64_t n_ln, const double *line6, const int64_t *ln_off, const int32_t *ln_img, const double *l2d4,
                        const double *l3d6, const lt_ba_config *cfg, int64_t track, const double p3[3], double *cost,
                        double g[4], double H[16]) {
  const Input in = make_input(n_img, img_ids, kvec4, qvec4, tvec3, n_pt, pt3, pt_off, pt_img, pt_xy2, n_ln, line6, ln_off,
                              ln_img, l2d4, l3d6, cfg);
  std::string msg;
  Plan pl;
  if (int rc = g_host_error.check("lt_fn_ba_point_eval", make_plan(in, pl, msg), msg)) return rc;
  if (!pl.constant_pose || !p3 || track < 0 || track >= pl.NP)
    return g_host_error.refuse("lt_fn_ba_point_eval", "constant_pose=1, a point and a point track's index are needed");
  BaDev d;
  bind_points(pl, d);
  std::vector<double> pose = pl.pose0, sp = pl.sp0;
  d.kvec = pl.kvec.data(); d.pose = pose.data(); d.sp = sp.data();
  d.st = pl.st.data(); d.blk = pl.blk.data();
  BaPointGroup<LmHostLanes<kBaWidth>> grp{{}, d, pl.st[(size_t)track]};
  if (cost) *cost = grp.cost(p3);
  double acc[kRfSums];
  grp.linearise(p3, acc);
  sums_to_gH<4>(acc, g, H);
  return LT_OK;
}

// a group whose reductions are read from a script: the k-th cost, the k-th linearisation
struct ScriptGroup {
  const double *costs, *accs;
  int64_t n_costs, n_lin, i_cost = 0, i_lin = 0;
  bool short_of = false;
  double cost(const double *) {
    if (i_cost >= n_costs) { short_of = true; return std::nan(""); }
    return costs[i_cost++];
  }
  void linearise(const double *, double acc[kRfSums]) {
    if (i_lin >= n_lin) { short_of = true; std::fill(acc, acc + kRfSums, std::nan("")); return; }
    std::copy(accs + kRfSums * i_lin, accs + kRfSums * (i_lin + 1), acc);
    ++i_lin;
  }
};

int lt_fn_lm_loop_script(double F, int max_iter, int64_t n_costs, const double *costs, int64_t n_lin, const double *acc14,
                         double p3[3], double *cost1, int32_t *iters, int32_t *code, int64_t used2[2]) {
  if (!p3 || !cost1 || !iters || !code || n_costs < 0 || n_lin < 0 || (n_costs > 0 && !costs) || (n_lin > 0 && !acc14))
    return LT_ERR_ARGUMENT;
  ScriptGroup grp{costs, acc14, n_costs, n_lin};
  int it = 0, cd = 0;
  lm_loop<BaPointChart>(grp, F, max_iter, p3, cost1, &it, &cd);
  *iters = it;
  *code = cd;
  if (used2) { used2[0] = grp.i_cost; used2[1] = grp.i_lin; }
  return grp.short_of ? LT_ERR_STATE : LT_OK;
}

int lt_fn_ba_host_trace(int n_img, const int32_t *img_ids, const double *kvec4, const double *qvec4, const double *tvec3,
                        int64_t n_pt, const double *pt3, const int64_t *pt_off, const int32_t *pt_img, const double *pt_xy2,
                        int64_t n_ln, const double *line6, const int64_t *ln_off, const int32_t *ln_img, const double *l2d4,
                        const double *l3d6, const lt_ba_config *cfg, int64_t cap, int64_t *n_attempts, double *total0,
                        double *rec5, double *cost2, int32_t *iters, int32_t *code) {
  const Input in = make_input(n_img, img_ids, kvec4, qvec4, tvec3, n_pt, pt3, pt_off, pt_img, pt_xy2, n_ln, line6, ln_off,
                              ln_img, l2d4, l3d6, cfg);
  std::string msg;
  Plan pl;
  if (int rc = g_host_error.check("lt_fn_ba_host_trace", make_plan(in, pl, msg), msg)) return rc;
  if (pl.constant_pose || pl.NB == 0 || cap < 0 || !n_attempts || !total0 || (cap > 0 && !rec5))
    return g_host_error.refuse("lt_fn_ba_host_trace", "free poses, a residual block and the outputs are needed");
  HostTables h;
  host_tables(pl, h);
  host_init(h.dev, 1, total0);
  int64_t n = 0;
  while (!h.status.done) {
    double rec[5];
    host_attempt(h.dev, 1, rec);
    if (n < cap) std::copy(rec, rec + 5, rec5 + 5 * n);
    ++n;
  }
  *n_attempts = n;
  if (cost2) { cost2[0] = h.status.F0; cost2[1] = h.status.F; }
  if (iters) *iters = h.status.iters;
  if (code) *code = h.status.code;
  return LT_OK;
}

int lt_fn_ba_cholesky(int64_t n, const double *S, const double *rhs, double *L, double *x) {
  if (n < 0 || n > 4096 || (n > 0 && (!S || !L))) return LT_ERR_ARGUMENT;
  std::vector<double> LT((size_t)n * (size_t)n, 0.0);
  const bool ok = ba_cholesky_host((int)n, S, rhs, LT.data(), x);
  for (int64_t i = 0; i < n; ++i)
    for (int64_t k = 0; k < n; ++k) L[(size_t)i * n + k] = k <= i ? LT[(size_t)k * n + i] : 0.0;
  return ok ? LT_OK : LT_ERR_STATE;
}

}  // extern "C"
