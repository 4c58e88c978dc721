// lt_assoc.cpp -- the global point-line association of limap.optimize.global_pl_association (GlobalAssociator:
// global_associator.cc:176-305) with constant cameras.  Validation, the residual blocks and association edges in SetUp()'s
// order with their ScaledLoss weights, the adjacency lists of the block-sparse matrix, upload, the launch loop of
// lt_kernels_assoc.hip and the download; lt_fn_assoc_host is the whole solve in plain C++ from the same inline functions
// (lt_assoc.h) with every reduction in the device's order, so both agree bit for bit.

#include "lt_host.h"
#include "lt_assoc.h"
#include "lt_ingest.h"
#include "lt_twin.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include <omp.h>

using namespace lt;
using namespace lt_impl;

namespace {

struct Plan {
  int NU = 0, NP = 0, NL = 0, NV = 0, NB = 0, NE = 0, n_img = 0;
  double alpha = 10.0, eta = kAsEtaDefault;
  int max_iter = 0, cg_cap = kAsCgCapDefault, poll = kAsPollDefault, cg_batch = kAsCgBatchDefault, kernel_timers = 0;
  std::vector<double> kvec, pose, sp0;  // 4 / 7 per image, 6 per unknown
  std::vector<AsUnk> unk;
  std::vector<BaBlk> blk;
  std::vector<AsEdge> edge;
  std::vector<int> adj;
};

int check_config(const lt_assoc_config *c, std::string &msg) {
  if (!c) { msg = "null configuration"; return 1; }
  if (!c->constant_intrinsics) { msg = "constant_intrinsics=0 is not built (the associator holds the cameras constant)"; return 1; }
  if (!c->constant_pose) { msg = "constant_pose=0 is not built (the associator holds the cameras constant)"; return 1; }
  if (!(c->geometric_alpha >= 0.0) || !(c->geometric_alpha <= 700.0)) { msg = "geometric_alpha outside [0, 700]"; return 1; }
  if (c->max_num_iterations < 0) { msg = "max_num_iterations is negative"; return 1; }
  if (!std::isfinite(c->lw_point) || !std::isfinite(c->lw_pointline_association) || !std::isfinite(c->lw_vpline_association) ||
      !std::isfinite(c->lw_vp_orthogonality) || !std::isfinite(c->lw_vp_collinearity)) {
    msg = "a loss weight is not finite";
    return 1;
  }
  if (!(c->cg_eta >= 0.0) || !(c->cg_eta < 1.0)) { msg = "cg_eta outside [0, 1)"; return 1; }
  if (c->cg_max_iterations < 1) { msg = "cg_max_iterations is below 1"; return 1; }
  if (c->poll_interval < 0 || c->cg_batch < 0 || c->cg_batch > kAsCgBatchMax) { msg = "poll_interval or cg_batch out of range"; return 1; }
  return 0;
}

// the adjacency lists of the unknowns from the edges: ascending edge order
void make_adjacency(std::vector<AsUnk> &unk, const std::vector<AsEdge> &edge, std::vector<int> &adj) {
  for (AsUnk &u : unk) u.na = 0;
  for (const AsEdge &e : edge) { unk[(size_t)e.a].na += 1; unk[(size_t)e.b].na += 1; }
  int at = 0;
  for (AsUnk &u : unk) { u.a0 = at; at += u.na; u.na = 0; }
  adj.assign(2 * (size_t)at, 0);
  for (size_t i = 0; i < edge.size(); ++i)
    for (int side = 0; side < 2; ++side) {
      AsUnk &u = unk[(size_t)(side ? edge[i].b : edge[i].a)];
      adj[2 * (size_t)(u.a0 + u.na)] = (int)i;
      adj[2 * (size_t)(u.a0 + u.na) + 1] = side;
      u.na += 1;
    }
}

int make_plan(const lt_assoc_input *inp, const lt_assoc_config *cfgp, Plan &pl, std::string &msg) {
  if (check_config(cfgp, msg)) return 1;
  if (!inp) { msg = "null input"; return 1; }
  const lt_assoc_input &in = *inp;
  const lt_assoc_config &cfg = *cfgp;
  IdRows id2row;
  if (ingest_cams(in.n_img, in.img_ids, in.kvec4, in.qvec4, in.tvec3, id2row, msg)) return 1;
  if (in.n_pt < 0 || in.n_ln < 0 || in.n_vp < 0 || in.n_edge < 0) { msg = "bad counts"; return 1; }
  if (in.n_pt > 0) {
    msg = offsets_msg("point track", in.n_pt, in.pt_off);
    if (!msg.empty()) return 1;
  }
  if (in.n_ln > 0) {
    msg = offsets_msg("line track", in.n_ln, in.ln_off);
    if (!msg.empty()) return 1;
  }
  const long long MP = in.n_pt > 0 ? in.pt_off[in.n_pt] : 0, ML = in.n_ln > 0 ? in.ln_off[in.n_ln] : 0;
  if ((in.n_pt > 0 && !in.pt3) || (MP > 0 && (!in.pt_img || !in.pt_xy2)) || (in.n_ln > 0 && !in.line6) ||
      (ML > 0 && (!in.ln_img || !in.l2d4)) || (in.n_vp > 0 && !in.vp3) ||
      (in.n_edge > 0 && (!in.edge_kind || !in.edge_a || !in.edge_b || !in.edge_w))) {
    msg = "null arrays";
    return 1;
  }
  if (!all_finite(in.pt3, 3 * in.n_pt) || !all_finite(in.pt_xy2, 2 * MP) || !all_finite(in.line6, 6 * in.n_ln) ||
      !all_finite(in.l2d4, 4 * ML) || !all_finite(in.vp3, 3 * in.n_vp) || !all_finite(in.edge_w, in.n_edge)) {
    msg = "non-finite coordinate";
    return 1;
  }
  if (in.n_pt + in.n_ln + in.n_vp > (long long)(1 << 27) || MP + ML + in.n_edge > (long long)(1 << 27)) {
    msg = "too many unknowns or blocks for one call";
    return 1;
  }
  pl.alpha = cfg.geometric_alpha;
  pl.eta = cfg.cg_eta;
  pl.cg_cap = cfg.cg_max_iterations;
  pl.max_iter = cfg.max_num_iterations;
  pl.poll = cfg.poll_interval > 0 ? cfg.poll_interval : kAsPollDefault;
  pl.cg_batch = cfg.cg_batch > 0 ? cfg.cg_batch : kAsCgBatchDefault;
  pl.kernel_timers = cfg.kernel_timers;
  pl.n_img = in.n_img;
  pl.NP = (int)in.n_pt; pl.NL = (int)in.n_ln; pl.NV = (int)in.n_vp;
  pl.NU = pl.NP + pl.NL + pl.NV;
  pl.unk.assign((size_t)pl.NU, AsUnk{0, 0, 0, 0, 0, 0, {0, 0}});
  pl.sp0.assign(6 * (size_t)pl.NU, 0.0);
  const bool cpt = cfg.constant_point != 0, cln = cfg.constant_line != 0, cvp = cfg.constant_vp != 0;
  // R1.1 (global_associator.cc:182-187): only where the points are free; AddPointGeometricResiduals returns at once
  // without a weight
  const bool add_points = !cpt && cfg.lw_point > 0.0;
  for (int64_t n = 0; n < in.n_pt; ++n) {
    AsUnk &u = pl.unk[(size_t)n];
    u.kind = kAsPoint;
    u.b0 = (int)pl.blk.size();
    for (int c = 0; c < 3; ++c) pl.sp0[6 * (size_t)n + c] = in.pt3[3 * n + c];
    if (add_points && ingest_point_track(n, (int)n, in.pt_off, in.pt_img, in.pt_xy2, cfg.lw_point, id2row, pl.blk, msg)) return 1;
    u.nb = (int)pl.blk.size() - u.b0;
  }
  // R1.2 (:189-194): only where the lines are free; §19's order (sorted images, then list order) and weights
  SupportOrder so;
  std::vector<char> few((size_t)std::max(pl.NL, 1), 0);
  for (int64_t n = 0; n < in.n_ln; ++n) {
    const int ui = pl.NP + (int)n;
    AsUnk &u = pl.unk[(size_t)ui];
    u.kind = kAsLine;
    u.b0 = (int)pl.blk.size();
    if (ingest_line_length("line track", n, in.line6 + 6 * n, msg)) return 1;
    rf_minimal(in.line6 + 6 * n, pl.sp0.data() + 6 * (size_t)ui);
    const long long a = in.ln_off[n];
    int n_images;
    if (ingest_supports("line track", n, in.ln_img + a, (int)(in.ln_off[n + 1] - a), id2row, so, &n_images, msg, [&](int, int x, int row) {
          if (!cln) pl.blk.push_back(line_blk(in.l2d4 + 4 * (a + x), row, ui));
        }))
      return 1;
    few[(size_t)n] = n_images < cfg.min_num_images;
    u.nb = (int)pl.blk.size() - u.b0;
  }
  pl.NB = (int)pl.blk.size();
  for (int64_t n = 0; n < in.n_vp; ++n) {
    const int ui = pl.NP + pl.NL + (int)n;
    pl.unk[(size_t)ui].kind = kAsVp;
    const double *v = in.vp3 + 3 * n;
    if (!(std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) > 0.0)) {
      msg = "vanishing point " + std::to_string(n) + " has zero length";
      return 1;
    }
    for (int c = 0; c < 3; ++c) pl.sp0[6 * (size_t)ui + c] = v[c];
  }
  // R2.1 - R2.4 (:196-213, 222-305)
  const bool on[4] = {cfg.enable_pointline && (!cpt || !cln) && cfg.lw_pointline_association > 0.0,
                      cfg.enable_vpline && (!cvp || !cln) && cfg.lw_vpline_association > 0.0,
                      cfg.enable_vpline && !cvp && cfg.lw_vp_orthogonality > 0.0,
                      cfg.enable_vpline && !cvp && cfg.lw_vp_collinearity > 0.0};
  for (int64_t i = 0; i < in.n_edge; ++i) {
    const int kind = in.edge_kind[i], a = in.edge_a[i], b = in.edge_b[i];
    if (kind < 0 || kind > 3) { msg = "edge " + std::to_string(i) + ": unknown kind"; return 1; }
    const int na = kind == kAsPL ? pl.NP : pl.NV, nb = kind <= kAsVL ? pl.NL : pl.NV;
    if (a < 0 || a >= na || b < 0 || b >= nb || (kind >= kAsOrth && a == b)) {
      msg = "edge " + std::to_string(i) + ": an id is not in the collection";
      return 1;
    }
    if (!on[kind]) continue;
    AsEdge e{0.0, kind, (kind == kAsPL ? 0 : pl.NP + pl.NL) + a, (kind <= kAsVL ? pl.NP : pl.NP + pl.NL) + b, 0};
    if (kind == kAsPL) e.w = in.edge_w[i] * cfg.lw_pointline_association;
    else if (kind == kAsVL) e.w = (in.edge_w[i] * 1e2) * cfg.lw_vpline_association;
    else e.w = 1e2 * (kind == kAsOrth ? cfg.lw_vp_orthogonality : cfg.lw_vp_collinearity);
    pl.edge.push_back(e);
  }
  pl.NE = (int)pl.edge.size();
  make_adjacency(pl.unk, pl.edge, pl.adj);
  // an unknown without a block is no parameter of the problem; the switches hold the others constant
  for (int u = 0; u < pl.NU; ++u) {
    AsUnk &un = pl.unk[(size_t)u];
    const bool any = un.nb > 0 || un.na > 0;
    if (un.kind == kAsPoint) un.nd = (!cpt && any) ? 3 : 0;
    else if (un.kind == kAsLine) un.nd = (!cln && !few[(size_t)(u - pl.NP)] && any) ? 4 : 0;
    else un.nd = (!cvp && any) ? 2 : 0;
    if (un.kind == kAsVp && un.nd) {  // the chart's point is a unit vector
      double *v = pl.sp0.data() + 6 * (size_t)u;
      const double nv = std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
      for (int c = 0; c < 3; ++c) v[c] = v[c] / nv;
    }
  }
  // every camera row; those of the images that carry an R1 block are checked
  std::vector<char> used((size_t)std::max(in.n_img, 1), 0);
  for (const BaBlk &b : pl.blk) used[(size_t)b.cam] = 1;
  pl.kvec.assign(4 * (size_t)std::max(in.n_img, 1), 0.0);
  pl.pose.assign(7 * (size_t)std::max(in.n_img, 1), 0.0);
  for (int r = 0; r < in.n_img; ++r)
    if (ingest_cam_row(in.img_ids, in.kvec4, in.qvec4, in.tvec3, r, used[(size_t)r] != 0, pl.kvec.data() + 4 * (size_t)r,
                       pl.pose.data() + 7 * (size_t)r, msg))
      return 1;
  return 0;
}

struct Result {
  std::vector<double> sp;  // the current set: 6 NU
  AsStatus status;
};

struct HostTables {
  std::vector<double> sp, lin, elin, E, D, A, Minv, x, r, z, p, Ap, xl, rl, Apl, chunk;
  AsStatus status;
  AsDev dev;
};

void bind_plan(const Plan &pl, AsDev &d) {
  d = AsDev{};
  d.NU = pl.NU; d.NP = pl.NP; d.NL = pl.NL; d.NV = pl.NV; d.NB = pl.NB; d.NE = pl.NE;
  d.n_chunks = lm_chunks_of((long long)pl.NB + pl.NE);
  d.n_uchunks = lm_chunks_of(pl.NU);
  d.alpha = pl.alpha;
}
AsStatus first_status(const Plan &pl) {
  AsStatus s = AsStatus{};
  s.lm.max_iter = pl.max_iter;
  s.eta = pl.eta;
  s.cg_cap = pl.cg_cap;
  s.phase = kAsHead;
  return s;
}

// the work tables of the linear solve alone (lt_fn_assoc_pcg) or of a whole solve
void host_solver_tables(HostTables &h) {
  AsDev &d = h.dev;
  const size_t nu = (size_t)std::max(d.NU, 1);
  h.D.assign(kRfSums * nu, 0.0); h.A.assign(16 * nu, 0.0); h.Minv.assign(16 * nu, 0.0);
  h.x.assign(4 * nu, 0.0); h.r.assign(4 * nu, 0.0); h.z.assign(4 * nu, 0.0); h.p.assign(4 * nu, 0.0); h.Ap.assign(4 * nu, 0.0);
  h.xl.assign(4 * nu, 0.0); h.rl.assign(4 * nu, 0.0); h.Apl.assign(4 * nu, 0.0);
  h.chunk.assign(2 * (size_t)std::max(d.n_chunks, d.n_uchunks), 0.0);
  d.D = h.D.data(); d.A = h.A.data(); d.Minv = h.Minv.data();
  d.x = h.x.data(); d.r = h.r.data(); d.z = h.z.data(); d.p = h.p.data(); d.Ap = h.Ap.data();
  d.xl = h.xl.data(); d.rl = h.rl.data(); d.Apl = h.Apl.data();
  d.chunk = h.chunk.data();
  d.status = &h.status;
}
void host_tables(const Plan &pl, HostTables &h) {
  AsDev &d = h.dev;
  bind_plan(pl, d);
  h.sp.assign(2 * 6 * (size_t)std::max(pl.NU, 1), 0.0);
  std::copy(pl.sp0.begin(), pl.sp0.end(), h.sp.begin());
  h.lin.assign((size_t)kAsLinFields * std::max(pl.NB, 1), 0.0);
  h.elin.assign((size_t)kAsELinFields * std::max(pl.NE, 1), 0.0);
  h.E.assign(16 * (size_t)std::max(pl.NE, 1), 0.0);
  d.kvec = pl.kvec.data(); d.pose = pl.pose.data(); d.sp = h.sp.data();
  d.unk = pl.unk.data(); d.blk = pl.blk.data(); d.edge = pl.edge.data(); d.adj = pl.adj.data();
  d.lin = h.lin.data(); d.elin = h.elin.data(); d.E = h.E.data();
  host_solver_tables(h);
  h.status = first_status(pl);
}

// ---- the host twins of the kernels ----
// the chunked reduction over the solve's chunk table (lm_chunks_host, lm_totals_host)
template <class F>
void host_chunks(const AsDev &d, int n_items, int n_chunks, int stride, int nt, F item) {
  lm_chunks_host(d.chunk, n_items, n_chunks, stride, nt, item);
}
void host_totals(const AsDev &d, int n, int stride, double *a, double *b) { lm_totals_host(d.chunk, n, stride, a, b); }
void host_cost(const AsDev &d, int set, bool with_md, int nt) {
  host_chunks(d, d.NB + d.NE, d.n_chunks, d.n_chunks, nt, [&](int i, double *a, double *b) {
    double c, m;
    as_item_cost(d, set, i, with_md, &c, &m);
    *a = *a + c;
    *b = *b + m;
  });
}
// k_as_linearize, k_as_diag, k_as_diag_vp
void host_linearise(const AsDev &d, int cur, int nt) {
#pragma omp parallel for num_threads(nt) schedule(static)
  for (int i = 0; i < d.NB + d.NE; ++i) {
    if (i < d.NB) as_item_lin_blk(d, cur, i);
    else as_item_lin_edge(d, cur, i - d.NB);
  }
#pragma omp parallel for num_threads(nt) schedule(static)
  for (int u = 0; u < d.NU; ++u) {
    const AsUnk un = d.unk[u];
    if (!un.nd) continue;
    if (un.kind == kAsVp) {
      double part[kAsWave][kRfSums], out[kRfSums];
      for (int l = 0; l < kAsWave; ++l) as_vp_part(d, un, l, part[l]);
      lm_tree_host(part, kRfSums, out);
      for (int c = 0; c < kRfSums; ++c) d.D[(size_t)kRfSums * u + c] = out[c];
    } else {
      double part[kAsWidth][kRfSums], out[kRfSums];
      for (int l = 0; l < kAsWidth; ++l) as_struct_part(d, un, l, part[l]);
      lm_tree_host(part, kRfSums, out);
      as_item_diag_store(d, u, out);
    }
  }
}
// k_as_precond (damp: from D and the radius; the linear solve alone brings its A) and k_as_cg_begin
void host_cg_begin(const AsDev &d, bool damp, int nt) {
  AsStatus &st = *d.status;
  int bad = 0;
  const double mu = st.lm.mu;
  std::vector<char> badv((size_t)d.n_uchunks, 0);
  host_chunks(d, d.NU, d.n_uchunks, d.n_uchunks, nt, [&](int u, double *a, double *b) {
    bool ok = true, nz = false;
    if (damp) as_item_damp(d, u, mu);
    *a = *a + as_item_cg_start(d, u, &ok, &nz);
    if (nz) *b = 1.0;
    if (!ok) badv[(size_t)(u / kAsChunk)] = 1;
  });
  for (char c : badv) bad |= c;
  if (bad) st.lm.bad = 1;
  double rz, flag;
  host_totals(d, d.n_uchunks, d.n_uchunks, &rz, &flag);
  as_decide_begin(st, rz, flag != 0.0);
}
// one CG iteration: k_as_matvec .. k_as_dir
void host_cg_iteration(const AsDev &d, int nt) {
  AsStatus &st = *d.status;
  double total, unused;
  host_chunks(d, d.NU, d.n_uchunks, 0, nt, [&](int u, double *a, double *) { *a = *a + as_item_matvec(d, u); });
  host_totals(d, d.n_uchunks, 0, &total, &unused);
  as_decide_alpha(st, total);
  if (st.phase != kAsCg) return;
  const double alpha = st.alpha;
  host_chunks(d, d.NU, d.n_uchunks, 0, nt, [&](int u, double *a, double *) { *a = *a + as_item_update(d, u, alpha); });
  host_totals(d, d.n_uchunks, 0, &total, &unused);
  as_decide_beta(st, total);
  if (st.phase != kAsCg) return;
  const double beta = st.beta;
#pragma omp parallel for num_threads(nt) schedule(static)
  for (int u = 0; u < d.NU; ++u) as_item_dir(d, u, beta);
}

void host_init(const AsDev &d, int nt, double *total0 = nullptr) {
  host_cost(d, 0, false, nt);
  double cost, md;
  host_totals(d, d.n_chunks, d.n_chunks, &cost, &md);
  if (total0) *total0 = cost;
  ba_decide_init(d.status->lm, cost);
  d.status->phase = kAsHead;
}

// one attempt: the head, the linear solve, the tail.  rec (tests): what the attempt hands to ba_decide_step
void host_attempt(const AsDev &d, int nt, double *rec = nullptr) {
  AsStatus &st = *d.status;
  if (st.lm.done) return;
  if (rec) { rec[0] = st.lm.mu; rec[1] = 0.0; rec[2] = st.lm.fresh; rec[3] = rec[4] = rec[5] = 0.0; }
  if (st.lm.fresh) host_linearise(d, st.lm.cur, nt);
  host_cg_begin(d, true, nt);
  if (st.lm.done) {
    if (rec) rec[1] = -1.0;
    return;
  }
  while (st.phase == kAsCg) host_cg_iteration(d, nt);
  if (!st.lm.bad) {
#pragma omp parallel for num_threads(nt) schedule(static)
    for (int u = 0; u < d.NU; ++u) as_item_backsub(d, st.lm.cur, u);
    host_cost(d, 1 - st.lm.cur, true, nt);
  }
  double cost, md;
  host_totals(d, d.n_chunks, d.n_chunks, &cost, &md);
  if (rec) { rec[1] = st.lm.bad; rec[3] = cost; rec[4] = md; rec[5] = st.lm.bad && st.cg_end == kAsCgPivot ? 0.0 : (double)st.cg_it; }
  ba_decide_step(st.lm, cost, md);
  st.phase = kAsHead;
}

void no_residuals(const Plan &pl, Result &res) {
  res.sp = pl.sp0;
  res.status = AsStatus{};
  res.status.lm.done = 1;
  res.status.lm.code = kLcNoResiduals;
}

void run_host(const Plan &pl, int n_threads, Result &res, int64_t cap, int64_t *n_attempts, double *total0, double *rec6) {
  const int nt = n_threads > 0 ? n_threads : omp_get_max_threads();
  HostTables h;
  host_tables(pl, h);
  host_init(h.dev, nt, total0);
  int64_t n = 0;
  while (!h.status.lm.done) {
    double rec[6];
    host_attempt(h.dev, nt, rec);
    if (rec6 && n < cap) std::copy(rec, rec + 6, rec6 + 6 * n);
    ++n;
  }
  if (n_attempts) *n_attempts = n;
  const int cur = h.status.lm.cur;
  res.sp.assign(h.sp.begin() + (size_t)cur * 6 * pl.NU, h.sp.begin() + (size_t)(cur + 1) * 6 * pl.NU);
  res.status = h.status;
}

struct Outputs {
  std::vector<double> pts, params, vps;
  double cost[2];
  int iters, code;
  long long cg_iters;
};
void gather(const Plan &pl, const Result &res, Outputs &o) {
  o.pts.resize(3 * (size_t)pl.NP);
  for (int n = 0; n < pl.NP; ++n)
    for (int x = 0; x < 3; ++x) o.pts[3 * (size_t)n + x] = res.sp[6 * (size_t)n + x];
  o.params.assign(res.sp.begin() + 6 * (size_t)pl.NP, res.sp.begin() + 6 * (size_t)(pl.NP + pl.NL));
  o.vps.resize(3 * (size_t)pl.NV);
  for (int n = 0; n < pl.NV; ++n)
    for (int x = 0; x < 3; ++x) o.vps[3 * (size_t)n + x] = res.sp[6 * (size_t)(pl.NP + pl.NL + n) + x];
  o.cost[0] = res.status.lm.F0;
  o.cost[1] = res.status.lm.F;
  o.iters = res.status.lm.iters;
  o.code = res.status.lm.code;
  o.cg_iters = res.status.cg_total;
}
void copy_out(const Outputs &o, double *pt3, double *params6, double *vp3, double *cost2, int32_t *iters, int64_t *cg_iters,
              int32_t *code) {
  if (pt3) std::copy(o.pts.begin(), o.pts.end(), pt3);
  if (params6) std::copy(o.params.begin(), o.params.end(), params6);
  if (vp3) std::copy(o.vps.begin(), o.vps.end(), vp3);
  if (cost2) { cost2[0] = o.cost[0]; cost2[1] = o.cost[1]; }
  if (iters) *iters = o.iters;
  if (cg_iters) *cg_iters = o.cg_iters;
  if (code) *code = o.code;
}

static thread_local HostError g_host_error;

#ifndef LT_HOST_ONLY  // (tools/assoc_host_asan.cpp compiles the host twin alone: no context, no HIP runtime)
int run_device(lt_ctx *ctx, const Plan &pl, Result &res, double timers[20]) {
  lt_host::AsState &as = ctx->as;
  const double t0 = now_ms();
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  AsDev d;
  bind_plan(pl, d);
  const size_t NU = (size_t)std::max(pl.NU, 1), NB = (size_t)std::max(pl.NB, 1), NE = (size_t)std::max(pl.NE, 1);
  std::vector<double> sp(2 * 6 * NU, 0.0), cam = pl.kvec;
  std::copy(pl.sp0.begin(), pl.sp0.end(), sp.begin());
  const size_t o_pose = cam.size();
  cam.insert(cam.end(), pl.pose.begin(), pl.pose.end());
  if (int rc = upload_vec(ctx, as.d_cam, cam)) return rc;
  if (int rc = upload_vec(ctx, as.d_sp, sp)) return rc;
  if (int rc = upload_vec(ctx, as.d_unk, pl.unk)) return rc;
  if (int rc = upload_vec(ctx, as.d_blk, pl.blk)) return rc;
  if (int rc = upload_vec(ctx, as.d_edge, pl.edge)) return rc;
  if (int rc = upload_vec(ctx, as.d_adj, pl.adj)) return rc;
  // lin 11 NB | elin 28 NE | E 16 NE
  const size_t o_elin = (size_t)kAsLinFields * NB, o_E = o_elin + (size_t)kAsELinFields * NE, n_lin = o_E + 16 * NE;
  // D 14 NU | A 16 NU | Minv 16 NU
  const size_t o_A = kRfSums * NU, o_Minv = o_A + 16 * NU, n_mat = o_Minv + 16 * NU;
  const size_t n_ch = 2 * (size_t)std::max(d.n_chunks, d.n_uchunks);
  ENSURE(ctx, as.d_lin, 8 * n_lin);
  ENSURE(ctx, as.d_mat, 8 * n_mat);
  ENSURE(ctx, as.d_vec, 8 * 8 * 4 * NU);  // x | r | z | p | Ap | xl | rl | Apl
  ENSURE(ctx, as.d_chunk, 8 * n_ch);
  ENSURE(ctx, as.d_status, sizeof(AsStatus));
  const AsStatus init = first_status(pl);
  HIPCHK(ctx, hipMemcpyAsync(as.d_status.p, &init, sizeof(AsStatus), hipMemcpyHostToDevice, st));
  d.kvec = as.d_cam.as<double>(); d.pose = d.kvec + o_pose; d.sp = as.d_sp.as<double>();
  d.unk = as.d_unk.as<AsUnk>(); d.blk = as.d_blk.as<BaBlk>(); d.edge = as.d_edge.as<AsEdge>(); d.adj = as.d_adj.as<int>();
  d.lin = as.d_lin.as<double>(); d.elin = d.lin + o_elin; d.E = d.lin + o_E;
  d.D = as.d_mat.as<double>(); d.A = d.D + o_A; d.Minv = d.D + o_Minv;
  d.x = as.d_vec.as<double>(); d.r = d.x + 4 * NU; d.z = d.r + 4 * NU; d.p = d.z + 4 * NU; d.Ap = d.p + 4 * NU;
  d.xl = d.Ap + 4 * NU; d.rl = d.xl + 4 * NU; d.Apl = d.rl + 4 * NU;
  d.chunk = as.d_chunk.as<double>();
  d.status = as.d_status.as<AsStatus>();
  if (int rc = stream_sync(ctx)) return rc;
  const double t1 = now_ms();
  timers[0] = t1 - t0;
  // the loop: its decisions are made on the device; `poll` batches -- the head of an attempt, cg_batch CG iterations, the
  // tail of an attempt -- are enqueued back to back, then the status record (128 bytes) comes back.  A kernel returns at
  // once unless the record is in its phase, so the result depends neither on the interval nor on the batch
  const int B = pl.cg_batch;
  EventList ev(pl.kernel_timers ? as_events(B) + 1 : 0);
  if (int rc = ev.create(ctx)) return rc;
  launch_as_init(st, d);
  AsStatus status = AsStatus{};
  long long launched = 0;
  if (int rc = run_polled(
          ctx, pl.kernel_timers ? 1 : pl.poll, as.d_status.p, status,
          [&]() {
            launch_as_attempt(st, d, B, pl.kernel_timers ? ev.data() : nullptr);
            ev.mark_all();
          },
          [](const AsStatus &s) { return s.lm.done != 0; },
          [&]() {
            for (int x = 0; x + 1 < ev.size(); ++x) {
              int slot;  // the kernel between the events x and x + 1
              if (x < kAsHeadKernels) slot = x;
              else if (x < kAsHeadKernels + kAsCgKernels * B) slot = kAsHeadKernels + (x - kAsHeadKernels) % kAsCgKernels;
              else slot = kAsHeadKernels + kAsCgKernels + (x - kAsHeadKernels - kAsCgKernels * B);
              timers[4 + slot] += ev.ms(x, x + 1);
            }
          },
          &launched))
    return rc;
  const double t2 = now_ms();
  timers[1] = t2 - t1;
  timers[3] = (double)launched;
  const int cur = status.lm.cur;
  if (int rc = download(ctx, res.sp, as.d_sp.as<double>() + (size_t)cur * 6 * pl.NU, 6 * (size_t)pl.NU)) return rc;
  if (int rc = stream_sync(ctx)) return rc;
  res.status = status;
  timers[2] = now_ms() - t2;
  return LT_OK;
}
#endif  // LT_HOST_ONLY

}  // namespace

extern "C" {

void lt_assoc_config_default(lt_assoc_config *cfg) {
  if (!cfg) return;
  *cfg = lt_assoc_config{};
  cfg->geometric_alpha = 10.0;  // hybrid_bundle_adjustment_config.h:17-49, global_associator.h:43-65
  cfg->lw_point = 0.1;
  cfg->lw_pointline_association = 10.0;
  cfg->lw_vpline_association = 1.0;
  cfg->lw_vp_orthogonality = 1.0;
  cfg->lw_vp_collinearity = 0.0;
  cfg->cg_eta = kAsEtaDefault;
  cfg->cg_max_iterations = kAsCgCapDefault;
  cfg->min_num_images = 4;
  cfg->max_num_iterations = 100;
  cfg->constant_intrinsics = 1;
  cfg->constant_pose = 1;
  cfg->enable_pointline = 1;
  cfg->enable_vpline = 1;
}

#ifndef LT_HOST_ONLY
int lt_assoc_arrays(lt_ctx *ctx, const lt_assoc_input *in, const lt_assoc_config *cfg) {
  if (!ctx) return LT_ERR_ARGUMENT;
  std::string msg;
  Plan pl;
  if (make_plan(in, cfg, pl, msg)) return fail(ctx, LT_ERR_ARGUMENT, "lt_assoc_arrays: " + msg);
  lt_host::AsState &as = ctx->as;
  for (double &x : as.timers) x = 0.0;
  Result res;
  if (pl.NB + pl.NE == 0) no_residuals(pl, res);
  else if (int rc = run_device(ctx, pl, res, as.timers)) return rc;
  Outputs o;
  gather(pl, res, o);
  as.pts = o.pts; as.params = o.params; as.vps = o.vps;
  as.cost[0] = o.cost[0]; as.cost[1] = o.cost[1];
  as.iters = o.iters; as.code = o.code; as.cg_iters = o.cg_iters;
  return LT_OK;
}

int lt_assoc_get(lt_ctx *ctx, double *pt3, double *params6, double *vp3, double *cost2, int32_t *iters, int64_t *cg_iters,
                 int32_t *code) {
  if (!ctx) return LT_ERR_ARGUMENT;
  const lt_host::AsState &as = ctx->as;
  Outputs o{as.pts, as.params, as.vps, {as.cost[0], as.cost[1]}, as.iters, as.code, as.cg_iters};
  copy_out(o, pt3, params6, vp3, cost2, iters, cg_iters, code);
  return LT_OK;
}

int lt_assoc_get_timers(lt_ctx *ctx, double out[20]) {
  if (!ctx || !out) return LT_ERR_ARGUMENT;
  for (int k = 0; k < 20; ++k) out[k] = ctx->as.timers[k];
  return LT_OK;
}
#endif  // LT_HOST_ONLY

const char *lt_fn_assoc_host_error(void) { return g_host_error.c_str(); }

int lt_fn_assoc_host(const lt_assoc_input *in, const lt_assoc_config *cfg, int host_threads, double *pt3, double *params6,
                     double *vp3, double *cost2, int32_t *iters, int64_t *cg_iters, int32_t *code, int64_t trace_cap,
                     int64_t *n_attempts, double *total0, double *rec6) {
  std::string msg;
  Plan pl;
  if (int rc = g_host_error.check("lt_fn_assoc_host", make_plan(in, cfg, pl, msg), msg)) return rc;
  Result res;
  if (n_attempts) *n_attempts = 0;
  if (total0) *total0 = 0.0;
  if (pl.NB + pl.NE == 0) no_residuals(pl, res);
  else run_host(pl, host_threads, res, trace_cap, n_attempts, total0, trace_cap > 0 ? rec6 : nullptr);
  Outputs o;
  gather(pl, res, o);
  copy_out(o, pt3, params6, vp3, cost2, iters, cg_iters, code);
  return LT_OK;
}

int lt_fn_assoc_eval(const lt_assoc_input *in, const lt_assoc_config *cfg, const double *sp6, int64_t *dims8,
                     int32_t *unk_nd, int32_t *blk_unk, int32_t *edge_info3, double *edge_w, double *sp6_out,
                     double *res_blk, double *res_edge, double *cost, double *g4, double *diag16, double *off16) {
  std::string msg;
  Plan pl;
  if (int rc = g_host_error.check("lt_fn_assoc_eval", make_plan(in, cfg, pl, msg), msg)) return rc;
  if (dims8) {
    const int64_t v[8] = {pl.NU, pl.NP, pl.NL, pl.NV, pl.NB, pl.NE, 0, 0};
    std::copy(v, v + 8, dims8);
  }
  if (!unk_nd && !blk_unk && !edge_info3 && !edge_w && !sp6_out && !res_blk && !res_edge && !cost && !g4 && !diag16 && !off16)
    return LT_OK;
  if (sp6) {
    if (!all_finite(sp6, 6 * (long long)pl.NU)) return g_host_error.refuse("lt_fn_assoc_eval", "non-finite point");
    std::copy(sp6, sp6 + 6 * (size_t)pl.NU, pl.sp0.begin());
  }
  HostTables h;
  host_tables(pl, h);
  const AsDev &d = h.dev;
  host_init(d, 1);
  host_linearise(d, 0, 1);
  for (int u = 0; u < pl.NU; ++u) {
    if (unk_nd) unk_nd[u] = pl.unk[(size_t)u].nd;
    const int nd = pl.unk[(size_t)u].nd;
    if (g4)
      for (int c = 0; c < 4; ++c) g4[4 * (size_t)u + c] = c < nd ? d.D[(size_t)kRfSums * u + 10 + c] : 0.0;
    if (diag16) {
      int o = 0;
      for (int i = 0; i < 4; ++i)
        for (int j = i; j < 4; ++j, ++o)
          diag16[16 * (size_t)u + 4 * i + j] = diag16[16 * (size_t)u + 4 * j + i] = (i < nd && j < nd) ? d.D[(size_t)kRfSums * u + o] : 0.0;
    }
  }
  if (sp6_out) std::copy(pl.sp0.begin(), pl.sp0.end(), sp6_out);
  for (int b = 0; b < pl.NB; ++b) {
    if (blk_unk) blk_unk[b] = pl.blk[(size_t)b].s;
    if (res_blk) { res_blk[2 * b] = as_lin(d, 0, b); res_blk[2 * b + 1] = as_lin(d, 1, b); }
  }
  for (int e = 0; e < pl.NE; ++e) {
    const AsEdge &ed = pl.edge[(size_t)e];
    if (edge_info3) { edge_info3[3 * e] = ed.kind; edge_info3[3 * e + 1] = ed.a; edge_info3[3 * e + 2] = ed.b; }
    if (edge_w) edge_w[e] = ed.w;
    if (res_edge)
      for (int m = 0; m < 3; ++m) res_edge[3 * e + m] = as_elin(d, m, e);
    if (off16) std::copy(d.E + (size_t)16 * e, d.E + (size_t)16 * (e + 1), off16 + (size_t)16 * e);
  }
  if (cost) *cost = h.status.lm.F;
  return LT_OK;
}

int lt_fn_assoc_link2d(const double l1[4], const double l2[4]) {
  if (!l1 || !l2) return 0;
  LinkCfg2 c;  // LineLinker2dConfig's defaults (line_linker.h:23-45)
  c.score_th = 0.5; c.th_angle = 8.0; c.th_overlap = 0.1; c.th_smartoverlap = 0.2; c.th_smartangle = 1.0;
  c.th_perp = 5.0; c.th_innerseg = 5.0;
  c.mult = 1.0 / std::sqrt(-std::log(c.score_th) * 2.0);
  c.use_angle = c.use_overlap = c.use_smartangle = c.use_perp = 1;
  c.use_innerseg = c.pad_ = 0;
  L2 a, b;
  a.s.x = l1[0]; a.s.y = l1[1]; a.e.x = l1[2]; a.e.y = l1[3];
  b.s.x = l2[0]; b.s.y = l2[1]; b.e.x = l2[2]; b.e.y = l2[3];
  return check2d(c, a, b) ? 1 : 0;
}

int lt_fn_assoc_pcg(int64_t n_unk, const int32_t *nd, const double *diag16, int64_t n_edge, const int32_t *edge_a,
                    const int32_t *edge_b, const double *off16, const double *rhs4, double eta, int32_t cap, double *x4,
                    int32_t *iters, int32_t *end, double *rz2) {
  if (n_unk < 1 || n_unk > (1 << 24) || n_edge < 0 || n_edge > (1 << 26) || !nd || !diag16 || !rhs4 || !x4 || !iters || !end ||
      (n_edge > 0 && (!edge_a || !edge_b || !off16)) || !(eta >= 0.0) || cap < 1)
    return LT_ERR_ARGUMENT;
  std::vector<AsUnk> unk((size_t)n_unk, AsUnk{0, 0, 0, 0, 0, 0, {0, 0}});
  for (int64_t u = 0; u < n_unk; ++u) {
    if (nd[u] < 0 || nd[u] > 4) return LT_ERR_ARGUMENT;
    unk[(size_t)u].nd = nd[u];
  }
  std::vector<AsEdge> edge((size_t)n_edge);
  for (int64_t e = 0; e < n_edge; ++e) {
    if (edge_a[e] < 0 || edge_a[e] >= n_unk || edge_b[e] < 0 || edge_b[e] >= n_unk || edge_a[e] == edge_b[e]) return LT_ERR_ARGUMENT;
    edge[(size_t)e] = AsEdge{0.0, 0, edge_a[e], edge_b[e], 0};
  }
  std::vector<int> adj;
  make_adjacency(unk, edge, adj);
  HostTables h;
  AsDev &d = h.dev;
  d = AsDev{};
  d.NU = (int)n_unk;
  d.NE = (int)n_edge;
  d.n_chunks = 1;
  d.n_uchunks = lm_chunks_of(d.NU);
  host_solver_tables(h);
  // the given blocks, the entries outside an unknown's dimensions zero
  std::vector<double> E(16 * (size_t)std::max<int64_t>(n_edge, 1), 0.0);
  for (int64_t u = 0; u < n_unk; ++u)
    for (int i = 0; i < nd[u]; ++i) {
      for (int j = 0; j < nd[u]; ++j) h.A[16 * (size_t)u + 4 * i + j] = diag16[16 * u + 4 * i + j];
      h.D[kRfSums * (size_t)u + 10 + i] = -rhs4[4 * u + i];
    }
  for (int64_t e = 0; e < n_edge; ++e)
    for (int i = 0; i < nd[edge_a[e]]; ++i)
      for (int j = 0; j < nd[edge_b[e]]; ++j) E[16 * (size_t)e + 4 * i + j] = off16[16 * e + 4 * i + j];
  d.unk = unk.data(); d.edge = edge.data(); d.adj = adj.data(); d.E = E.data();
  h.status = AsStatus{};
  h.status.eta = eta;
  h.status.cg_cap = cap;
  h.status.phase = kAsHead;
  host_cg_begin(d, false, 1);
  while (h.status.phase == kAsCg) host_cg_iteration(d, 1);
  std::copy(h.x.begin(), h.x.begin() + 4 * (size_t)n_unk, x4);
  *iters = h.status.cg_it;
  *end = h.status.cg_end;
  if (rz2) { rz2[0] = h.status.rz0; rz2[1] = h.status.rz; }
  return LT_OK;
}

}  // extern "C"
