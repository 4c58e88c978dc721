// lt_assoc.h -- records and the FP64 expressions shared by the host side (lt_assoc.cpp) and the device side
// (lt_kernels_assoc.hip) of the global point-line association: limap.optimize.global_pl_association's GlobalAssociator
// with constant cameras.  The unknowns are the points (3 each), the lines (4, §19's chart) and the
// vanishing points (2, the chart below), coupled by a sparse graph of association edges; the linear step of §27's loop
// is preconditioned conjugate gradients on the explicitly assembled block-sparse matrix.  Both sides compile the same
// inline functions with -ffp-contract=off and reduce in the same fixed orders, so the device and lt_fn_assoc_host agree
// bit for bit.
//
// limap's own part is restated in its operation order: paths relative to src/limap,
//   optimize/global_pl_association/cost_functions.h:105-136   PointLineAssociation3dFunctor (R2.1)
//   optimize/global_pl_association/cost_functions.h:142-159   VPLineAssociation3dFunctor (R2.2)
//   optimize/global_pl_association/cost_functions.h:165-199   VPOrthogonalityFunctor (R2.3), VPCollinearityFunctor (R2.4)
//   ceresbase/line_dists.h:40-78                              CeresComputeDist3D_sine / _cosine
//   optimize/global_pl_association/global_associator.cc:176-305   SetUp and the four Add*Residuals (weights and losses)
//   optimize/global_pl_association/global_associator.h:68-73      HuberLoss(0.01) twice, TrivialLoss twice
// R1.1 and R1.2 are §27's blocks (ba_res) with the camera a constant.
// ASSUMPTIONS as in lt_ba.h, and ceres::CrossProduct, HuberLoss (rho = s, or 2 a sqrt(s) - a^2 above a^2) as published.
#pragma once

#include "lt_ba.h"

namespace lt {

constexpr int kAsWave = kBaWave;   // lanes per chunk of the reductions, per vanishing point of k_as_diag_vp
constexpr int kAsWidth = kBaWidth; // lanes per point or line of k_as_diag (§19's group)
constexpr int kAsChunk = kBaChunk; // residual blocks per chunk of the cost, unknowns per chunk of a dot product
constexpr int kAsLinFields = 11;   // doubles per R1 block of a linearisation (SoA): r[2], rho', J[2][4]
constexpr int kAsELinFields = 28;  // per association edge: r[3], rho', J_a[3][4], J_b[3][4]
constexpr int kAsPollDefault = 4;  // attempts enqueued between two reads of the status record
constexpr int kAsCgBatchDefault = 4;   // CG iterations enqueued per attempt of a batch (Jacobi blocks meet eta 0.1 in 1 - 2)
constexpr int kAsCgBatchMax = 64;
constexpr double kAsHuberA = 0.01;     // both association losses (global_associator.h:69-70)
constexpr double kAsEtaDefault = 0.1;  // Ceres' Solver::Options::eta
constexpr int kAsCgCapDefault = 500;   // Ceres' Solver::Options::max_linear_solver_iterations

enum AsKind : int { kAsPoint = 0, kAsLine = 1, kAsVp = 2 };
// association edges: point-line (R2.1), VP-line (R2.2), VP-VP orthogonality (R2.3), VP-VP collinearity (R2.4)
enum AsEdgeKind : int { kAsPL = 0, kAsVL = 1, kAsOrth = 2, kAsColl = 3 };
enum AsPhase : int { kAsHead = 0, kAsCg = 1, kAsTail = 2 };
// how the last linear solve ended
enum AsCgEnd : int { kAsCgConverged = 0, kAsCgCap = 1, kAsCgBreakdown = 2, kAsCgPivot = 3 };

// an unknown: its R1 blocks [b0, b0 + nb), its entries [a0, a0 + na) of the adjacency list (ascending edge order);
// nd = 0: constant (no parameter of the problem), else 3 / 4 / 2
struct AsUnk {
  int b0, nb, a0, na;
  int kind, nd;
  int pad_[2];
};
static_assert(sizeof(AsUnk) == 32, "AsUnk layout");

// an association edge between the unknowns a and b (point-line: a the point; VP-line: a the VP), w = the ScaledLoss weight
struct AsEdge {
  double w;
  int kind, a, b, pad_;
};
static_assert(sizeof(AsEdge) == 24, "AsEdge layout");

// the status record: §27's loop state (ba_decide_init / ba_decide_step write it) and the scalars of the linear solve
struct AsStatus {
  BaStatus lm;
  double rz, rz0, alpha, beta, eta;
  int phase;     // which kernels of a batch run: the head of an attempt, CG iterations, the tail
  int cg_it;     // iterations of the current linear solve
  int cg_cap;
  int cg_end;    // AsCgEnd of the last linear solve
  long long cg_total;  // CG iterations of the whole solve
};
static_assert(sizeof(AsStatus) == 128, "AsStatus layout");

// the tables of a solve (device or host addresses).  Unknowns in the order points, lines, VPs
struct AsDev {
  int NU, NP, NL, NV, NB, NE;
  int n_chunks, n_uchunks;  // chunks of the NB + NE blocks, of the NU unknowns
  double alpha;
  const double *kvec, *pose;  // 4 / 7 per image
  double *sp;                 // 2 sets x 6 NU (point: p[3]; line: uvec, wvec; VP: v[3])
  const AsUnk *unk;
  const BaBlk *blk;           // R1 blocks (s = the unknown)
  const AsEdge *edge;
  const int *adj;             // 2 per entry: the edge, the side (0: the unknown is the edge's a, 1: its b)
  double *lin, *elin;         // kAsLinFields x NB, kAsELinFields x NE
  double *E;                  // 16 per edge: rho' J_a^T J_b, row-major 4 x 4
  double *D;                  // 14 per unknown: the upper triangle of its diagonal block by rows, then its gradient
  double *A, *Minv;           // 16 per unknown: the damped diagonal block and its inverse
  double *x, *r, *z, *p, *Ap; // 4 per unknown
  double *xl, *rl, *Apl;      // 4 per unknown: the low parts of the pairs (x, xl), (r, rl), (Ap, Apl)
  double *chunk;              // 2 x max(n_chunks, n_uchunks)
  AsStatus *status;
};

LT_HD const double *as_sp(const AsDev &d, int set, int u) { return d.sp + ((size_t)set * d.NU + u) * 6; }
LT_HD double as_lin(const AsDev &d, int f, int b) { return d.lin[(size_t)f * d.NB + b]; }
LT_HD double as_elin(const AsDev &d, int f, int e) { return d.elin[(size_t)f * d.NE + e]; }

// ---- the chart of a vanishing point v (a unit vector): the tangent basis b1 = (v x e_k) / |v x e_k| with k the axis of
// the smallest |v_k| (the first among equals), b2 = v x b1, and the retraction normalize(v + a b1 + c b2).  sqrt and
// division only ----
LT_HD void as_vp_basis(const double v[3], double b1[3], double b2[3]) {
  const double a0 = rf_abs(v[0]), a1 = rf_abs(v[1]), a2 = rf_abs(v[2]);
  int k = 0;
  if (a1 < a0) k = 1;
  if (a2 < (k ? a1 : a0)) k = 2;
  double c[3];
  if (k == 0) { c[0] = 0.0; c[1] = v[2]; c[2] = -v[1]; }
  else if (k == 1) { c[0] = -v[2]; c[1] = 0.0; c[2] = v[0]; }
  else { c[0] = v[1]; c[1] = -v[0]; c[2] = 0.0; }
  const double n = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
  for (int i = 0; i < 3; ++i) b1[i] = c[i] / n;
  b2[0] = v[1] * b1[2] - v[2] * b1[1];
  b2[1] = v[2] * b1[0] - v[0] * b1[2];
  b2[2] = v[0] * b1[1] - v[1] * b1[0];
}
LT_HD void as_vp_retract(const double v[3], const double dl[2], double out[3]) {
  double b1[3], b2[3], t[3];
  as_vp_basis(v, b1, b2);
  for (int i = 0; i < 3; ++i) t[i] = (v[i] + dl[0] * b1[i]) + dl[1] * b2[i];
  const double n = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
  for (int i = 0; i < 3; ++i) out[i] = t[i] / n;
}
// the point a step leads to: additive, §19's chart, the chart above
LT_HD void as_retract(int kind, const double p[6], const double dl[4], double out[6]) {
  if (kind == kAsLine) {
    RfChart::retract(p, dl, out);
    return;
  }
  if (kind == kAsVp) as_vp_retract(p, dl, out);
  else
    for (int c = 0; c < 3; ++c) out[c] = p[c] + dl[c];
  for (int c = 3; c < 6; ++c) out[c] = 0.0;
}

// the parameters of an unknown as jets: constants, or with the local directions of its chart
template <int N>
LT_HD void as_const(const double p[6], Jet<N> x[6]) {
  for (int i = 0; i < 6; ++i) x[i] = Jet<N>(p[i]);
}
LT_HD void as_seed(int kind, const double p[6], Jet<4> x[6]) {
  as_const<4>(p, x);
  if (kind == kAsLine) {  // rf_seed's directions
    lm_seed_quat(p, x);
    x[4].d[3] = -p[5];
    x[5].d[3] = p[4];
  } else if (kind == kAsVp) {
    double b1[3], b2[3];
    as_vp_basis(p, b1, b2);
    for (int i = 0; i < 3; ++i) { x[i].d[0] = b1[i]; x[i].d[1] = b2[i]; }
  } else {
    for (int i = 0; i < 3; ++i) x[i].d[i] = 1.0;
  }
}

// ---- residuals ----
// ceres::CrossProduct
template <class T>
LT_HD void as_cross(const T x[3], const T y[3], T o[3]) {
  o[0] = x[1] * y[2] - x[2] * y[1];
  o[1] = x[2] * y[0] - x[0] * y[2];
  o[2] = x[0] * y[1] - x[1] * y[0];
}
// the two normalised directions of CeresComputeDist3D_sine / _cosine (line_dists.h:41-49, 61-69)
template <class T>
LT_HD void as_unit2(const T a[3], const T b[3], T an[3], T bn[3]) {
  const T n1 = rf_sqrt(((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]) + kEps);
  const T n2 = rf_sqrt(((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]) + kEps);
  for (int i = 0; i < 3; ++i) { an[i] = a[i] / n1; bn[i] = b[i] / n2; }
}
template <class T>
LT_HD T as_sine(const T a[3], const T b[3]) {
  T an[3], bn[3], c[3];
  as_unit2<T>(a, b, an, bn);
  as_cross<T>(an, bn, c);
  T s = rf_sqrt(((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]) + kEps);
  if (rf_val(s) > 1.0) rf_set(s, 1.0);
  return s;
}
template <class T>
LT_HD T as_cosine(const T a[3], const T b[3]) {
  T an[3], bn[3];
  as_unit2<T>(a, b, an, bn);
  T c = ((0.0 + an[0] * bn[0]) + an[1] * bn[1]) + an[2] * bn[2];
  c = rf_abs(c);
  if (rf_val(c) > 1.0) rf_set(c, 1.0);
  return c;
}
// the residuals of an edge (3 of a point-line edge, else 1 and two zeros) at the parameters pa, pb of its two unknowns
template <class T>
LT_HD void as_edge_res(int kind, const T pa[6], const T pb[6], T res[3]) {
  res[1] = T(0.0);
  res[2] = T(0.0);
  if (kind == kAsPL) {  // d x (d x p + m) + EPS
    T d[3], m[3], bp[3], disp[3];
    rf_plucker_c<T>(pb, pb + 4, d, m);
    as_cross<T>(d, pa, bp);
    for (int i = 0; i < 3; ++i) bp[i] = bp[i] + m[i];
    as_cross<T>(d, bp, disp);
    for (int i = 0; i < 3; ++i) res[i] = disp[i] + kEps;
  } else if (kind == kAsVL) {
    T d[3], m[3];
    rf_plucker_c<T>(pb, pb + 4, d, m);
    res[0] = as_sine<T>(d, pa);
  } else if (kind == kAsOrth) {
    res[0] = as_cosine<T>(pa, pb);
  } else {
    res[0] = as_sine<T>(pa, pb);
  }
}

// ScaledLoss over the squared norm: HuberLoss(0.01) for the two associations, TrivialLoss for the VP pairs
LT_HD double as_edge_rho(const AsEdge &e, double sq) {
  if (e.kind >= kAsOrth) return e.w * sq;
  const double b = kAsHuberA * kAsHuberA;
  return sq > b ? e.w * ((2.0 * kAsHuberA) * sqrt(sq) - b) : e.w * sq;
}
LT_HD double as_edge_rho1(const AsEdge &e, double sq) {
  if (e.kind >= kAsOrth) return e.w;
  const double b = kAsHuberA * kAsHuberA;
  return sq > b ? e.w * (kAsHuberA / sqrt(sq)) : e.w;
}
LT_HD double as_sq3(const double r[3]) { return (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]; }

LT_HD double as_edge_cost_term(const AsEdge &e, const double pa[6], const double pb[6]) {
  double r[3];
  as_edge_res<double>(e.kind, pa, pb, r);
  return as_edge_rho(e, as_sq3(r));
}

// ---- the items of the kernels; `set` selects the parameter set ----
// k_as_linearize: R1 block bi at the current point -- §27's pass over the structure with the camera a constant
LT_HD void as_item_lin_blk(const AsDev &d, int cur, int bi) {
  const BaBlk b = d.blk[bi];
  double r[2], J[2][4];
  const double *k = d.kvec + 4 * b.cam, *pose = d.pose + (size_t)7 * b.cam, *s = as_sp(d, cur, b.s);
  if (b.kind) ba_pass<4>(b, k, pose, s, d.alpha, 2, r, J);
  else ba_pass<3>(b, k, pose, s, d.alpha, 2, r, J);
  const size_t nb = (size_t)d.NB;
  double *o = d.lin + bi;
  o[0] = r[0]; o[nb] = r[1]; o[2 * nb] = ba_rho1(b, r[0] * r[0] + r[1] * r[1]);
  for (int m = 0; m < 2; ++m)
    for (int c = 0; c < 4; ++c) o[(3 + 4 * m + c) * nb] = J[m][c];
}
// k_as_linearize: edge ei -- one pass of four derivatives per free side, then its off-diagonal block rho' J_a^T J_b
LT_HD void as_item_lin_edge(const AsDev &d, int cur, int ei) {
  const AsEdge e = d.edge[ei];
  const AsUnk ua = d.unk[e.a], ub = d.unk[e.b];
  const double *pa = as_sp(d, cur, e.a), *pb = as_sp(d, cur, e.b);
  double r[3], Ja[3][4], Jb[3][4];
  for (int m = 0; m < 3; ++m)
    for (int c = 0; c < 4; ++c) Ja[m][c] = Jb[m][c] = 0.0;
  as_edge_res<double>(e.kind, pa, pb, r);
  if (ua.nd) {
    Jet<4> xa[6], xb[6], res[3];
    as_seed(ua.kind, pa, xa);
    as_const<4>(pb, xb);
    as_edge_res<Jet<4>>(e.kind, xa, xb, res);
    for (int m = 0; m < 3; ++m)
      for (int c = 0; c < 4; ++c) Ja[m][c] = res[m].d[c];
  }
  if (ub.nd) {
    Jet<4> xa[6], xb[6], res[3];
    as_const<4>(pa, xa);
    as_seed(ub.kind, pb, xb);
    as_edge_res<Jet<4>>(e.kind, xa, xb, res);
    for (int m = 0; m < 3; ++m)
      for (int c = 0; c < 4; ++c) Jb[m][c] = res[m].d[c];
  }
  const double rho1 = as_edge_rho1(e, as_sq3(r));
  const size_t ne = (size_t)d.NE;
  double *o = d.elin + ei;
  for (int m = 0; m < 3; ++m) o[m * ne] = r[m];
  o[3 * ne] = rho1;
  for (int m = 0; m < 3; ++m)
    for (int c = 0; c < 4; ++c) {
      o[(4 + 4 * m + c) * ne] = Ja[m][c];
      o[(16 + 4 * m + c) * ne] = Jb[m][c];
    }
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j)
      d.E[(size_t)16 * ei + 4 * i + j] = rho1 * ((Ja[0][i] * Jb[0][j] + Ja[1][i] * Jb[1][j]) + Ja[2][i] * Jb[2][j]);
}

// k_as_diag: lane `lane` of a point's or line's group adds its R1 blocks (lane, lane + 16, ...): §27's ba_struct_part
LT_HD void as_struct_part(const AsDev &d, const AsUnk &un, int lane, double part[kRfSums]) {
  for (int c = 0; c < kRfSums; ++c) part[c] = 0.0;
  for (int i = lane; i < un.nb; i += kAsWidth) {
    const int b = un.b0 + i;
    const double r[2] = {as_lin(d, 0, b), as_lin(d, 1, b)}, rho1 = as_lin(d, 2, b);
    double J[2][4];
    for (int c = 0; c < 4; ++c) { J[0][c] = as_lin(d, 3 + c, b); J[1][c] = as_lin(d, 7 + c, b); }
    lm_block_add<2, 4>(r, rho1, J, part);
  }
}
// entry i of the adjacency list added to the 14 sums acc: rho' J^T J (upper triangle by rows) and rho' J^T r of the
// unknown's side of the edge
LT_HD void as_adj_add(const AsDev &d, int i, double acc[kRfSums]) {
  const int e = d.adj[2 * i], f0 = d.adj[2 * i + 1] ? 16 : 4;
  const double r[3] = {as_elin(d, 0, e), as_elin(d, 1, e), as_elin(d, 2, e)}, rho1 = as_elin(d, 3, e);
  double J[3][4];
  for (int c = 0; c < 4; ++c)
    for (int m = 0; m < 3; ++m) J[m][c] = as_elin(d, f0 + 4 * m + c, e);
  lm_block_add<3, 4>(r, rho1, J, acc);
}
// k_as_diag, after the tree: the reduced R1 sums, then the unknown's edges in ascending edge order
LT_HD void as_item_diag_store(const AsDev &d, int u, double acc[kRfSums]) {
  const AsUnk un = d.unk[u];
  for (int i = un.a0; i < un.a0 + un.na; ++i) as_adj_add(d, i, acc);
  for (int c = 0; c < kRfSums; ++c) d.D[(size_t)kRfSums * u + c] = acc[c];
}
// k_as_diag_vp: lane `lane` of a vanishing point's wave adds entries lane, lane + 64, ... of its adjacency list
LT_HD void as_vp_part(const AsDev &d, const AsUnk &un, int lane, double part[kRfSums]) {
  for (int c = 0; c < kRfSums; ++c) part[c] = 0.0;
  for (int i = un.a0 + lane; i < un.a0 + un.na; i += kAsWave) as_adj_add(d, i, part);
}

// k_as_precond: the inverse of the damped diagonal block A_u (lm_inverse4), zero outside the unknown's dimensions.
// false: a pivot is not positive or not finite
LT_HD bool as_item_minv(const AsDev &d, int u) {
  double *M = d.Minv + (size_t)16 * u;
  for (int c = 0; c < 16; ++c) M[c] = 0.0;
  return lm_inverse4(d.A + (size_t)16 * u, d.unk[u].nd, M);
}
LT_HD void as_item_damp(const AsDev &d, int u, double mu) {
  const int nd = d.unk[u].nd;
  double *A = d.A + (size_t)16 * u;
  for (int c = 0; c < 16; ++c) A[c] = 0.0;
  const double *D = d.D + (size_t)kRfSums * u;
  int o = 0;
  for (int i = 0; i < 4; ++i)
    for (int j = i; j < 4; ++j, ++o)
      if (i < nd && j < nd) A[4 * i + j] = A[4 * j + i] = i == j ? lm_damp(D[o], mu) : D[o];
}
// ---- the pairs of the linear solve.  x, r and A p are carried as unevaluated sums hi + lo of two doubles: the rounding
// of r -= alpha A p while r is still of the size of the right-hand side, and that of the products of A p, otherwise
// stay in the step along the weak directions of a diagonal block.  Error-free transformations from IEEE
// additions and multiplications alone (Knuth's TwoSum, Dekker's TwoProduct by Veltkamp's split): no fused operation, so
// -ffp-contract=off keeps them exact on both sides ----
LT_HD void as_two_sum(double a, double b, double *s, double *e) {
  const double t = a + b, bb = t - a;
  *e = (a - (t - bb)) + (b - bb);
  *s = t;
}
LT_HD void as_split(double a, double *hi, double *lo) {
  const double c = 134217729.0 * a;  // 2^27 + 1
  *hi = c - (c - a);
  *lo = a - *hi;
}
LT_HD void as_two_prod(double a, double b, double *p, double *e) {
  double ah, al, bh, bl;
  const double t = a * b;
  as_split(a, &ah, &al);
  as_split(b, &bh, &bl);
  *e = (((ah * bh - t) + ah * bl) + al * bh) + al * bl;
  *p = t;
}
// (h, l) += a b: the product and the sum exact, their errors collected in l
LT_HD void as_dd_acc(double *h, double *l, double a, double b) {
  double p, e, s, t;
  as_two_prod(a, b, &p, &e);
  as_two_sum(*h, p, &s, &t);
  *l = *l + (t + e);
  *h = s;
}
LT_HD void as_dd_norm(double *h, double *l) {
  const double s = *h + *l;
  *l = *l - (s - *h);
  *h = s;
}

// out = M v over the 4 slots of an unknown, every row from 0.0 in ascending column order
LT_HD void as_mul4(const double *M, const double *v, double out[4]) {
  for (int i = 0; i < 4; ++i) {
    double s = 0.0;
    for (int j = 0; j < 4; ++j) s = s + M[4 * i + j] * v[j];
    out[i] = s;
  }
}
LT_HD double as_dot4(const double *a, const double *b) {
  double s = 0.0;
  for (int j = 0; j < 4; ++j) s = s + a[j] * b[j];
  return s;
}
// the start of a linear solve at unknown u: x = 0, r = -g, z = M^-1 r, p = z; returns r . z.  ok = false: a bad pivot
// (z = 0).  nz: a gradient entry of a free unknown is not zero
LT_HD double as_item_cg_start(const AsDev &d, int u, bool *ok, bool *nz) {
  const int nd = d.unk[u].nd;
  const size_t o = (size_t)4 * u;
  *ok = as_item_minv(d, u);
  double r[4], z[4];
  for (int i = 0; i < 4; ++i) {
    r[i] = i < nd ? -d.D[(size_t)kRfSums * u + 10 + i] : 0.0;
    if (r[i] != 0.0) *nz = true;
  }
  as_mul4(d.Minv + 4 * o, r, z);
  for (int i = 0; i < 4; ++i) {
    if (!*ok) z[i] = 0.0;
    d.x[o + i] = 0.0; d.r[o + i] = r[i]; d.z[o + i] = z[i]; d.p[o + i] = z[i]; d.Ap[o + i] = 0.0;
    d.xl[o + i] = 0.0; d.rl[o + i] = 0.0; d.Apl[o + i] = 0.0;
  }
  return as_dot4(r, z);
}
// k_as_matvec: Ap_u = A_u p_u, then the unknown's edges in ascending edge order, every row one pair that takes its
// products in that order; returns p_u . Ap_u (the high parts)
LT_HD double as_item_matvec(const AsDev &d, int u) {
  const AsUnk un = d.unk[u];
  const size_t o = (size_t)4 * u;
  double ah[4] = {0.0, 0.0, 0.0, 0.0}, al[4] = {0.0, 0.0, 0.0, 0.0};
  if (un.nd) {
    const double *A = d.A + 4 * o, *pu = d.p + o;
    for (int j = 0; j < 4; ++j)
      for (int r = 0; r < 4; ++r) as_dd_acc(&ah[r], &al[r], A[4 * r + j], pu[j]);
    for (int i = un.a0; i < un.a0 + un.na; ++i) {
      const int e = d.adj[2 * i], side = d.adj[2 * i + 1];
      const double *E = d.E + (size_t)16 * e;
      const double *q = d.p + (size_t)4 * (side ? d.edge[e].a : d.edge[e].b);
      for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 4; ++r) as_dd_acc(&ah[r], &al[r], side ? E[4 * c + r] : E[4 * r + c], q[c]);
    }
    for (int r = 0; r < 4; ++r) as_dd_norm(&ah[r], &al[r]);
  }
  for (int i = 0; i < 4; ++i) { d.Ap[o + i] = ah[i]; d.Apl[o + i] = al[i]; }
  return as_dot4(d.p + o, ah);
}
// k_as_update: x += alpha p, r -= alpha Ap on the pairs, z = M^-1 r; returns r . z (the high parts)
LT_HD double as_item_update(const AsDev &d, int u, double alpha) {
  const size_t o = (size_t)4 * u;
  double r[4], z[4];
  for (int i = 0; i < 4; ++i) {
    double h = d.x[o + i], l = d.xl[o + i];
    as_dd_acc(&h, &l, alpha, d.p[o + i]);
    as_dd_norm(&h, &l);
    d.x[o + i] = h; d.xl[o + i] = l;
    h = d.r[o + i]; l = d.rl[o + i];
    as_dd_acc(&h, &l, -alpha, d.Ap[o + i]);
    double s, t;
    as_two_sum(h, (-alpha) * d.Apl[o + i], &s, &t);
    h = s; l = l + t;
    as_dd_norm(&h, &l);
    d.r[o + i] = h; d.rl[o + i] = l;
    r[i] = h;
  }
  as_mul4(d.Minv + 4 * o, r, z);
  for (int i = 0; i < 4; ++i) d.z[o + i] = z[i];
  return as_dot4(r, z);
}
// k_as_dir: p = z + beta p
LT_HD void as_item_dir(const AsDev &d, int u, double beta) {
  const size_t o = (size_t)4 * u;
  for (int i = 0; i < 4; ++i) d.p[o + i] = d.z[o + i] + beta * d.p[o + i];
}

// the one-wave decisions of a linear solve, on the reduced totals
// k_as_cg_begin: after k_as_precond.  total = r0 . z0, nz = a gradient entry is not zero
LT_HD void as_decide_begin(AsStatus &st, double total, bool nz) {
  if (st.lm.bad) { st.cg_end = kAsCgPivot; st.phase = kAsTail; return; }
  if (st.lm.fresh && !nz) { st.lm.code = kRfZeroGrad; st.lm.done = 1; return; }
  st.cg_it = 0;
  st.rz = st.rz0 = total;
  if (!(total > 0.0) || !(total < kMaxDist)) { st.lm.bad = 1; st.cg_end = kAsCgBreakdown; st.phase = kAsTail; return; }
  st.phase = kAsCg;
}
// k_as_alpha: total = p . Ap
LT_HD void as_decide_alpha(AsStatus &st, double total) {
  if (!(total > 0.0) || !(total < kMaxDist)) { st.lm.bad = 1; st.cg_end = kAsCgBreakdown; st.phase = kAsTail; return; }
  st.alpha = st.rz / total;
}
// k_as_beta: total = r . z after the update
LT_HD void as_decide_beta(AsStatus &st, double total) {
  const double prev = st.rz;
  st.cg_it += 1;
  st.cg_total += 1;
  st.rz = total;
  if (sqrt(total) <= st.eta * sqrt(st.rz0)) { st.cg_end = kAsCgConverged; st.phase = kAsTail; return; }
  if (st.cg_it >= st.cg_cap) { st.cg_end = kAsCgCap; st.phase = kAsTail; return; }
  st.beta = total / prev;
}

// k_as_backsub: the candidate parameters of unknown u in the other set, from the step x
LT_HD void as_item_backsub(const AsDev &d, int cur, int u) {
  const AsUnk un = d.unk[u];
  const double *p = as_sp(d, cur, u);
  double *out = d.sp + ((size_t)(1 - cur) * d.NU + u) * 6;
  if (!un.nd) {
    for (int c = 0; c < 6; ++c) out[c] = p[c];
    return;
  }
  as_retract(un.kind, p, d.x + (size_t)4 * u, out);
}
// k_as_cost: term i of the cost at parameter set `set` (i < NB: an R1 block, else edge i - NB); with md its term of the
// model decrease rho' ((J d) . r + |J d|^2 / 2) from the linearisation and the step
LT_HD void as_item_cost(const AsDev &d, int set, int i, bool with_md, double *cost, double *md) {
  *md = 0.0;
  if (i < d.NB) {
    const BaBlk b = d.blk[i];
    *cost = ba_cost_term(b, d.kvec + 4 * b.cam, d.pose + (size_t)7 * b.cam, as_sp(d, set, b.s), d.alpha);
    if (with_md) {
      const double *dl = d.x + (size_t)4 * b.s;
      double jd[2];
      for (int m = 0; m < 2; ++m) {
        double sum = 0.0;
        for (int l = 0; l < 4; ++l) sum = sum + as_lin(d, 3 + 4 * m + l, i) * dl[l];
        jd[m] = sum;
      }
      const double r[2] = {as_lin(d, 0, i), as_lin(d, 1, i)};
      *md = lm_model_term<2>(jd, r, as_lin(d, 2, i));
    }
    return;
  }
  const int ei = i - d.NB;
  const AsEdge e = d.edge[ei];
  *cost = as_edge_cost_term(e, as_sp(d, set, e.a), as_sp(d, set, e.b));
  if (with_md) {
    const double *da = d.x + (size_t)4 * e.a, *db = d.x + (size_t)4 * e.b;
    double jd[3];
    for (int m = 0; m < 3; ++m) {
      double sum = 0.0;
      for (int l = 0; l < 4; ++l) sum = sum + as_elin(d, 4 + 4 * m + l, ei) * da[l];
      for (int l = 0; l < 4; ++l) sum = sum + as_elin(d, 16 + 4 * m + l, ei) * db[l];
      jd[m] = sum;
    }
    const double r[3] = {as_elin(d, 0, ei), as_elin(d, 1, ei), as_elin(d, 2, ei)};
    *md = lm_model_term<3>(jd, r, as_elin(d, 3, ei));
  }
}

// the launches of lt_kernels_assoc.hip; every kernel reads the status record and returns at once when its phase has
// ended.  ev: as_events(cg_batch) + 1 events around the kernels, or null
constexpr int kAsHeadKernels = 5, kAsCgKernels = 5, kAsTailKernels = 3;
constexpr int as_events(int cg_batch) { return kAsHeadKernels + kAsCgKernels * cg_batch + kAsTailKernels; }
void launch_as_init(hipStream_t st, const AsDev &dev);  // the cost at the initial point, then k_as_decide's first call
void launch_as_attempt(hipStream_t st, const AsDev &dev, int cg_batch, hipEvent_t *ev);

}  // namespace lt
