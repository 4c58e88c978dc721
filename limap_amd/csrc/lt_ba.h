// lt_ba.h -- records and the FP64 expressions shared by the host side (lt_ba.cpp) and the device side
// (lt_kernels_ba.hip) of the bundle adjustment with free poses, points and lines: limap.optimize's
// solve_hybrid_bundle_adjustment / solve_point_bundle_adjustment.  Intrinsics are constant.  Both sides
// compile the same inline functions with -ffp-contract=off and reduce in the same fixed orders, so the device and
// lt_fn_ba_host agree bit for bit.
//
// limap's own part is restated in its operation order, the pose a variable of every block: paths relative to src/limap,
//   optimize/hybrid_bundle_adjustment/cost_functions.h:28-85          PointGeometricRefinementFunctor
//   optimize/hybrid_bundle_adjustment/hybrid_bundle_adjustment.cc:61-123   ParameterizeCameras / Points / Lines
//   optimize/hybrid_bundle_adjustment/hybrid_bundle_adjustment.cc:125-197  AddPointGeometricResiduals (tracks in ascending
//                                        id, observations in list order, ScaledLoss(TrivialLoss, lw_point)),
//                                        AddLineGeometricResiduals (sorted images, then list order: §19's make_plan;
//                                        ScaledLoss(CauchyLoss(0.25), length / 30))
//   optimize/hybrid_bundle_adjustment/hybrid_bundle_adjustment.cc:199-264  SetUp (R1.1, R1.2), Solve
//   ceresbase/point_projection.h:8-57    ImgFromCam, WorldToPixel (Ceres' QuaternionRotatePoint, two divisions by the depth)
//   ceresbase/line_transforms.h:8-29     MinimalPluckerToPlucker
//   ceresbase/line_projection.h:14-80    Line_ImgFromCam, Line_WorldToPixel: R [m]x R^T - t (R d)^T + (R d) t^T with
//                                        R = Ceres' QuaternionToRotation(qvec), then K [m']x K^T -- the products of
//                                        rf_w2p (lt_refine.h), here with R and t carrying derivatives; not §19's
//                                        precomputed 3x6 view matrix, which assumed a constant camera
//   optimize/line_refinement/cost_functions.h:96-127   Ceres_CosineWeightedPerpendicularDist2D_1D (rf_residual's tail)
// ASSUMPTIONS as in lt_refine.h and lt_loc.h (Ceres and Eigen are not part of limap): QuaternionRotatePoint,
// QuaternionToRotation, TrivialLoss, CauchyLoss, ScaledLoss, the Jet rules d|x|/dx = +1 at 0 and derivative 0 at the
// clamp.  The minimiser is this project's own definition: §19's Levenberg-Marquardt loop over all unknowns
// at once, its linear step by a Schur complement and a dense Cholesky factorisation in a fixed order.
#pragma once

#include "lt_loc.h"

namespace lt {

constexpr int kBaMaxImages = 128;    // LT_BA_MAX_IMAGES: images that carry residuals (k_ba_chol keeps two vectors of 6 x 128 doubles in LDS)
constexpr int kBaWidth = 16;         // lanes per structure track of k_ba_blocks (§19's group)
constexpr int kBaWave = kLmWave;     // lanes per image of k_ba_images, per chunk of k_ba_cost, of k_ba_decide
constexpr int kBaChunk = kLmChunk;   // residual blocks per chunk of the cost reduction (lm_chunks_host, lm_chunk_sums)
constexpr int kBaCholThreads = 1024; // lanes of the one workgroup of k_ba_chol
static_assert(6 * kBaMaxImages <= kBaCholThreads, "k_ba_chol gives every row of S a lane of its own");
constexpr int kBaLinFields = 23;     // doubles per block of a linearisation (SoA): r[2], rho', J_cam[2][6], J_struct[2][4]
constexpr int kBaPollDefault = 8;    // attempts enqueued between two reads of the status record
static_assert(kRfSums == 14 && kLcSums == 27 && kLcWidth == kBaWave, "the sums of a structure and of an image");

// a structure track: point (3 unknowns) or line (4); blocks [b0, b0 + nb), its (track, image) pairs [p0, p0 + np)
struct BaStruct {
  int b0, nb, p0, np;
  int kind, constant;  // kind 0 point, 1 line
  int pad_[2];
};
static_assert(sizeof(BaStruct) == 32, "BaStruct layout");

// a residual block: its observation (point: x y; line: x1 y1 x2 y2), ScaledLoss weight, image row, structure, pair
struct BaBlk {
  double o[4], w;
  int cam, s, pair, kind;
};
static_assert(sizeof(BaBlk) == 56, "BaBlk layout");

// the status record of a solve: written by k_ba_decide (and `bad` / the zero-gradient end by the solve kernels), read by
// every kernel
struct BaStatus {
  double mu, nu, F, F0;
  int cur;       // which parameter set is current
  int fresh;     // the current point has no linearisation yet
  int done, code, iters;
  int bad;       // the attempt's factorisation failed: a rejected step
  int max_iter, attempts;
};
static_assert(sizeof(BaStatus) == 64, "BaStatus layout");

// the tables of a solve (device or host addresses)
struct BaDev {
  int C, NS, NB, NPair, n, n_chunks;  // images, structures, blocks, pairs, 6 C, chunks
  double alpha;
  const double *kvec;  // 4 per image
  double *pose;        // 2 sets x 7 C (q, t)
  double *sp;          // 2 sets x 6 NS (point: p[3]; line: uvec, wvec)
  const BaStruct *st;
  const BaBlk *blk;
  const int *pair_cam, *pair_s;          // per pair, pairs ordered by (structure, image)
  const int *pair_blk_off, *pair_blk;    // CSR: the blocks of a pair in residual order
  const int *cam_blk_off, *cam_blk;      // CSR: the blocks of an image in ascending order
  const int *sch_off, *sch;              // CSR over the image pairs (i, j <= i), row i (i + 1) / 2 + j: the couples (p, q)
                                         // of pairs of the free structures that see both, p in image i, q in image j,
                                         // in ascending structure order
  double *lin;                           // kBaLinFields x NB
  double *V, *bs, *W, *U, *g, *Vinv, *Y; // 10, 4, 24, 21, 6, 16, 24 doubles per structure / pair / image; Y = W V^-1
  double *S, *LT, *rhs, *dc, *ds;        // n x n (rows), n x n (LT[k n + i] = L_ik), n, n, 4 NS
  double *chunk;                         // 2 x n_chunks: cost terms, model terms
  BaStatus *status;
};

// PointGeometricRefinementFunctor::operator() (cost_functions.h:65-78): WorldToPixel, then the difference
template <class T>
LT_HD void ba_point_res(const double k[4], const T q[4], const T t[3], const T X[3], const double o[4], T res[2]) {
  T r[3];
  lm_rotate<T, T>(q, X, r);
  const T p2 = r[2] + t[2];
  const T u = (r[0] + t[0]) / p2, v = (r[1] + t[1]) / p2;
  res[0] = (k[0] * u + k[2]) - o[0];
  res[1] = (k[1] * v + k[3]) - o[1];
}

// GeometricRefinementFunctor::operator() with the pose as a variable (line_refinement/cost_functions.h:129-178):
// MinimalPluckerToPlucker, Line_WorldToPixel, Ceres_CosineWeightedPerpendicularDist2D_1D (rf_residual's expressions
// after the projection, with §19's Jet rules and every EPS)
template <class T>
LT_HD void ba_line_res(const double k[4], const T q[4], const T t[3], const T u[4], const T w[2], const double o[4],
                       double alpha, T res[2]) {
  T d[3], m[3], c[3];
  rf_plucker_c<T>(u, w, d, m);
  const T a = q[0], b = q[1], cq = q[2], e = q[3];
  const T aa = a * a, ab = a * b, ac = a * cq, ae = a * e, bb = b * b, bc = b * cq, be = b * e, cc = cq * cq, ce = cq * e,
          ee = e * e;
  const T n = rf_inv(((aa + bb) + cc) + ee);
  const T R[9] = {(((aa + bb) - cc) - ee) * n, (2.0 * (bc - ae)) * n, (2.0 * (ac + be)) * n,
                  (2.0 * (ae + bc)) * n, (((aa - bb) + cc) - ee) * n, (2.0 * (ce - ab)) * n,
                  (2.0 * (be - ac)) * n, (2.0 * (ab + ce)) * n, (((aa - bb) - cc) + ee) * n};
  lm_w2p<T, T>(k, R, t, d, m, c);  // R and t carry derivatives
  const T c0 = c[0], c1 = c[1], c2 = c[2];
  const T dn = rf_sqrt((c0 * c0 + c1 * c1) + kEps);
  const T e0 = -(c1 / dn), e1 = c0 / dn;
  const double f0 = o[2] - o[0], f1 = o[3] - o[1];
  const T n1 = rf_sqrt((e0 * e0 + e1 * e1) + kEps);
  const double n2 = sqrt((f0 * f0 + f1 * f1) + kEps);
  T cosine = rf_abs((e0 * f0 + e1 * f1) / (n1 * n2));
  if (rf_val(cosine) > 1.0) rf_set(cosine, 1.0);
  const T wgt = rf_exp((1.0 - cosine) * alpha);
  res[0] = (((c0 * o[0] + c1 * o[1]) + c2) / dn) * wgt;
  res[1] = (((c0 * o[2] + c1 * o[3]) + c2) / dn) * wgt;
}

// the residuals of a block with the pose p = (q, t) and the structure's parameters sp; T = double or a jet
template <class T>
LT_HD void ba_res(const BaBlk &b, const double k[4], const T q[4], const T t[3], const T s[6], double alpha, T res[2]) {
  if (b.kind) ba_line_res<T>(k, q, t, s, s + 4, b.o, alpha, res);
  else ba_point_res<T>(k, q, t, s, b.o, res);
}

// ScaledLoss over the squared norm: points TrivialLoss, lines CauchyLoss(0.25)
LT_HD double ba_rho(const BaBlk &b, double sq) { return b.kind ? rf_rho(b.w, sq) : b.w * sq; }
LT_HD double ba_rho1(const BaBlk &b, double sq) { return b.kind ? rf_rho1(b.w, sq) : b.w; }

LT_HD double ba_cost_term(const BaBlk &b, const double k[4], const double p[7], const double s[6], double alpha) {
  double r[2];
  ba_res<double>(b, k, p, p + 4, s, alpha, r);
  return ba_rho(b, r[0] * r[0] + r[1] * r[1]);
}

// one pass of the chain with N derivatives: which = 0 rotation, 1 translation, 2 structure
template <int N>
LT_HD void ba_pass(const BaBlk &b, const double k[4], const double p[7], const double s[6], double alpha, int which,
                   double r[2], double J[2][4]) {
  typedef Jet<N> T;
  T q[4], t[3], x[6], res[2];
  for (int i = 0; i < 4; ++i) q[i] = T(p[i]);
  for (int i = 0; i < 3; ++i) t[i] = T(p[4 + i]);
  for (int i = 0; i < 6; ++i) x[i] = T(s[i]);
  if (which == 0) {
    lm_seed_quat(p, q);
  } else if (which == 1) {
    for (int i = 0; i < 3; ++i) t[i].d[i] = 1.0;
  } else if (b.kind) {  // rf_seed's directions
    lm_seed_quat(s, x);
    x[4].d[N - 1] = -s[5];
    x[5].d[N - 1] = s[4];
  } else {
    for (int i = 0; i < 3; ++i) x[i].d[i] = 1.0;
  }
  ba_res<T>(b, k, q, t, x, alpha, res);
  for (int m = 0; m < 2; ++m) {
    r[m] = res[m].v;
    for (int c = 0; c < 4; ++c) J[m][c] = c < N ? res[m].d[c < N ? c : 0] : 0.0;
  }
}

// the linearisation of a block: residuals, rho', the 2 x 6 Jacobian of its image's (dq, dt) and the 2 x 3 / 2 x 4
// Jacobian of its structure (a point's fourth column is 0), by passes of three or four derivatives
LT_HD void ba_linearise(const BaBlk &b, const double k[4], const double p[7], const double s[6], double alpha, double r[2],
                        double *rho1, double Jc[2][6], double Js[2][4]) {
  double J[2][4];
  ba_pass<3>(b, k, p, s, alpha, 0, r, J);
  for (int m = 0; m < 2; ++m)
    for (int c = 0; c < 3; ++c) Jc[m][c] = J[m][c];
  ba_pass<3>(b, k, p, s, alpha, 1, r, J);
  for (int m = 0; m < 2; ++m)
    for (int c = 0; c < 3; ++c) Jc[m][3 + c] = J[m][c];
  if (b.kind) ba_pass<4>(b, k, p, s, alpha, 2, r, Js);
  else ba_pass<3>(b, k, p, s, alpha, 2, r, Js);
  *rho1 = ba_rho1(b, r[0] * r[0] + r[1] * r[1]);
}

// ---- the items of the kernels; `set` selects the parameter set ----
LT_HD const double *ba_pose(const BaDev &d, int set, int c) { return d.pose + ((size_t)set * d.C + c) * 7; }
LT_HD const double *ba_sp(const BaDev &d, int set, int s) { return d.sp + ((size_t)set * d.NS + s) * 6; }
LT_HD double ba_lin(const BaDev &d, int f, int b) { return d.lin[(size_t)f * d.NB + b]; }

// k_ba_linearize: block bi at the current point
LT_HD void ba_item_linearise(const BaDev &d, int cur, int bi) {
  const BaBlk b = d.blk[bi];
  double r[2], rho1, Jc[2][6], Js[2][4];
  ba_linearise(b, d.kvec + 4 * b.cam, ba_pose(d, cur, b.cam), ba_sp(d, cur, b.s), d.alpha, r, &rho1, Jc, Js);
  const size_t nb = (size_t)d.NB;
  double *o = d.lin + bi;
  o[0] = r[0]; o[nb] = r[1]; o[2 * nb] = rho1;
  for (int m = 0; m < 2; ++m) {
    for (int c = 0; c < 6; ++c) o[(3 + 6 * m + c) * nb] = Jc[m][c];
    for (int c = 0; c < 4; ++c) o[(15 + 4 * m + c) * nb] = Js[m][c];
  }
}

// k_ba_blocks: lane `lane` of structure s adds its blocks (lane, lane + 16, ...) to part: V upper triangle, then b
LT_HD void ba_struct_part(const BaDev &d, const BaStruct &st, int lane, double part[kRfSums]) {
  for (int c = 0; c < kRfSums; ++c) part[c] = 0.0;
  for (int i = lane; i < st.nb; i += kBaWidth) {
    const int b = st.b0 + i;
    const double r[2] = {ba_lin(d, 0, b), ba_lin(d, 1, b)}, rho1 = ba_lin(d, 2, b);
    double J[2][4];
    for (int c = 0; c < 4; ++c) { J[0][c] = ba_lin(d, 15 + c, b); J[1][c] = ba_lin(d, 19 + c, b); }
    lm_block_add<2, 4>(r, rho1, J, part);
  }
}
// W of pair p (6 x 4, row-major): its blocks in residual order, from 0.0
LT_HD void ba_pair_W(const BaDev &d, int p) {
  double W[24];
  for (int c = 0; c < 24; ++c) W[c] = 0.0;
  for (int i = d.pair_blk_off[p]; i < d.pair_blk_off[p + 1]; ++i) {
    const int b = d.pair_blk[i];
    const double rho1 = ba_lin(d, 2, b);
    for (int a = 0; a < 6; ++a) {
      const double c0 = ba_lin(d, 3 + a, b), c1 = ba_lin(d, 9 + a, b);
      for (int l = 0; l < 4; ++l) W[4 * a + l] = W[4 * a + l] + rho1 * (c0 * ba_lin(d, 15 + l, b) + c1 * ba_lin(d, 19 + l, b));
    }
  }
  for (int c = 0; c < 24; ++c) d.W[(size_t)24 * p + c] = W[c];
}
// k_ba_images: lane `lane` of image c adds entries lane, lane + 64, ... of the image's block list: U upper triangle, g
LT_HD void ba_cam_part(const BaDev &d, int c, int lane, double part[kLcSums]) {
  for (int x = 0; x < kLcSums; ++x) part[x] = 0.0;
  for (int i = d.cam_blk_off[c] + lane; i < d.cam_blk_off[c + 1]; i += kBaWave) {
    const int b = d.cam_blk[i];
    const double r[2] = {ba_lin(d, 0, b), ba_lin(d, 1, b)}, rho1 = ba_lin(d, 2, b);
    double J[2][6];
    for (int x = 0; x < 6; ++x) { J[0][x] = ba_lin(d, 3 + x, b); J[1][x] = ba_lin(d, 9 + x, b); }
    lm_block_add<2, 6>(r, rho1, J, part);
  }
}

// k_ba_damp: V_s^{-1} of the damped block (lm_inverse4).  false: a pivot is not positive or not finite
LT_HD bool ba_item_vinv(const BaDev &d, int s, double mu) {
  const BaStruct st = d.st[s];
  if (st.constant) return true;
  const int nd = st.kind ? 4 : 3;
  double H[16];  // the lower triangle of V_s, its diagonal damped
  int o = 0;
  for (int i = 0; i < 4; ++i)
    for (int j = i; j < 4; ++j, ++o) H[4 * j + i] = d.V[(size_t)10 * s + o];
  for (int i = 0; i < nd; ++i) H[5 * i] = lm_damp(H[5 * i], mu);
  if (!lm_inverse4(H, nd, d.Vinv + (size_t)16 * s)) return false;
  // Y = W_p V_s^{-1} (6 x 4; a point's fourth column is 0) of the structure's pairs
  for (int p = st.p0; p < st.p0 + st.np; ++p)
    for (int e = 0; e < 24; ++e) {
      double sum = 0.0;
      if (e % 4 < nd)
        for (int m = 0; m < nd; ++m) sum = sum + d.W[(size_t)24 * p + 4 * (e / 4) + m] * d.Vinv[(size_t)16 * s + 4 * m + e % 4];
      d.Y[(size_t)24 * p + e] = sum;
    }
  return true;
}

// k_ba_schur: entry e of the image pair (i, j <= i).  e < 36: S(6 i + a, 6 j + b), a = e / 6, b = e % 6 -- the sum of
// (Y_p W_q^T)(a, b) over the pair's couples in ascending structure order from 0.0, every product summed over the four
// columns (a point's fourth column is 0 in Y and in W), then U_i[i == j] damped minus the sum.  36 <= e < 42 on the
// diagonal (i == j): rhs(6 i + a), a = e - 36: -g + the sum of (Y_p b_s)(a) over the same couples
LT_HD void ba_item_schur(const BaDev &d, int i, int j, int e, double mu) {
  const int blk = (i * (i + 1)) / 2 + j, c0 = d.sch_off[blk], c1 = d.sch_off[blk + 1];
  double acc = 0.0;
  if (e < 36) {
    const int a = e / 6, b = e % 6;
    for (int c = c0; c < c1; ++c) {
      const double *Y = d.Y + (size_t)24 * d.sch[2 * c] + 4 * a, *W = d.W + (size_t)24 * d.sch[2 * c + 1] + 4 * b;
      double sum = 0.0;
      for (int l = 0; l < 4; ++l) sum = sum + Y[l] * W[l];
      acc = acc + sum;
    }
    double u = 0.0;
    if (i == j) {
      const int x = a < b ? a : b, y = a < b ? b : a;
      u = d.U[(size_t)21 * i + (x * 6 - (x * (x - 1)) / 2) + (y - x)];
      if (a == b) u = lm_damp(u, mu);
    }
    d.S[(size_t)(6 * i + a) * d.n + 6 * j + b] = u - acc;
  } else if (i == j) {
    const int a = e - 36;
    for (int c = c0; c < c1; ++c) {
      const int p = d.sch[2 * c];
      const double *Y = d.Y + (size_t)24 * p + 4 * a, *bs = d.bs + (size_t)4 * d.pair_s[p];
      double sum = 0.0;
      for (int l = 0; l < 4; ++l) sum = sum + Y[l] * bs[l];
      acc = acc + sum;
    }
    d.rhs[6 * i + a] = (-d.g[6 * i + a]) + acc;
  }
}
// k_ba_backsub: the step of structure s, ds = V^{-1} (-b - sum_c W^T dc) over its images in ascending order, and its
// candidate parameters in the other set
LT_HD void ba_item_backsub_struct(const BaDev &d, int cur, int s) {
  const BaStruct st = d.st[s];
  const double *p = ba_sp(d, cur, s);
  double *out = d.sp + ((size_t)(1 - cur) * d.NS + s) * 6;
  double dl[4] = {0.0, 0.0, 0.0, 0.0};
  if (!st.constant) {
    const int nd = st.kind ? 4 : 3;
    double tmp[4];
    for (int l = 0; l < nd; ++l) tmp[l] = -d.bs[(size_t)4 * s + l];
    for (int q = st.p0; q < st.p0 + st.np; ++q) {
      const double *dc = d.dc + 6 * d.pair_cam[q];
      for (int l = 0; l < nd; ++l) {
        double acc = 0.0;
        for (int a = 0; a < 6; ++a) acc = acc + d.W[(size_t)24 * q + 4 * a + l] * dc[a];
        tmp[l] = tmp[l] - acc;
      }
    }
    for (int l = 0; l < nd; ++l) {
      double sum = 0.0;
      for (int m = 0; m < nd; ++m) sum = sum + d.Vinv[(size_t)16 * s + 4 * l + m] * tmp[m];
      dl[l] = sum;
    }
  }
  for (int l = 0; l < 4; ++l) d.ds[(size_t)4 * s + l] = dl[l];
  if (st.constant) {
    for (int c = 0; c < 6; ++c) out[c] = p[c];
  } else if (st.kind) {
    RfChart::retract(p, dl, out);
  } else {
    for (int c = 0; c < 3; ++c) out[c] = p[c] + dl[c];
    for (int c = 3; c < 6; ++c) out[c] = 0.0;
  }
}
LT_HD void ba_item_backsub_cam(const BaDev &d, int cur, int c) {
  LcChart::retract(ba_pose(d, cur, c), d.dc + 6 * c, d.pose + ((size_t)(1 - cur) * d.C + c) * 7);
}

// k_ba_cost: block bi's term of the cost at parameter set `set`; with md its term of the model decrease
// rho' ((J d) . r + |J d|^2 / 2) from the linearisation and the step
LT_HD void ba_item_cost(const BaDev &d, int set, int bi, bool with_md, double *cost, double *md) {
  const BaBlk b = d.blk[bi];
  *cost = ba_cost_term(b, d.kvec + 4 * b.cam, ba_pose(d, set, b.cam), ba_sp(d, set, b.s), d.alpha);
  *md = 0.0;
  if (with_md) {
    const double *dc = d.dc + 6 * b.cam, *dsv = d.ds + (size_t)4 * b.s;
    double jd[2];
    for (int m = 0; m < 2; ++m) {
      double sum = 0.0;
      for (int a = 0; a < 6; ++a) sum = sum + ba_lin(d, 3 + 6 * m + a, bi) * dc[a];
      for (int l = 0; l < 4; ++l) sum = sum + ba_lin(d, 15 + 4 * m + l, bi) * dsv[l];
      jd[m] = sum;
    }
    const double r[2] = {ba_lin(d, 0, bi), ba_lin(d, 1, bi)};
    *md = lm_model_term<2>(jd, r, ba_lin(d, 2, bi));
  }
}

// k_ba_decide after the cost at the initial point (total: the sum of the blocks' terms)
LT_HD void ba_decide_init(BaStatus &st, double total) {
  const double F = 0.5 * total;
  st.F = st.F0 = F;
  st.mu = kRfMu0;
  st.nu = 2.0;
  st.cur = 0;
  st.fresh = 1;
  st.iters = 0;
  st.bad = 0;
  st.attempts = 0;
  st.done = 0;
  st.code = kRfMaxIter;
  if (!(F <= kMaxDist)) { st.done = 1; st.code = kRfEvalFailed; }
  else if (st.max_iter <= 0) st.done = 1;
}
// k_ba_decide after an attempt: the ratio test, the radius, the iteration count and the end of the solve.  A failed
// factorisation (st.bad) or a model decrease that is not positive and finite is a rejected step
LT_HD void ba_decide_step(BaStatus &st, double total, double md_total) {
  const double Fn = 0.5 * total, md = -md_total;
  bool accept = false;
  double ratio = 0.0;
  if (!st.bad && md > 0.0 && md < kMaxDist) {
    ratio = (st.F - Fn) / md;
    accept = ratio > kRfMinRatio;
  }
  st.attempts += 1;
  st.iters += 1;
  st.bad = 0;
  if (accept) {
    st.cur = 1 - st.cur;
    st.F = Fn;
    st.mu = rf_grow(st.mu, ratio);
    st.nu = 2.0;
    st.fresh = 1;
  } else {
    st.fresh = 0;
    st.mu = st.mu / st.nu;
    st.nu = 2.0 * st.nu;
    if (st.mu < kRfMuMin) { st.done = 1; st.code = kRfRadius; return; }
  }
  if (st.iters >= st.max_iter) { st.done = 1; st.code = kRfMaxIter; }
}

// the defined Cholesky solve on the host (lt_fn_ba_cholesky, the host twin of k_ba_chol): S by rows (its lower
// triangle is read), LT[k n + i] = L_ik.  L_ij = (S_ij - sum_{k<j} L_ik L_jk) / L_jj with the sum in ascending k from
// S_ij; the substitutions under the same rule.  false: a pivot is not positive or not finite
inline bool ba_cholesky_host(int n, const double *S, const double *rhs, double *LT, double *x) {
  for (int j = 0; j < n; ++j)
    for (int i = j; i < n; ++i) {
      double sum = S[(size_t)i * n + j];
      for (int k = 0; k < j; ++k) sum = sum - LT[(size_t)k * n + i] * LT[(size_t)k * n + j];
      if (i == j) {
        if (!lm_pivot_ok(sum)) return false;
        LT[(size_t)j * n + j] = sqrt(sum);
      } else {
        LT[(size_t)j * n + i] = sum / LT[(size_t)j * n + j];
      }
    }
  if (!rhs || !x) return true;
  for (int i = 0; i < n; ++i) {
    double sum = rhs[i];
    for (int k = 0; k < i; ++k) sum = sum - LT[(size_t)k * n + i] * x[k];
    x[i] = sum / LT[(size_t)i * n + i];
  }
  for (int i = n - 1; i >= 0; --i) {
    double sum = x[i];
    for (int k = i + 1; k < n; ++k) sum = sum - LT[(size_t)i * n + k] * x[k];
    x[i] = sum / LT[(size_t)i * n + i];
  }
  return true;
}

// ---- constant poses (constant_pose = 1): the tracks separate.  The line side is §19's (lt_refine); every point track is
// its own 3-unknown problem under §19's loop -- its own radius, §19's termination codes 0-6 -- with the additive chart.
// G supplies cost(p) and linearise(p, acc) over the track's blocks as values every lane of its 16-lane group holds bit
// for bit; acc is §19's 14 sums with the fourth direction zero, so lm_step<4> solves the 3x3 system (its fourth pivot is
// the clamp's 1e-12 / mu, its fourth step 0) and the fourth gradient sum never decides the zero-gradient test (§28)
struct BaPtOut {
  double p[3], cost0, cost1;
  int iters, code;
};
static_assert(sizeof(BaPtOut) == 48, "BaPtOut layout");

struct BaPointChart {
  static constexpr int kParams = 3, kStep = 4;
  static LT_HD void retract(const double p[3], const double dl[4], double out[3]) {
    for (int c = 0; c < 3; ++c) out[c] = p[c] + dl[c];
  }
};
// a constant track reports kRfConstant before a start that is not finite
template <class G>
LT_HD void ba_point_lm(G &grp, bool constant, int max_iter, double p[3], double *cost0, double *cost1, int *iters, int *code_out) {
  const double F = grp.cost(p);
  *cost0 = F;
  if (constant) lm_skip(F, kRfConstant, cost1, iters, code_out);
  else if (!(F <= kMaxDist)) lm_skip(F, kRfEvalFailed, cost1, iters, code_out);
  else lm_loop<BaPointChart>(grp, F, max_iter, p, cost1, iters, code_out);
}
// lane `lane` of a point track's group: its blocks' terms of the cost, and of §19's sums at p
LT_HD double ba_point_cost_part(const BaDev &d, const BaStruct &st, int lane, const double p[3]) {
  const double sp[6] = {p[0], p[1], p[2], 0.0, 0.0, 0.0};
  double s = 0.0;
  for (int i = lane; i < st.nb; i += kBaWidth) {
    const BaBlk b = d.blk[st.b0 + i];
    s = s + ba_cost_term(b, d.kvec + 4 * b.cam, ba_pose(d, 0, b.cam), sp, d.alpha);
  }
  return s;
}
LT_HD void ba_point_lin_part(const BaDev &d, const BaStruct &st, int lane, const double p[3], double part[kRfSums]) {
  const double sp[6] = {p[0], p[1], p[2], 0.0, 0.0, 0.0};
  for (int c = 0; c < kRfSums; ++c) part[c] = 0.0;
  for (int i = lane; i < st.nb; i += kBaWidth) {
    const BaBlk b = d.blk[st.b0 + i];
    double r[2], J[2][4];
    ba_pass<3>(b, d.kvec + 4 * b.cam, ba_pose(d, 0, b.cam), sp, d.alpha, 2, r, J);
    const double rho1 = ba_rho1(b, r[0] * r[0] + r[1] * r[1]);
    lm_block_add<2, 4>(r, rho1, J, part);
  }
}
// the group of a point track over the lanes.  The host twin runs it over LmHostLanes; k_ba_point_lm keeps a device
// group of its own over the same two parts
template <class Lanes>
struct BaPointGroup {
  Lanes lanes;
  const BaDev &d;
  const BaStruct &st;
  LT_HD double cost(const double p[3]) const {
    double s;
    lanes.template sum<1>(1, [&](int l, double *a) { a[0] = ba_point_cost_part(d, st, l, p); }, &s);
    return 0.5 * s;
  }
  LT_HD void linearise(const double p[3], double acc[kRfSums]) const {
    lanes.template sum<kRfSums>(kRfSums, [&](int l, double *a) { ba_point_lin_part(d, st, l, p, a); }, acc);
  }
};

// the launches of lt_kernels_ba.hip; every kernel reads the status record and returns at once when the solve has ended
void launch_ba_init(hipStream_t st, const BaDev &dev);     // the cost at the initial point, then k_ba_decide's first call
void launch_ba_attempt(hipStream_t st, const BaDev &dev, hipEvent_t *ev);  // one attempt; ev: 10 events around the kernels, or null
void launch_ba_points(hipStream_t st, const BaDev &dev, int max_iter, BaPtOut *out);  // constant poses: k_ba_point_lm

}  // namespace lt
