// lt_loc.h -- records and the FP64 expressions shared by the host side (lt_loc.cpp) and the device side
// (lt_kernels_loc.hip) of the point-line pose refinement: limap.optimize.solve_jointloc / solve_lineloc, the core of
// runners/hybrid_localization.py with `ransac.method: null`.  Every problem refines one camera pose
// (6 degrees of freedom, constant intrinsics) from 2D-3D line and point correspondences.  Both sides compile the same
// inline functions with -ffp-contract=off, so the device and lt_fn_loc_host agree bit for bit.
//
// limap's own part is restated in its operation order: paths relative to src/limap,
//   ceresbase/point_projection.h:8-57                          CamFromImg, ImgFromCam, PixelToWorld, WorldToPixel
//   ceresbase/line_dists.h:8-28                                CeresComputeDist2D_sine / _cosine
//   optimize/hybrid_localization/cost_functions.h:29-62        Ceres_Compute2DWeight (alpha is always 10: Create does
//                                                              not pass it on, :213-234, :282)
//   optimize/hybrid_localization/cost_functions.h:64-117       the four 2D distances
//   optimize/hybrid_localization/cost_functions.h:122-194      the two 3D distances
//   optimize/hybrid_localization/cost_functions.h:204-347      ReprojectionLineFunctor, ReprojectionPointFunctor
//   optimize/hybrid_localization/hybrid_localization.cc:91-134 JointLocEngine::AddResiduals: the blocks' order and weights
//   optimize/hybrid_localization/hybrid_localization.h:36-40   points_3d_dist follows the 3D cost functions
// ASSUMPTIONS of the same kind as lt_svd.h and lt_refine.h (the libraries are not part of limap; their published
// procedures are followed): Ceres' QuaternionRotatePoint (the scale 1 / |q|, then UnitQuaternionRotatePoint in its
// cross-product form, rotation.h of Ceres 2.1 and later), Eigen's `q.conjugate() * v` (uv = 2 vec x v, then
// v + w uv + vec x uv, no normalisation), Ceres' CrossProduct and DotProduct (summed left to right), pow(x, 2) as x x,
// TrivialLoss, HuberLoss, SoftLOneLoss, CauchyLoss and ScaledLoss as loss_function.cc evaluates them, with rho'' <= 0 for
// all four so that the corrector is the scaling by rho' (DESIGN §19), and the Jet rules d|x|/dx = +1 at 0, derivative 0
// at a clamp.  The minimiser is §19's Levenberg-Marquardt definition with six unknowns, not Ceres' iterates.
#pragma once

#include "lt_refine.h"

namespace lt {

constexpr int kLcWidth = 64;    // lanes per problem: one wave64 (the choice: DESIGN §25)
constexpr int kLcFields = 12;   // doubles per residual block (SoA): s3d[3], e3d[3], s2d[2], e2d[2], loss weight, kind
constexpr int kLcSums = 27;     // H upper triangle by rows (21), then g (6)
static_assert(kLcSums == lm_sums(6), "the sums of six unknowns");
constexpr double kLcEps8 = 1e-8;  // upstream's `+ 1e-8`
constexpr double kLcAlpha = 10.0; // Ceres_Compute2DWeight's default, which every caller gets
constexpr double kLcDblMin = 2.2250738585072014e-308;

enum LcCost : int { kLcMidpoint2 = 0, kLcMidpointAngle3 = 1, kLcPerp2 = 2, kLcPerp4 = 3, kLcLineLine2 = 4, kLcPlaneLine2 = 5 };
enum LcWeight : int { kLcNone = 0, kLcCosine = 1, kLcLine3dpp = 2, kLcLength = 3, kLcInvLength = 4 };
enum LcLoss : int { kLcTrivial = 0, kLcHuber = 1, kLcSoftLOne = 2, kLcCauchy = 3 };
// termination codes: RfCode's 0-4 and 6 (the cost at the initial pose is not finite: the pose is kept), and
constexpr int kLcNoResiduals = 7;  // a problem without residual blocks: Solve() returns false upstream, the pose is kept

// what a call fixes for all of its problems
struct LcCfg {
  int cost, weight, loss, points_3d_dist;
  double loss_a;
  int max_iter, pad_;
};

// a problem: blocks [b0, b0 + n) of the call's block table, its lines first
struct LcProb {
  long long b0;
  int n, n_res;  // n_res: the number of residuals (GetInitialCost / GetFinalCost divide by it)
};
static_assert(sizeof(LcProb) == 16, "LcProb layout");

// per problem result
struct LcOut {
  double q[4], t[3];
  double cost0, cost1;
  int iters, code;
};
static_assert(sizeof(LcOut) == 80, "LcOut layout");

// the forward-mode scalar (lt_lm.h).  A linearisation runs the chain twice with three directions -- the rotation's with
// the translation a plain double, then the reverse -- so that no expression carries six derivatives
typedef Jet<3> Lc3;

// ---- point_projection.h ----
// WorldToPixel (:45-57)
template <class TQ, class TT, class T>
LT_HD void lc_world_to_pixel(const double k[4], const TQ q[4], const TT t[3], const double xyz[3], T xy[2]) {
  TQ r[3];
  lm_rotate<TQ, double>(q, xyz, r);
  const T p2 = r[2] + t[2];
  const T u = (r[0] + t[0]) / p2, v = (r[1] + t[1]) / p2;
  xy[0] = k[0] * u + k[2];
  xy[1] = k[1] * v + k[3];
}

// PixelToWorld (:30-43): Eigen's q.conjugate() * (local * depth - t)
template <class TQ, class TT, class T>
LT_HD void lc_pixel_to_world(const double k[4], const TQ q[4], const TT t[3], double x, double y, double depth, T out[3]) {
  const double u = (x - k[2]) / k[0], v = (y - k[3]) / k[1];
  const TT l0 = u * depth - t[0], l1 = v * depth - t[1], l2 = 1.0 * depth - t[2];
  const TQ vx = -q[1], vy = -q[2], vz = -q[3];
  T uv0 = vy * l2 - vz * l1, uv1 = vz * l0 - vx * l2, uv2 = vx * l1 - vy * l0;
  uv0 = uv0 + uv0; uv1 = uv1 + uv1; uv2 = uv2 + uv2;
  out[0] = (l0 + q[0] * uv0) + (vy * uv2 - vz * uv1);
  out[1] = (l1 + q[0] * uv1) + (vz * uv0 - vx * uv2);
  out[2] = (l2 + q[0] * uv2) + (vx * uv1 - vy * uv0);
}

// ---- line_dists.h:8-28 (EPS = 1e-12) ----
template <class T, class A, class B>
LT_HD T lc_sine(const A a[2], const B b[2]) {
  const A n1 = rf_sqrt((a[0] * a[0] + a[1] * a[1]) + kEps);
  const B n2 = rf_sqrt((b[0] * b[0] + b[1] * b[1]) + kEps);
  T s = rf_abs((a[0] * b[1] - a[1] * b[0]) / (n1 * n2));
  if (rf_val(s) > 1.0) rf_set(s, 1.0);
  return s;
}
template <class T, class A, class B>
LT_HD T lc_cosine(const A a[2], const B b[2]) {
  const A n1 = rf_sqrt((a[0] * a[0] + a[1] * a[1]) + kEps);
  const B n2 = rf_sqrt((b[0] * b[0] + b[1] * b[1]) + kEps);
  T c = rf_abs((a[0] * b[0] + a[1] * b[1]) / (n1 * n2));
  if (rf_val(c) > 1.0) rf_set(c, 1.0);
  return c;
}

// a residual block as the kernels read it
struct LcBlk {
  double s3[3], e3[3], s2[2], e2[2], w;
  int kind;  // 0 line, 1 point (s3 = the 3D point, s2 = the 2D point)
};
LT_HD LcBlk lc_load(const double *tab, long long stride, long long i) {
  LcBlk b;
  for (int c = 0; c < 3; ++c) { b.s3[c] = tab[(long long)c * stride + i]; b.e3[c] = tab[(long long)(3 + c) * stride + i]; }
  for (int c = 0; c < 2; ++c) { b.s2[c] = tab[(long long)(6 + c) * stride + i]; b.e2[c] = tab[(long long)(8 + c) * stride + i]; }
  b.w = tab[10 * stride + i];
  b.kind = tab[11 * stride + i] != 0.0 ? 1 : 0;
  return b;
}
LT_HD int lc_num_res(int cost) { return cost == kLcPerp4 ? 4 : (cost == kLcMidpointAngle3 ? 3 : 2); }

// Ceres_3DLineLineDist (cost_functions.h:122-155)
template <class TQ, class TT, class T>
LT_HD T lc_line_line(const double k[4], const TQ q[4], const TT t[3], const double p3d[3], const double dir3d[3],
                     const double p2d[2]) {
  T pa[3], pb[3], dir[3], n[3], d[3];
  lc_pixel_to_world<TQ, TT, T>(k, q, t, p2d[0], p2d[1], 1.0, pa);
  lc_pixel_to_world<TQ, TT, T>(k, q, t, p2d[0], p2d[1], 2.0, pb);
  for (int i = 0; i < 3; ++i) dir[i] = pb[i] - pa[i];
  n[0] = dir[1] * dir3d[2] - dir[2] * dir3d[1];
  n[1] = dir[2] * dir3d[0] - dir[0] * dir3d[2];
  n[2] = dir[0] * dir3d[1] - dir[1] * dir3d[0];
  const T nsq = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
  for (int i = 0; i < 3; ++i) d[i] = p3d[i] - pa[i];
  if (rf_val(nsq) <= kLcEps8) {
    T c[3];
    c[0] = dir[1] * d[2] - dir[2] * d[1];
    c[1] = dir[2] * d[0] - dir[0] * d[2];
    c[2] = dir[0] * d[1] - dir[1] * d[0];
    const T cc = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2], dd = (dir[0] * dir[0] + dir[1] * dir[1]) + dir[2] * dir[2];
    return rf_sqrt(cc / dd + kLcEps8);
  }
  const T dt = (n[0] * d[0] + n[1] * d[1]) + n[2] * d[2];
  return dt / rf_sqrt(nsq);
}

// ReprojectionLineFunctor::operator() (cost_functions.h:236-286); returns the number of residuals.  res: four slots, zero
// on entry -- the slots a form does not write stay zero, so that no loop over them depends on the form
template <class TQ, class TT, class T>
LT_HD int lc_line_residual(const LcCfg &cfg, const double k[4], const TQ q[4], const TT t[3], const LcBlk &b, T res[4]) {
  double dir3d[3] = {b.e3[0] - b.s3[0], b.e3[1] - b.s3[1], b.e3[2] - b.s3[2]};
  const double dn3 = sqrt(((dir3d[0] * dir3d[0] + dir3d[1] * dir3d[1]) + dir3d[2] * dir3d[2]) + kLcEps8);
  for (int i = 0; i < 3; ++i) dir3d[i] = dir3d[i] / dn3;
  const bool is3d = cfg.cost == kLcLineLine2 || cfg.cost == kLcPlaneLine2;
  T sr[2], er[2], dir2d[2] = {T(0.0), T(0.0)};
  // the reprojection reaches the residuals of the 2D distances and the cosine weight only
  if (!is3d || cfg.weight == kLcCosine) {
    lc_world_to_pixel<TQ, TT, T>(k, q, t, b.s3, sr);
    lc_world_to_pixel<TQ, TT, T>(k, q, t, b.e3, er);
    dir2d[0] = er[0] - sr[0];
    dir2d[1] = er[1] - sr[1];
    const T dn = rf_sqrt((dir2d[0] * dir2d[0] + dir2d[1] * dir2d[1]) + kLcEps8);
    dir2d[0] = dir2d[0] / dn;
    dir2d[1] = dir2d[1] / dn;
  }
  int n = 2;
  switch (cfg.cost) {
    case kLcMidpoint2:
    case kLcMidpointAngle3: {
      const T m0 = (sr[0] + er[0]) * 0.5, m1 = (sr[1] + er[1]) * 0.5;
      const double c0 = 0.5 * (b.s2[0] + b.e2[0]), c1 = 0.5 * (b.s2[1] + b.e2[1]);
      res[0] = m0 - c0;
      res[1] = m1 - c1;
      if (cfg.cost == kLcMidpointAngle3) {
        T d1[2] = {er[0] - sr[0], er[1] - sr[1]};
        const T n1 = rf_sqrt((d1[0] * d1[0] + d1[1] * d1[1]) + kLcEps8);
        d1[0] = d1[0] / n1; d1[1] = d1[1] / n1;
        double d2[2] = {b.e2[0] - b.s2[0], b.e2[1] - b.s2[1]};
        const double n2 = sqrt((d2[0] * d2[0] + d2[1] * d2[1]) + kLcEps8);
        d2[0] = d2[0] / n2; d2[1] = d2[1] / n2;
        res[2] = n1 * lc_sine<T, T, double>(d1, d2);
        n = 3;
      }
      break;
    }
    case kLcPerp2:
    case kLcPerp4: {
      const T disp1[2] = {b.s2[0] - sr[0], b.s2[1] - sr[1]}, disp2[2] = {b.e2[0] - sr[0], b.e2[1] - sr[1]};
      const T s1 = lc_sine<T, T, T>(dir2d, disp1), s2 = lc_sine<T, T, T>(dir2d, disp2);
      const T r0 = disp1[0] * s1, r1 = disp1[1] * s1, r2 = disp2[0] * s2, r3 = disp2[1] * s2;
      if (cfg.cost == kLcPerp4) {
        res[0] = r0; res[1] = r1; res[2] = r2; res[3] = r3;
        n = 4;
      } else {
        res[0] = rf_sqrt((r0 * r0 + r1 * r1) + kLcEps8);
        res[1] = rf_sqrt((r2 * r2 + r3 * r3) + kLcEps8);
      }
      break;
    }
    case kLcLineLine2:
      res[0] = lc_line_line<TQ, TT, T>(k, q, t, b.s3, dir3d, b.s2);
      res[1] = lc_line_line<TQ, TT, T>(k, q, t, b.s3, dir3d, b.e2);
      break;
    default: {  // kLcPlaneLine2 (cost_functions.h:165-194)
      T p1a[3], p1b[3], p2a[3], p2b[3], d1[3], d2[3], nn[3];
      lc_pixel_to_world<TQ, TT, T>(k, q, t, b.s2[0], b.s2[1], 1.0, p1a);
      lc_pixel_to_world<TQ, TT, T>(k, q, t, b.s2[0], b.s2[1], 2.0, p1b);
      lc_pixel_to_world<TQ, TT, T>(k, q, t, b.e2[0], b.e2[1], 1.0, p2a);
      lc_pixel_to_world<TQ, TT, T>(k, q, t, b.e2[0], b.e2[1], 2.0, p2b);
      for (int i = 0; i < 3; ++i) { d1[i] = p1b[i] - p1a[i]; d2[i] = p2b[i] - p2a[i]; }
      nn[0] = d1[1] * d2[2] - d1[2] * d2[1];
      nn[1] = d1[2] * d2[0] - d1[0] * d2[2];
      nn[2] = d1[0] * d2[1] - d1[1] * d2[0];
      const T nsq = (nn[0] * nn[0] + nn[1] * nn[1]) + nn[2] * nn[2];
      const T ds0 = b.s3[0] - p1a[0], ds1 = b.s3[1] - p1a[1], ds2 = b.s3[2] - p1a[2];
      const T de0 = b.e3[0] - p1a[0], de1 = b.e3[1] - p1a[1], de2 = b.e3[2] - p1a[2];
      res[0] = ((nn[0] * ds0 + nn[1] * ds1) + nn[2] * ds2) / rf_sqrt(nsq);
      res[1] = ((nn[0] * de0 + nn[1] * de1) + nn[2] * de2) / rf_sqrt(nsq);
      break;
    }
  }
  // Ceres_Compute2DWeight (cost_functions.h:29-62); ENoneWeight multiplies by 1.0, which changes no bit
  const double direc[2] = {b.e2[0] - b.s2[0], b.e2[1] - b.s2[1]};
  if (cfg.weight == kLcCosine) {
    const T w = rf_exp((1.0 - lc_cosine<T, T, double>(dir2d, direc)) * kLcAlpha);
    for (int i = 0; i < 4; ++i) res[i] = res[i] * w;
  } else if (cfg.weight == kLcLength || cfg.weight == kLcInvLength) {
    double w = sqrt((direc[0] * direc[0] + direc[1] * direc[1]) + kLcEps8);
    if (cfg.weight == kLcInvLength) w = 1.0 / w;
    for (int i = 0; i < 4; ++i) res[i] = res[i] * w;
  }
  return n;
}

// ReprojectionPointFunctor::operator() (cost_functions.h:309-341): always two residuals
template <class TQ, class TT, class T>
LT_HD int lc_point_residual(const LcCfg &cfg, const double k[4], const TQ q[4], const TT t[3], const LcBlk &b, T res[4]) {
  if (cfg.points_3d_dist) {
    T pa[3], pb[3], dir[3], d[3];
    lc_pixel_to_world<TQ, TT, T>(k, q, t, b.s2[0], b.s2[1], 1.0, pa);
    lc_pixel_to_world<TQ, TT, T>(k, q, t, b.s2[0], b.s2[1], 2.0, pb);
    for (int i = 0; i < 3; ++i) dir[i] = pb[i] - pa[i];
    const T dn = rf_sqrt(((dir[0] * dir[0] + dir[1] * dir[1]) + dir[2] * dir[2]) + kLcEps8);
    for (int i = 0; i < 3; ++i) { dir[i] = dir[i] / dn; d[i] = b.s3[i] - pa[i]; }
    const T dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2], dp = (d[0] * dir[0] + d[1] * dir[1]) + d[2] * dir[2];
    res[0] = rf_sqrt((dd - dp * dp) + kLcEps8);
    res[1] = T(0.0);
  } else {
    T xy[2];
    lc_world_to_pixel<TQ, TT, T>(k, q, t, b.s3, xy);
    res[0] = xy[0] - b.s2[0];
    res[1] = xy[1] - b.s2[1];
  }
  return 2;
}
template <class TQ, class TT, class T>
LT_HD int lc_residual(const LcCfg &cfg, const double k[4], const TQ q[4], const TT t[3], const LcBlk &b, T res[4]) {
  return b.kind ? lc_point_residual<TQ, TT, T>(cfg, k, q, t, b, res) : lc_line_residual<TQ, TT, T>(cfg, k, q, t, b, res);
}

// ---- the losses of ceresbase/bindings.cc as Ceres' loss_function.cc evaluates them: rho(s) and rho'(s) ----
LT_HD void lc_loss(const LcCfg &cfg, double s, double *rho, double *rho1) {
  const double a = cfg.loss_a, b = a * a, c = 1.0 / b;
  switch (cfg.loss) {
    case kLcHuber:
      if (s > b) {
        const double r = sqrt(s), m = a / r;
        *rho = (2.0 * a) * r - b;
        *rho1 = m > kLcDblMin ? m : kLcDblMin;
      } else {
        *rho = s;
        *rho1 = 1.0;
      }
      break;
    case kLcSoftLOne: {
      const double tmp = sqrt(1.0 + s * c), m = 1.0 / tmp;
      *rho = (2.0 * b) * (tmp - 1.0);
      *rho1 = m > kLcDblMin ? m : kLcDblMin;
      break;
    }
    case kLcCauchy: {
      const double sum = 1.0 + s * c, m = 1.0 / sum;
      *rho = b * lt_log(sum);
      *rho1 = m > kLcDblMin ? m : kLcDblMin;
      break;
    }
    default:
      *rho = s;
      *rho1 = 1.0;
  }
}

// the pose as the minimiser carries it: p = (q w x y z, t)
LT_HD void lc_seed_t(const double p[7], Lc3 t[3]) {
  for (int i = 0; i < 3; ++i) {
    t[i] = Lc3(p[4 + i]);
    t[i].d[i] = 1.0;
  }
}

// ScaledLoss(loss, w) over the squared norm of the block: its term of the cost (before the 1/2)
LT_HD double lc_cost_term(const LcCfg &cfg, const double k[4], const double p[7], const LcBlk &b) {
  double r[4] = {0.0, 0.0, 0.0, 0.0};
  lc_residual<double, double, double>(cfg, k, p, p + 4, b, r);
  double sq = 0.0;
  for (int i = 0; i < 4; ++i) sq = sq + r[i] * r[i];  // the unused slots add +0
  double rho, rho1;
  lc_loss(cfg, sq, &rho, &rho1);
  return b.w * rho;
}

// the sums of a block with NR residuals: every index is a compile-time constant, so J and r stay in registers
template <int NR>
LT_HD void lc_block_sums(const LcCfg &cfg, double w, const double J[4][6], const double r[4], double acc[kLcSums]) {
  double sq = 0.0;
  for (int i = 0; i < NR; ++i) sq = sq + r[i] * r[i];
  double rho, rho1;
  lc_loss(cfg, sq, &rho, &rho1);
  rho1 = w * rho1;
  int o = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j, ++o) {
      double s = 0.0;
      for (int m = 0; m < NR; ++m) s = s + J[m][i] * J[m][j];
      acc[o] = acc[o] + rho1 * s;
    }
  for (int i = 0; i < 6; ++i) {
    double s = 0.0;
    for (int m = 0; m < NR; ++m) s = s + J[m][i] * r[m];
    acc[21 + i] = acc[21 + i] + rho1 * s;
  }
}

// the block's part of H = sum rho' J^T J and g = sum rho' J^T r: the chain runs once for the rotation's three
// directions and once for the translation's.  res (tests): the block's residuals, 4 slots
LT_HD void lc_accumulate(const LcCfg &cfg, const double k[4], const double p[7], const LcBlk &b, double acc[kLcSums],
                         double *res = nullptr) {
  double J[4][6], r[4];
  int n;
  {
    Lc3 q[4], rr[4];
    for (int i = 0; i < 4; ++i) rr[i] = Lc3(0.0);
    lm_seed_quat(p, q);
    n = lc_residual<Lc3, double, Lc3>(cfg, k, q, p + 4, b, rr);
    for (int i = 0; i < 4; ++i) {
      r[i] = rr[i].v;
      for (int c = 0; c < 3; ++c) J[i][c] = rr[i].d[c];
    }
  }
  {
    Lc3 t[3], rr[4];
    for (int i = 0; i < 4; ++i) rr[i] = Lc3(0.0);
    lc_seed_t(p, t);
    lc_residual<double, Lc3, Lc3>(cfg, k, p, t, b, rr);
    for (int i = 0; i < 4; ++i)
      for (int c = 0; c < 3; ++c) J[i][3 + c] = rr[i].d[c];
  }
  if (res)
    for (int i = 0; i < n; ++i) res[i] = r[i];
  if (n == 2) lc_block_sums<2>(cfg, b.w, J, r, acc);
  else if (n == 3) lc_block_sums<3>(cfg, b.w, J, r, acc);
  else lc_block_sums<4>(cfg, b.w, J, r, acc);
}

// the chart of a pose: q+ = normalize((1, dq) (x) q), t+ = t + dt
struct LcChart {
  static constexpr int kParams = 7, kStep = 6;
  static LT_HD void retract(const double p[7], const double dl[6], double out[7]) {
    lm_retract_quat(p, dl, out);
    for (int i = 0; i < 3; ++i) out[4 + i] = p[4 + i] + dl[3 + i];
  }
};

// lm_loop with the pose as the unknown.  A problem without blocks is not optimised and its cost is not evaluated; one
// whose cost at the initial pose is not finite (a point in the camera's plane) ends with kRfEvalFailed; both keep the pose
template <class G>
LT_HD void lc_lm(G &grp, int n_blocks, int max_iter, double p[7], double *cost0, double *cost1, int *iters, int *code_out) {
  if (n_blocks <= 0) {
    *cost0 = 0.0;
    lm_skip(0.0, kLcNoResiduals, cost1, iters, code_out);
    return;
  }
  const double F = grp.cost(p);
  *cost0 = F;
  if (!(F <= kMaxDist)) lm_skip(F, kRfEvalFailed, cost1, iters, code_out);
  else lm_loop<LcChart>(grp, F, max_iter, p, cost1, iters, code_out);
}

// the group of a pose: blocks [b0, b0 + n) of a kLcFields table over the lanes (LmWaveLanes in the kernels, LmHostLanes
// in their host twins)
template <class Lanes>
struct LcGroup {
  Lanes lanes;
  const LcCfg &cfg;
  const double *tab;
  long long stride, b0;
  int n;
  const double *k;
  LT_HD double cost(const double p[7]) const {
    double s;
    lanes.template over<1>(n, 1, [&](int i, double *a) { a[0] = a[0] + lc_cost_term(cfg, k, p, lc_load(tab, stride, b0 + i)); }, &s);
    return 0.5 * s;
  }
  // res: 4 slots per block (tests)
  LT_HD void linearise_res(const double p[7], double acc[kLcSums], double *res) const {
    lanes.template over<kLcSums>(n, kLcSums, [&](int i, double *a) {
      lc_accumulate(cfg, k, p, lc_load(tab, stride, b0 + i), a, res ? res + 4 * (size_t)i : nullptr);
    }, acc);
  }
  LT_HD void linearise(const double p[7], double acc[kLcSums]) const { linearise_res(p, acc, nullptr); }
};

// ---- pose scoring: JointPoseEstimator::EvaluateModelOnPoint (estimators/absolute_pose/joint_pose_estimator.cc:176-251)
// for H poses x N correspondences, points first.  CameraView's members are lt_geom.h's (cam_build, cam_depth,
// cam_project, cam_ray); base/infinite_line.cc:55-71,151-163 and base/linebase.cc:20-27,93-98 are restated here ----
constexpr int kLcScoreFields = 16;  // doubles per correspondence (SoA): s3d[3], e3d[3], s2d[2], e2d[2], d[3], m[3]
// cos(1 degree) = 0.99984769515639123915701155881391..., rounded to nearest: 0x1.ffec097f5af8ap-1.  Upstream's
// `acos(|x|) 180 / pi < 1.0` is restated as |x| > this constant; an |x| above 1, whose arccosine is not a number and
// passes upstream's comparison, fails here -- its unprojection divides by the squared norm of a cross product of
// parallel vectors
constexpr double kLcCos1Deg = 0x1.ffec097f5af8ap-1;

struct LcScoreCfg {
  LcCfg cfg;                 // cost, weight = none, points_3d_dist
  double min_depth, overlap; // cheirality_min_depth, cheirality_overlap_pixels
  double thr2[2], w[2];      // squared inlier thresholds and data type weights: points, lines
  int n_points, n_lines;     // correspondences
  int want_msac, pad_;
};

// a correspondence as the scoring reads it; d, m: InfiniteLine3d(l3d), prepared once per call
struct LcItem {
  LcBlk b;
  d3 d, m;
};
LT_HD LcItem lc_load_item(const double *tab, long long stride, long long i, bool is_point) {
  LcItem it;
  for (int c = 0; c < 3; ++c) { it.b.s3[c] = tab[(long long)c * stride + i]; it.b.e3[c] = tab[(long long)(3 + c) * stride + i]; }
  for (int c = 0; c < 2; ++c) { it.b.s2[c] = tab[(long long)(6 + c) * stride + i]; it.b.e2[c] = tab[(long long)(8 + c) * stride + i]; }
  it.b.w = 1.0;
  it.b.kind = is_point ? 1 : 0;
  it.d = mk3(tab[10 * stride + i], tab[11 * stride + i], tab[12 * stride + i]);
  it.m = mk3(tab[13 * stride + i], tab[14 * stride + i], tab[15 * stride + i]);
  return it;
}
// InfiniteLine3d(Line3d) (infinite_line.cc:67-71); the caller has checked length > 0
LT_HD void lc_item_prep(const double l3[6], double d[3], double m[3]) {
  const d3 s = mk3(l3[0], l3[1], l3[2]);
  const d3 dir = unit(sub(mk3(l3[3], l3[4], l3[5]), s));
  const d3 mo = cross(s, dir);
  d[0] = dir.x; d[1] = dir.y; d[2] = dir.z;
  m[0] = mo.x; m[1] = mo.y; m[2] = mo.z;
}
// project_from_infinite_line (infinite_line.cc:151-163): the point of (l1, m1) nearest to (l2, m2)
LT_HD d3 lc_project_from(d3 l1, d3 m1, d3 l2, d3 m2) {
  const d3 c = cross(l1, l2);
  const d3 a = cross(m1, cross(l2, c));
  const double s = dot(m2, c), n = sqn(c);
  return mk3((-a.x + s * l1.x) / n, (-a.y + s * l1.y) / n, (-a.z + s * l1.z) / n);
}
// Line2d::point_projection (linebase.cc:20-27) on the segment ps - pe
LT_HD d2 lc_seg_projection(d2 ps, d2 pe, d2 p) {
  const d2 dir = unit(sub(pe, ps));
  const double len = sqrt(sqn(sub(ps, pe)));
  const double pr = dot(sub(p, ps), dir);
  if (pr < 0.0) return ps;
  if (pr > len) return pe;
  return add(ps, scale(dir, pr));
}
// the pose of a hypothesis: CameraPose's constructor normalises the quaternion once; nan: cheirality_test_point's
// isnan(qvec.norm()) || isnan(tvec.norm())
struct LcPose {
  Cam cam;
  double p[7];
  bool nan;
};
LT_HD void lc_pose_build(const double k[4], const double q4[4], const double t3[3], LcPose *ps) {
  lm_normalise_q(q4, ps->p);
  for (int i = 0; i < 3; ++i) ps->p[4 + i] = t3[i];
  const double qn = sqrt((ps->p[0] * ps->p[0] + ps->p[2] * ps->p[2]) + (ps->p[1] * ps->p[1] + ps->p[3] * ps->p[3]));
  const double tn = sqrt((t3[0] * t3[0] + t3[1] * t3[1]) + t3[2] * t3[2]);
  ps->nan = qn != qn || tn != tn;
  cam_build(k, q4, t3, &ps->cam);
}
// EvaluateModelOnPoint: the squared error of correspondence `it` under the pose, DBL_MAX where a cheirality test fails
LT_HD double lc_score_cell(const LcScoreCfg &sc, const double k[4], const LcPose &ps, const LcItem &it) {
  if (ps.nan) return kMaxDist;
  double r[4] = {0.0, 0.0, 0.0, 0.0};
  if (it.b.kind) {
    if (!(cam_depth(ps.cam, mk3(it.b.s3[0], it.b.s3[1], it.b.s3[2])) >= sc.min_depth)) return kMaxDist;
    lc_point_residual<double, double, double>(sc.cfg, k, ps.p, ps.p + 4, it.b, r);
    return r[0] * r[0] + r[1] * r[1];
  }
  // cheirality_test_line (:216-251)
  const d3 C = cam_center(ps.cam);
  const d2 s2 = mk2(it.b.s2[0], it.b.s2[1]), e2 = mk2(it.b.e2[0], it.b.e2[1]);
  const d3 rs = cam_ray(ps.cam, s2), re = cam_ray(ps.cam, e2);
  if (fabs(dot(rs, it.d)) > kLcCos1Deg) return kMaxDist;
  if (fabs(dot(re, it.d)) > kLcCos1Deg) return kMaxDist;
  const d3 p_start = lc_project_from(it.d, it.m, rs, cross(C, rs));
  if (!(cam_depth(ps.cam, p_start) >= sc.min_depth)) return kMaxDist;
  const d3 p_end = lc_project_from(it.d, it.m, re, cross(C, re));
  if (!(cam_depth(ps.cam, p_end) >= sc.min_depth)) return kMaxDist;
  const d2 a = cam_project(ps.cam, mk3(it.b.s3[0], it.b.s3[1], it.b.s3[2]));
  const d2 b = cam_project(ps.cam, mk3(it.b.e3[0], it.b.e3[1], it.b.e3[2]));
  const d2 p1 = lc_seg_projection(a, b, s2), p2 = lc_seg_projection(a, b, e2);
  if (sqrt(sqn(sub(p1, p2))) < sc.overlap) return kMaxDist;
  const int n = lc_line_residual<double, double, double>(sc.cfg, k, ps.p, ps.p + 4, it.b, r);
  if (n == 4) return (r[0] * r[0] + r[2] * r[2]) + (r[1] * r[1] + r[3] * r[3]);  // Eigen's 4-vector squaredNorm
  return r[0] * r[0] + r[1] * r[1];
}
// ScoreModel's term of a correspondence (pl_absolute_pose_hybrid_ransac.h:338-358) and GetInliers' test (:360-393)
LT_HD double lc_msac_term(const LcScoreCfg &sc, int type, double r2) {
  return (r2 < sc.thr2[type] ? r2 : sc.thr2[type]) * sc.w[type];  // std::min(r2, thr2)
}
// ScoreModel of the pose (q4, t3) against correspondences [c0, c0 + n_pts + n_lines) of a kLcScoreFields table, the
// points first: the MSAC sum over the lanes, which every lane returns (0.0 where the call does not want it).
// each(i, is_point, r2) sees correspondence c0 + i's squared error first: the callers' stores and inlier counts
template <class Lanes, class Each>
LT_HD double lc_msac_sum(const Lanes &lanes, const LcScoreCfg &sc, const double k[4], const double q4[4], const double t3[3],
                         const double *tab, long long stride, long long c0, int n_pts, int n_lines, Each each) {
  LcPose ps;
  lc_pose_build(k, q4, t3, &ps);
  double sum;
  lanes.template over<1>(n_pts + n_lines, 1, [&](int i, double *a) {
    const bool is_point = i < n_pts;
    const double r2 = lc_score_cell(sc, k, ps, lc_load_item(tab, stride, c0 + i, is_point));
    each(i, is_point, r2);
    if (sc.want_msac) a[0] = a[0] + lc_msac_term(sc, is_point ? 0 : 1, r2);
  }, &sum);
  return sum;
}

struct LcScoreDev {
  const double *tab;  // kLcScoreFields x stride
  long long stride;
  const double *qvec, *tvec;  // per pose
  long long n_poses;
  double k[4];
  LcScoreCfg sc;
};
// table[h N + i]; per pose scores[h] and inliers[2 h + type] where the call wants the MSAC score
void launch_loc_score(hipStream_t st, const LcScoreDev &dev, double *table, double *scores, int *inliers);

// the call's tables on the device
struct LcDev {
  const LcProb *probs;
  long long n_probs;
  const double *tab;  // kLcFields x stride
  long long stride;
  const double *kvec;  // 4 per problem
  LcCfg cfg;
};

// out[i].q, out[i].t hold the initial poses (q normalised on the host) and receive the results
void launch_loc_lm(hipStream_t st, const LcDev &dev, LcOut *out);

// hybrid_localization.h:36-40: points_3d_dist follows the 3D cost functions; a trivial loss has no parameter
LT_HD LcCfg lc_cfg_of(int cost, int weight, int loss, double loss_a, int max_iter) {
  return LcCfg{cost, weight, loss, (cost == kLcLineLine2 || cost == kLcPlaneLine2) ? 1 : 0, loss == kLcTrivial ? 1.0 : loss_a, max_iter, 0};
}

}  // namespace lt

#ifndef __HIPCC__
// ---- the host's checks and table rows, shared by lt_loc.cpp and lt_est.cpp ----
#include "../../include/limap_amd.h"

#include <cmath>
#include <string>

namespace lt {

// a refinement configuration; 1 with msg: an argument error
inline int lc_check_config(const lt_loc_config *c, LcCfg &cfg, std::string &msg) {
  if (!c) { msg = "null configuration"; return 1; }
  if (c->cost_function < kLcMidpoint2 || c->cost_function > kLcPlaneLine2) { msg = "unknown line cost function"; return 1; }
  if (c->weight_function == kLcLine3dpp) { msg = "ELine3dppWeight is not built (it needs an arccosine)"; return 1; }
  if (c->weight_function < kLcNone || c->weight_function > kLcInvLength) { msg = "unknown line weight function"; return 1; }
  if (c->loss < kLcTrivial || c->loss > kLcCauchy) { msg = "unknown loss function"; return 1; }
  if (c->loss != kLcTrivial && !(c->loss_a > 0.0 && std::isfinite(c->loss_a))) { msg = "the loss parameter must be > 0"; return 1; }
  if (c->max_num_iterations < 0) { msg = "max_num_iterations is negative"; return 1; }
  if (!std::isfinite(c->weight_line) || !std::isfinite(c->weight_point) || c->weight_line < 0.0 || c->weight_point < 0.0) {
    msg = "weight_line and weight_point must be finite and >= 0";  // ScaledLoss with a negative scale is no loss
    return 1;
  }
  cfg = lc_cfg_of(c->cost_function, c->weight_function, c->loss, c->loss_a, c->max_num_iterations);
  return 0;
}

// row i of a kLcScoreFields table (zeroed by the caller) for a point correspondence
inline void lc_score_fill_point(double *tab, long long st, long long i, const double p3d[3], const double p2d[2]) {
  for (int k = 0; k < 3; ++k) tab[(long long)k * st + i] = p3d[k];
  tab[6 * st + i] = p2d[0];
  tab[7 * st + i] = p2d[1];
}
// ... and for the 2D segment seg of 3D line id of the n_l3d lines at line3d6.  dm, have: the pose-independent part of
// every 3D line (6 doubles) and whether it is there yet, where the caller keeps it; null: prepared per segment
inline int lc_score_fill_line(double *tab, long long st, long long i, long long n_l3d, const double *line3d6, long long id,
                              const double seg[4], double *dm, char *have, std::string &msg) {
  if (id < 0 || id >= n_l3d) { msg = "l3d_id " + std::to_string(id) + " is outside the " + std::to_string(n_l3d) + " 3D lines"; return 1; }
  const double *l3 = line3d6 + 6 * id;
  double own[6];
  double *pre = dm ? dm + 6 * id : own;
  if (!have || !have[id]) {
    const double dx = l3[3] - l3[0], dy = l3[4] - l3[1], dz = l3[5] - l3[2];
    if (!(std::sqrt((dx * dx + dy * dy) + dz * dz) > 0.0)) {  // CHECK_GT(line.length(), 0.0) (infinite_line.cc:68)
      msg = "3D line " + std::to_string(id) + " has zero length";
      return 1;
    }
    lc_item_prep(l3, pre, pre + 3);
    if (have) have[id] = 1;
  }
  for (int k = 0; k < 6; ++k) tab[(long long)k * st + i] = l3[k];
  for (int k = 0; k < 4; ++k) tab[(long long)(6 + k) * st + i] = seg[k];
  for (int k = 0; k < 6; ++k) tab[(long long)(10 + k) * st + i] = pre[k];
  return 0;
}

}  // namespace lt
#endif
